// The cut catalogue of a cube in the C++ mirror (include/ws_watershed.hpp, ws_merge_tree_cut_catalogue_batch) against a host walk
// and fold per slice over the mirror's own merge_tree_stats of that slice alone, in the pattern of test_cut_catalogue.cpp: the table
// of cut_table(cut, stats), along `parent` while the node dies no later than max(arrival level, merge_level), every pixel folded
// into the record of the node it ends on, in the slice's own plane; a slice without seeds shows nothing and hides its plane.
// Needs device 0.
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../../include/ws_watershed.hpp"
#include "../../oracle/ws_oracle.h"

namespace ws = rustronomy_watershed;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static ws_lake_stats nothing() { return ws_lake_stats{0, 0, 0, 0, 0, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u}; }

static void fold(ws_lake_stats &s, uint32_t v, uint32_t r, uint32_t c, uint32_t pixel) {      // pixels come in row-major order
  s.sum_w += v; s.sum_wr += (uint64_t)v * r; s.sum_wc += (uint64_t)v * c; s.sum_r += r; s.sum_c += c;
  s.r_min = std::min(s.r_min, r); s.r_max = std::max(s.r_max, r); s.c_min = std::min(s.c_min, c); s.c_max = std::max(s.c_max, c);
  s.w_min = std::min(s.w_min, v);
  if (s.peak_pixel == 0xFFFFFFFFu || v > s.w_max) { s.w_max = v; s.peak_pixel = pixel; }
}

static bool same(const ws_lake_stats &a, const ws_lake_stats &b) {
  return a.sum_w == b.sum_w && a.sum_wr == b.sum_wr && a.sum_wc == b.sum_wc && a.sum_r == b.sum_r && a.sum_c == b.sum_c && a.r_min == b.r_min &&
         a.r_max == b.r_max && a.c_min == b.c_min && a.c_max == b.c_max && a.w_min == b.w_min && a.w_max == b.w_max && a.peak_pixel == b.peak_pixel &&
         a.reserved == b.reserved;
}

template <class W>
static int check(const W &watershed, size_t S, size_t H, size_t Wd, unsigned seed, bool edge) {
  using Seed = typename std::decay<decltype(watershed.find_local_minima(ws::ArrayView2<uint8_t>(nullptr, 0, 0, 0))[0])>::type;
  const size_t hw = H * Wd, off = edge ? 1 : 0;
  std::vector<uint8_t> cube(S * hw);
  std::vector<uint16_t> wt(S * hw);
  for (size_t s = 0; s < S; ++s) ws_or_random_field(cube.data() + s * hw, H, Wd, seed + 7 * (unsigned)s);
  for (size_t p = 0; p < wt.size(); ++p) wt[p] = (uint16_t)((p * 40503u + 17u * seed) & 0xFFFFu);
  std::vector<std::vector<Seed>> seeds(S);
  for (size_t s = 0; s < S; ++s)
    if (s != 1) seeds[s] = watershed.find_local_minima(ws::ArrayView2<uint8_t>(cube.data() + s * hw, H, Wd, Wd));      // slice 1: no seed
  std::vector<uint8_t> all;
  for (unsigned l = 0; l <= watershed.max_water_level(); ++l) all.push_back((uint8_t)l);
  const size_t levels = all.size();
  const std::vector<ws_lake_cut> cuts = {W::lake_cut(), W::lake_cut(0, 0, 0, 4, 0, 254, 20), W::lake_cut(0, 0, 0, 0, 0, (uint8_t)(levels / 2), 30),
                                         W::lake_cut(300000), W::lake_cut()};
  const auto got = watershed.merge_tree_cut_catalogue_cube(cube.data(), S, H, Wd, cuts, wt.data(), &seeds);
  CHECK(got.size() == S);
  size_t shown = 0;
  for (size_t s = 0; s < S; ++s) {
    const auto &g = got[s];
    ws::ArrayView2<uint8_t> view(cube.data() + s * hw, H, Wd, Wd);
    ws::ArrayView2<uint16_t> wview(wt.data() + s * hw, H, Wd, Wd);
    CHECK(g.planes.size() == cuts.size() && g.offsets.size() == cuts.size() + 1 && g.hidden.size() == cuts.size() && g.offsets[0] == 0);
    CHECK(g.hidden_stats.size() == cuts.size() && g.region_stats.size() == g.lakes.size() && g.offsets.back() == g.lakes.size());
    const size_t prow = g.planes[0].rows, pcol = g.planes[0].cols, npx = prow * pcol;
    CHECK(prow == H + 2 * off && pcol == Wd + 2 * off);
    std::vector<uint32_t> weight(npx, 0);
    for (size_t p = 0; p < npx; ++p) {
      const size_t r = p / pcol - off, c = p % pcol - off;      // (the ring wraps to far above H and Wd)
      if (r < H && c < Wd) weight[p] = wt[s * hw + r * Wd + c];
    }
    if (seeds[s].empty()) {      // nothing shown: every cut hides the whole plane
      ws_lake_stats whole = nothing();
      for (size_t p = 0; p < npx; ++p) fold(whole, weight[p], (uint32_t)(p / pcol), (uint32_t)(p % pcol), (uint32_t)p);
      CHECK(g.lakes.empty() && g.tree.nodes.size() == 1);
      for (size_t k = 0; k < cuts.size(); ++k) {
        CHECK(g.hidden[k] == npx && same(g.hidden_stats[k], whole));
        for (size_t p = 0; p < npx; ++p) CHECK(g.planes[k].data[p] == 0);
      }
      continue;
    }
    const auto planes = watershed.transform_history_levels(view, seeds[s], all);
    const auto cat = watershed.merge_tree_stats(view, seeds[s], wview, true);
    const auto &tree = cat.tree;
    CHECK(g.tree.nodes.size() == tree.nodes.size());
    for (size_t c = 0; c < tree.nodes.size(); ++c) CHECK(same(g.stats[c], cat.stats[c]) && g.tree.nodes[c].parent == tree.nodes[c].parent);
    std::vector<uint32_t> arrival(npx, 255);      // the first level that shows the pixel
    for (size_t p = 0; p < npx; ++p)
      for (size_t l = 0; l < levels; ++l)
        if (planes[l].second.data[p]) { arrival[p] = (uint32_t)l; break; }
    for (size_t k = 0; k < cuts.size(); ++k) {
      const auto table = tree.cut_table(cuts[k], cat.stats);
      std::vector<ws_lake_stats> want(tree.nodes.size(), nothing());
      std::vector<uint64_t> count(tree.nodes.size(), 0);
      for (size_t p = 0; p < npx; ++p) {
        const size_t c = tree.labels.data[p];
        uint32_t at = 0;
        if (c != 0 && arrival[p] <= cuts[k].show_level) {
          const uint32_t until = std::max<uint32_t>(arrival[p], cuts[k].merge_level);
          at = table[c];
          while (tree.nodes[at].death_level <= until) at = tree.nodes[at].parent;
        }
        CHECK(g.planes[k].data[p] == at);
        fold(want[at], weight[p], (uint32_t)(p / pcol), (uint32_t)(p % pcol), (uint32_t)p);
        ++count[at];
      }
      CHECK(g.hidden[k] == count[0] && same(g.hidden_stats[k], want[0]));
      size_t i = g.offsets[k];
      for (size_t a = 1; a < count.size(); ++a)      // the records: every colour with pixels, in increasing colour
        if (count[a]) {
          CHECK(i < g.offsets[k + 1] && g.lakes[i].colour == a && g.lakes[i].area == count[a]);
          CHECK(same(g.region_stats[i], want[a]));
          ++i;
          ++shown;
        }
      CHECK(i == g.offsets[k + 1]);
    }
  }
  CHECK(shown > S);
  // seeds == nullptr: every slice's own minima, which are the lists above but for slice 1
  std::vector<size_t> n_seeds;
  const auto own = watershed.merge_tree_cut_catalogue_cube(cube.data(), S, H, Wd, cuts, wt.data(), nullptr, &n_seeds);
  CHECK(own.size() == S && n_seeds.size() == S);
  for (size_t s = 0; s < S; ++s) {
    if (s == 1) { CHECK(n_seeds[s] > 0 && !own[s].lakes.empty()); continue; }
    CHECK(n_seeds[s] == seeds[s].size() && own[s].lakes.size() == got[s].lakes.size() && own[s].offsets == got[s].offsets && own[s].hidden == got[s].hidden);
    for (size_t i = 0; i < own[s].lakes.size(); ++i)
      CHECK(own[s].lakes[i].colour == got[s].lakes[i].colour && own[s].lakes[i].area == got[s].lakes[i].area && same(own[s].region_stats[i], got[s].region_stats[i]));
    for (size_t k = 0; k < cuts.size(); ++k) CHECK(own[s].planes[k].data == got[s].planes[k].data);
  }
  return 0;
}

int main() {
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(100).enable_edge_correction().build_merging();
  // 8 x 16: the smallest planes that stack; 38 x 30 under edge correction: a 40 x 32 plane that stacks; 30 x 37: a loop
  if (check(mer, 9, 8, 16, 1, false) || check(mer_e, 4, 38, 30, 2, true) || check(mer, 3, 30, 37, 3, false)) return 1;
  std::printf("cut catalogue cube ok\n");
  return 0;
}
