// The cut catalogue of the C++ mirror (include/ws_watershed.hpp, ws_merge_tree_cut_catalogue) against a host walk and fold over
// the mirror's own merge_tree_stats: the table of cut_table(cut, stats), along `parent` while the node dies no later than
// max(arrival level, merge_level), and every pixel folded into the record of the node it ends on -- sums, box, extrema and the
// first pixel of the largest weight, in the padded plane's coordinates, the ring weighing 0 under edge correction.
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
static int check(const W &watershed, size_t H, size_t Wd, unsigned seed, bool u16, bool edge) {
  std::vector<uint8_t> img(H * Wd);
  ws_or_random_field(img.data(), H, Wd, seed);
  ws::ArrayView2<uint8_t> view(img.data(), H, Wd, Wd);
  std::vector<uint16_t> wt(H * Wd);
  for (size_t p = 0; p < wt.size(); ++p) wt[p] = (uint16_t)((p * 40503u + 17u * seed) & 0xFFFFu);
  ws::ArrayView2<uint16_t> wview(wt.data(), H, Wd, Wd);
  const auto mins = watershed.find_local_minima(view);
  std::vector<uint8_t> all;
  for (unsigned l = 0; l <= watershed.max_water_level(); ++l) all.push_back((uint8_t)l);
  const auto planes = watershed.transform_history_levels(view, mins, all);
  const auto cat = u16 ? watershed.merge_tree_stats(view, mins, wview, true) : watershed.merge_tree_stats(view, mins, true);
  const auto &tree = cat.tree;
  const size_t prow = tree.labels.rows, pcol = tree.labels.cols, npx = prow * pcol, levels = all.size(), off = edge ? 1 : 0;
  std::vector<uint64_t> sums;
  for (size_t c = 1; c < tree.nodes.size(); ++c)
    if (tree.nodes[c].death_level != W::MergeTree::ALIVE && tree.nodes[c].n_leaves) sums.push_back(cat.stats[c].sum_w);
  CHECK(sums.size() > 8);
  std::sort(sums.begin(), sums.end());
  const std::vector<ws_lake_cut> cuts = {W::lake_cut(sums[sums.size() / 2]), W::lake_cut(0, 0, 0, 4, 0, 254, 20), W::lake_cut(0, 0, 0, 0, 0, (uint8_t)(levels / 2), 30),
                                         W::lake_cut(), W::lake_cut(sums[sums.size() / 2])};
  const auto got = u16 ? watershed.tree_cut_catalogue(view, mins, cuts, wview) : watershed.tree_cut_catalogue(view, mins, cuts);
  CHECK(got.planes.size() == cuts.size() && got.offsets.size() == cuts.size() + 1 && got.hidden.size() == cuts.size());
  CHECK(got.hidden_stats.size() == cuts.size() && got.region_stats.size() == got.lakes.size() && got.offsets.back() == got.lakes.size());
  for (size_t c = 0; c < tree.nodes.size(); ++c) CHECK(same(got.stats[c], cat.stats[c]) && got.tree.nodes[c].parent == tree.nodes[c].parent);
  std::vector<uint32_t> arrival(npx, 255), weight(npx, 0);      // the first level that shows the pixel; the weights over the padded plane
  for (size_t p = 0; p < npx; ++p) {
    for (size_t l = 0; l < levels; ++l)
      if (planes[l].second.data[p]) { arrival[p] = (uint32_t)l; break; }
    const size_t r = p / pcol - off, c = p % pcol - off;      // (the ring wraps to far above H and Wd)
    if (r < H && c < Wd) weight[p] = u16 ? wt[r * Wd + c] : img[r * Wd + c];
  }
  size_t differ = 0;
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
      CHECK(got.planes[k].data[p] == at);
      fold(want[at], weight[p], (uint32_t)(p / pcol), (uint32_t)(p % pcol), (uint32_t)p);
      ++count[at];
    }
    CHECK(got.hidden[k] == count[0] && same(got.hidden_stats[k], want[0]));
    size_t i = got.offsets[k];
    for (size_t a = 1; a < count.size(); ++a)      // the records: every colour with pixels, in increasing colour
      if (count[a]) {
        CHECK(i < got.offsets[k + 1] && got.lakes[i].colour == a && got.lakes[i].area == count[a]);
        CHECK(same(got.region_stats[i], want[a]));
        differ += !same(got.region_stats[i], cat.stats[a]);
        ++i;
      }
    CHECK(i == got.offsets[k + 1]);
  }
  CHECK(differ > 0);      // a region is not the lake the hierarchy's catalogue measured
  for (size_t i = got.offsets[0], j = got.offsets[4]; i < got.offsets[1]; ++i, ++j)      // a repeated cut: identical records
    CHECK(same(got.region_stats[i], got.region_stats[j]) && got.lakes[i].colour == got.lakes[j].colour);
  CHECK(same(got.hidden_stats[0], got.hidden_stats[4]));
  return 0;
}

int main() {
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(100).enable_edge_correction().shift_seeds_into_padded_plane().build_merging();
  if (check(mer, 48, 52, 1, false, false) || check(mer_e, 40, 37, 2, true, true)) return 1;
  std::printf("cut catalogue ok\n");
  return 0;
}
