// tree_cut with catalogue thresholds of the C++ mirror (include/ws_watershed.hpp, ws_merge_tree_stats_cut) against a host walk over
// the mirror's own merge_tree_stats: the table of cut_table(cut, stats), then along `parent` while the node dies no later than
// max(arrival level, merge_level) -- the arrival level of a pixel being the first level whose history plane shows it.
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

template <class W>
static int check(const W &watershed, size_t H, size_t Wd, unsigned seed, bool u16) {
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
  const size_t npx = tree.labels.rows * tree.labels.cols, levels = all.size();
  // thresholds from the catalogue itself: the median dead node's sum and peak, a depth most nodes miss
  std::vector<uint64_t> sums;
  std::vector<uint32_t> peaks;
  for (size_t c = 1; c < tree.nodes.size(); ++c)
    if (tree.nodes[c].death_level != W::MergeTree::ALIVE && tree.nodes[c].n_leaves) { sums.push_back(cat.stats[c].sum_w); peaks.push_back(cat.stats[c].w_max); }
  CHECK(sums.size() > 8);
  std::sort(sums.begin(), sums.end());
  std::sort(peaks.begin(), peaks.end());
  const std::vector<ws_lake_cut> cuts = {W::lake_cut(sums[sums.size() / 2]), W::lake_cut(0, peaks[peaks.size() / 2], 0, 2, 0, 254, 20),
                                         W::lake_cut(0, 0, u16 ? 1 : 40, 0, 0, (uint8_t)(levels / 2), 30), W::lake_cut(),
                                         W::lake_cut(sums[sums.size() / 2] + 1, 0, 0, 0, 2)};
  const auto got = u16 ? watershed.tree_cut(view, mins, cuts, wview) : watershed.tree_cut(view, mins, cuts);
  CHECK(got.planes.size() == cuts.size() && got.offsets.size() == cuts.size() + 1 && got.hidden.size() == cuts.size());
  CHECK(got.tree.nodes.size() == tree.nodes.size() && got.stats.size() == cat.stats.size());
  for (size_t c = 0; c < tree.nodes.size(); ++c) {
    CHECK(got.tree.nodes[c].parent == tree.nodes[c].parent && got.tree.nodes[c].death_level == tree.nodes[c].death_level &&
          got.tree.nodes[c].area == tree.nodes[c].area && got.tree.nodes[c].n_leaves == tree.nodes[c].n_leaves);
    CHECK(got.stats[c].sum_w == cat.stats[c].sum_w && got.stats[c].w_min == cat.stats[c].w_min && got.stats[c].w_max == cat.stats[c].w_max &&
          got.stats[c].peak_pixel == cat.stats[c].peak_pixel && got.stats[c].sum_wr == cat.stats[c].sum_wr);
  }
  std::vector<uint32_t> arrival(npx, 255);      // the first level that shows the pixel
  for (size_t p = 0; p < npx; ++p)
    for (size_t l = 0; l < levels; ++l)
      if (planes[l].second.data[p]) { arrival[p] = (uint32_t)l; break; }
  size_t moved = 0;
  for (size_t k = 0; k < cuts.size(); ++k) {
    const auto table = tree.cut_table(cuts[k], cat.stats);
    const auto plain = tree.cut_table(W::cut(cuts[k].min_area, cuts[k].min_leaves, cuts[k].show_level, cuts[k].merge_level));
    for (size_t c = 0; c < table.size(); ++c) moved += table[c] != plain[c];
    CHECK(got.planes[k].rows == tree.labels.rows && got.planes[k].cols == tree.labels.cols);
    std::vector<uint64_t> count(tree.nodes.size(), 0);
    for (size_t p = 0; p < npx; ++p) {
      const size_t c = tree.labels.data[p];
      uint32_t want = 0;
      if (c != 0 && arrival[p] <= cuts[k].show_level) {
        const uint32_t until = std::max<uint32_t>(arrival[p], cuts[k].merge_level);
        want = table[c];
        while (tree.nodes[want].death_level <= until) want = tree.nodes[want].parent;
      }
      CHECK(got.planes[k].data[p] == want);
      ++count[want];
    }
    CHECK(got.hidden[k] == count[0]);
    size_t at = got.offsets[k];
    for (size_t a = 1; a < count.size(); ++a)      // the records: every colour with pixels, in increasing colour
      if (count[a]) {
        CHECK(at < got.offsets[k + 1] && got.lakes[at].colour == a && got.lakes[at].area == count[a]);
        ++at;
      }
    CHECK(at == got.offsets[k + 1]);
  }
  CHECK(moved > 0);      // the catalogue thresholds decide something
  CHECK(got.offsets.back() == got.lakes.size());
  // the cut without thresholds is tree_cut's
  const auto old = watershed.tree_cut(view, mins, std::vector<ws_tree_cut>{W::cut()});
  for (size_t p = 0; p < npx; ++p) CHECK(got.planes[3].data[p] == old.planes[0].data[p]);
  return 0;
}

int main() {
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(100).enable_edge_correction().shift_seeds_into_padded_plane().build_merging();
  if (check(mer, 48, 52, 1, false) || check(mer_e, 40, 37, 2, true)) return 1;
  std::printf("tree cut stats ok\n");
  return 0;
}
