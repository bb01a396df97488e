// tree_cut of the C++ mirror (include/ws_watershed.hpp, ws_merge_tree_cut) against a host walk over the mirror's own merge_tree:
// the table of cut_table(), then along `parent` while the node dies no later than max(arrival level, merge_level) -- the arrival
// level of a pixel being the first level whose history plane shows it.  The level cut is compared with the history plane.
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
static int check(const W &watershed, size_t H, size_t Wd, unsigned seed) {
  std::vector<uint8_t> img(H * Wd);
  ws_or_random_field(img.data(), H, Wd, seed);
  ws::ArrayView2<uint8_t> view(img.data(), H, Wd, Wd);
  const auto mins = watershed.find_local_minima(view);
  std::vector<uint8_t> all;
  for (unsigned l = 0; l <= watershed.max_water_level(); ++l) all.push_back((uint8_t)l);
  const auto planes = watershed.transform_history_levels(view, mins, all);
  const auto tree = watershed.merge_tree(view, mins, true);
  const size_t npx = tree.labels.rows * tree.labels.cols, levels = all.size();
  const uint8_t L = (uint8_t)std::min<size_t>(40, levels - 1);
  const std::vector<ws_tree_cut> cuts = {W::cut(12, 2, 254, 0), W::cut(0, 0, L, L), W::cut(5, 0, (uint8_t)(levels / 2), 30)};
  const auto got = watershed.tree_cut(view, mins, cuts);
  CHECK(got.planes.size() == cuts.size() && got.offsets.size() == cuts.size() + 1 && got.hidden.size() == cuts.size());
  CHECK(got.tree.nodes.size() == tree.nodes.size());
  for (size_t c = 0; c < tree.nodes.size(); ++c)
    CHECK(got.tree.nodes[c].parent == tree.nodes[c].parent && got.tree.nodes[c].death_level == tree.nodes[c].death_level &&
          got.tree.nodes[c].area == tree.nodes[c].area && got.tree.nodes[c].n_leaves == tree.nodes[c].n_leaves);
  std::vector<uint32_t> arrival(npx, 255);      // the first level that shows the pixel
  for (size_t p = 0; p < npx; ++p)
    for (size_t l = 0; l < levels; ++l)
      if (planes[l].second.data[p]) { arrival[p] = (uint32_t)l; break; }
  for (size_t k = 0; k < cuts.size(); ++k) {
    const auto table = tree.cut_table(cuts[k]);
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
  CHECK(got.offsets.back() == got.lakes.size());
  for (size_t p = 0; p < npx; ++p) CHECK(got.planes[1].data[p] == planes[L].second.data[p]);      // the level cut is the history plane
  return 0;
}

int main() {
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(100).enable_edge_correction().shift_seeds_into_padded_plane().build_merging();
  if (check(mer, 48, 52, 1) || check(mer_e, 40, 37, 2)) return 1;
  std::printf("tree cut ok\n");
  return 0;
}
