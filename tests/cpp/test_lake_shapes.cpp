// merge_tree_shapes of the C++ mirror (include/ws_watershed.hpp, ws_merge_tree_shapes) against a fold over the mirror's own
// transform_history_levels planes, by the definition of the records: record c over the pixels equal to c in the plane before c's
// death level (the last plane if it never died, the seed pixel alone if it died at level 0), record 0 over what the last plane
// leaves uncoloured -- image weights, u8 and u16 weight planes, with and without edge correction.  The tree and the statistics
// must be merge_tree_stats'.  Needs device 0.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/ws_watershed.hpp"
#include "../../oracle/ws_oracle.h"

namespace ws = rustronomy_watershed;

#define CHECK(cond)                                                        \
  do {                                                                     \
    if (!(cond)) { std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

static void add128(uint64_t s[2], unsigned __int128 t) {
  unsigned __int128 x = ((unsigned __int128)s[1] << 64 | s[0]) + t;
  s[0] = uint64_t(x);
  s[1] = uint64_t(x >> 64);
}

static void add(ws_lake_shape &s, uint64_t v, uint64_t r, uint64_t c) {
  add128(s.sum_wrr, (unsigned __int128)v * r * r); add128(s.sum_wcc, (unsigned __int128)v * c * c); add128(s.sum_wrc, (unsigned __int128)v * r * c);
  add128(s.sum_rr, (unsigned __int128)r * r); add128(s.sum_cc, (unsigned __int128)c * c); add128(s.sum_rc, (unsigned __int128)r * c);
}

// kind: 0 the image weighs, 1 a u8 plane, 2 a u16 plane (row stride cols + 5)
template <class W>
static int check(const W &watershed, size_t H, size_t Wd, unsigned seed, int kind, size_t shift = 0) {
  std::vector<uint8_t> img(H * Wd), w8(H * Wd);
  ws_or_random_field(img.data(), H, Wd, seed);
  ws_or_random_field(w8.data(), H, Wd, seed + 100);
  const size_t ws16 = Wd + 5;
  std::vector<uint16_t> w16(H * ws16, 7);
  for (size_t r = 0; r < H; ++r)
    for (size_t c = 0; c < Wd; ++c) w16[r * ws16 + c] = uint16_t(w8[r * Wd + c] * 257u);      // 0 .. 65535
  ws::ArrayView2<uint8_t> view(img.data(), H, Wd, Wd);
  const auto mins = watershed.find_local_minima(view);
  std::vector<uint8_t> all;
  for (unsigned l = 0; l <= watershed.max_water_level(); ++l) all.push_back((uint8_t)l);
  const auto planes = watershed.transform_history_levels(view, mins, all);
  const auto cat = kind == 0   ? watershed.merge_tree_shapes(view, mins, true)
                   : kind == 1 ? watershed.merge_tree_shapes(view, mins, ws::ArrayView2<uint8_t>(w8.data(), H, Wd, Wd), true)
                               : watershed.merge_tree_shapes(view, mins, ws::ArrayView2<uint16_t>(w16.data(), H, Wd, ws16), true);
  const auto plain = kind == 0   ? watershed.merge_tree_stats(view, mins, true)
                     : kind == 1 ? watershed.merge_tree_stats(view, mins, ws::ArrayView2<uint8_t>(w8.data(), H, Wd, Wd), true)
                                 : watershed.merge_tree_stats(view, mins, ws::ArrayView2<uint16_t>(w16.data(), H, Wd, ws16), true);
  const size_t S = mins.size(), levels = all.size();
  CHECK(cat.tree.nodes.size() == S + 1 && cat.stats.size() == S + 1 && cat.shapes.size() == S + 1 && plain.shapes.empty());
  CHECK(std::memcmp(cat.tree.nodes.data(), plain.tree.nodes.data(), (S + 1) * sizeof(ws_tree_node)) == 0);
  CHECK(std::memcmp(cat.stats.data(), plain.stats.data(), (S + 1) * sizeof(ws_lake_stats)) == 0);
  const size_t rows = cat.tree.labels.rows, cols = cat.tree.labels.cols, e = (rows - H) / 2;
  CHECK(rows == planes[0].second.rows && cols == planes[0].second.cols);
  std::vector<uint64_t> v(rows * cols, 0);      // v(p) over the padded plane
  for (size_t r = 0; r < H; ++r)
    for (size_t c = 0; c < Wd; ++c)
      v[(r + e) * cols + c + e] = kind == 0 ? img[r * Wd + c] : kind == 1 ? w8[r * Wd + c] : w16[r * ws16 + c];
  for (size_t c = 0; c <= S; ++c) {
    const ws_tree_node &n = cat.tree.nodes[c];
    ws_lake_shape want{};
    if (c != 0 && n.death_level == 0) {
      const size_t r = mins[c - 1].first + shift, x = mins[c - 1].second + shift;
      add(want, v[r * cols + x], r, x);
    } else {
      const size_t L = c == 0 || n.death_level == W::MergeTree::ALIVE ? levels - 1 : n.death_level - 1;
      const auto &plane = planes[L].second.data;
      for (size_t p = 0; p < rows * cols; ++p)
        if (plane[p] == c) add(want, v[p], p / cols, p % cols);
    }
    CHECK(std::memcmp(&cat.shapes[c], &want, sizeof want) == 0);
  }
  return 0;
}

int main() {
  static_assert(sizeof(ws_lake_shape) == 96, "ws_lake_shape is 96 bytes");
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_low = ws::TransformBuilder<>().set_max_water_lvl(60).build_merging();
  auto mer_e = ws::TransformBuilder<>().enable_edge_correction().shift_seeds_into_padded_plane().build_merging();
  auto mer_p = ws::TransformBuilder<>().set_max_water_lvl(200).enable_edge_correction().build_merging();
  if (check(mer, 96, 80, 4, 0) || check(mer, 96, 80, 4, 2) || check(mer_low, 70, 53, 6, 1) || check(mer_e, 64, 75, 7, 2, 1) ||
      check(mer_e, 64, 75, 7, 0, 1) || check(mer_p, 40, 44, 8, 1))
    return 1;
  bool threw = false;
  try {
    std::vector<uint8_t> img(64, 3), wt(72, 1);
    mer.merge_tree_shapes(ws::ArrayView2<uint8_t>(img.data(), 8, 8, 8), {}, ws::ArrayView2<uint8_t>(wt.data(), 8, 9, 9));
  } catch (const std::invalid_argument &) { threw = true; }
  if (!threw) { std::printf("FAIL a weight plane of another shape was taken\n"); return 1; }
  std::printf("lake shapes ok\n");
  return 0;
}
