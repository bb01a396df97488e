// merge_tree_shapes_cube of the C++ mirror (include/ws_watershed.hpp, ws_merge_tree_shapes_batch) against the mirror's own
// merge_tree_shapes slice by slice with that slice's weight plane: own minima and given seed lists, the cube itself, a u8 and a u16
// weight cube, a cube whose slices stack and one whose slices do not, with and without edge correction and labels.  Needs device 0.
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

template <class T>
static int same(const T &a, const T &b) {
  const size_t n = a.tree.nodes.size();
  CHECK(n == b.tree.nodes.size() && a.stats.size() == n && b.stats.size() == n && a.shapes.size() == n && b.shapes.size() == n);
  CHECK(std::memcmp(a.tree.nodes.data(), b.tree.nodes.data(), n * sizeof(ws_tree_node)) == 0);
  CHECK(std::memcmp(a.stats.data(), b.stats.data(), n * sizeof(ws_lake_stats)) == 0);
  CHECK(std::memcmp(a.shapes.data(), b.shapes.data(), n * sizeof(ws_lake_shape)) == 0);      // all twelve words of every record
  CHECK(a.tree.labels.rows == b.tree.labels.rows && a.tree.labels.cols == b.tree.labels.cols && a.tree.labels.data == b.tree.labels.data);
  return 0;
}

// kind: 0 the cube weighs, 1 a u8 cube, 2 a u16 cube
template <class W>
static int check(const W &watershed, size_t S, size_t H, size_t Wd, unsigned seed, int kind) {
  const size_t px = H * Wd;
  std::vector<uint8_t> cube(S * px), w8(S * px);
  for (size_t k = 0; k < S; ++k) {
    ws_or_random_field(cube.data() + k * px, H, Wd, seed + (unsigned)k);
    ws_or_random_field(w8.data() + k * px, H, Wd, seed + 100 + (unsigned)k);      // every slice weighs differently
  }
  std::vector<uint16_t> w16(S * px);
  for (size_t i = 0; i < S * px; ++i) w16[i] = uint16_t(w8[i] * 257u);      // 0 .. 65535
  std::vector<std::vector<ws::Seed>> mins;
  for (size_t k = 0; k < S; ++k) mins.push_back(watershed.find_local_minima(ws::ArrayView2<uint8_t>(cube.data() + k * px, H, Wd, Wd)));
  auto lists = mins;
  lists[1].clear();           // a slice without seeds owns its record 0 alone
  lists[2].resize(1);
  std::vector<size_t> counts;
  const auto own = kind == 0   ? watershed.merge_tree_shapes_cube(cube.data(), S, H, Wd, nullptr, true, &counts)
                   : kind == 1 ? watershed.merge_tree_shapes_cube(cube.data(), S, H, Wd, w8.data(), nullptr, true, &counts)
                               : watershed.merge_tree_shapes_cube(cube.data(), S, H, Wd, w16.data(), nullptr, true, &counts);
  const auto given = kind == 0   ? watershed.merge_tree_shapes_cube(cube.data(), S, H, Wd, &lists)
                     : kind == 1 ? watershed.merge_tree_shapes_cube(cube.data(), S, H, Wd, w8.data(), &lists)
                                 : watershed.merge_tree_shapes_cube(cube.data(), S, H, Wd, w16.data(), &lists);
  CHECK(own.size() == S && given.size() == S && counts.size() == S);
  for (size_t k = 0; k < S; ++k) {
    const ws::ArrayView2<uint8_t> view(cube.data() + k * px, H, Wd, Wd);
    const ws::ArrayView2<uint8_t> v8(w8.data() + k * px, H, Wd, Wd);
    const ws::ArrayView2<uint16_t> v16(w16.data() + k * px, H, Wd, Wd);
    CHECK(counts[k] == mins[k].size());
    if (kind == 0) {
      if (same(own[k], watershed.merge_tree_shapes(view, mins[k], true)) || same(given[k], watershed.merge_tree_shapes(view, lists[k]))) return 1;
    } else if (kind == 1) {
      if (same(own[k], watershed.merge_tree_shapes(view, mins[k], v8, true)) || same(given[k], watershed.merge_tree_shapes(view, lists[k], v8))) return 1;
    } else {
      if (same(own[k], watershed.merge_tree_shapes(view, mins[k], v16, true)) || same(given[k], watershed.merge_tree_shapes(view, lists[k], v16))) return 1;
    }
  }
  // the seedless slice: record 0 alone, over every pixel of its own padded plane in the slice's own rows and columns
  const uint64_t rows = own[0].tree.labels.rows, cols = own[0].tree.labels.cols;
  CHECK(given[1].shapes.size() == 1 && given[1].tree.nodes[0].area == rows * cols);
  CHECK(given[1].shapes[0].sum_rr[0] == cols * ((rows - 1) * rows * (2 * rows - 1) / 6) && given[1].shapes[0].sum_rr[1] == 0);
  CHECK(given[1].shapes[0].sum_cc[0] == rows * ((cols - 1) * cols * (2 * cols - 1) / 6) && given[1].shapes[0].sum_cc[1] == 0);
  CHECK(given[1].shapes[0].sum_rc[0] == (rows * (rows - 1) / 2) * (cols * (cols - 1) / 2));
  return 0;
}

int main() {
  auto mer = ws::TransformBuilder<>().build_merging();
  auto mer_e = ws::TransformBuilder<>().set_max_water_lvl(200).enable_edge_correction().build_merging();
  // 128 x 96 planes stack (126 x 94 padded to them); 130 x 98 run as the loop
  for (int kind = 0; kind < 3; ++kind)
    if (check(mer, 5, 128, 96, 40, kind) || check(mer_e, 4, 126, 94, 50, kind) || check(mer, 4, 130, 98, 60, kind)) return 1;
  if (check(mer_e, 3, 130, 98, 70, 2)) return 1;
  std::printf("lake shapes cube ok\n");
  return 0;
}
