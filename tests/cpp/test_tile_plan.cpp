// The cut of a tiled field (csrc/ws_tile_plan.hpp) on a CPU, exhaustively over small inputs.
//   a. tile_place() for h, w in 1..40 and py, px in 1..8: the owned rectangles tile the field once, held = owned + one pixel towards
//      every neighbour, neighbours are mutual, px = 1 is the row cut of distributed.py's tile_rows (written out below), fields
//      with fewer rows or columns than tiles are refused;
//   b. gather_layout(): the packed offsets are the running sum of the owned areas of the ranks that send, in rank order;
//   c. image_window() with and without edge correction: every image pixel lands in the owned region of exactly one rank at plane
//      position (r + o, c + o), no ring pixel comes from the image; a rank that owns only the ring row included;
//   d. first_seed_outside() and deal_seeds(): the range form and the seed-by-seed form name the same (pixel, colour) pairs on
//      lists whose rows never decrease, a halo-row seed goes to both ranks, wrapped and 2^31-scale coordinates are refused.
#include "../../rustronomy-watershed_amd/csrc/ws_tile_plan.hpp"

#include <cstdio>
#include <map>
#include <utility>

using namespace wsapi;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      if (++failures <= 20) {                                                \
        std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);          \
        std::printf(__VA_ARGS__);                                            \
        std::printf("\n");                                                   \
      }                                                                      \
    }                                                                        \
  } while (0)

// distributed.py's tile_rows: rank's owned rows [r0, r1) and held rows [lo, hi)
void tile_rows_py(size_t h, size_t rank, size_t world, size_t *r0, size_t *r1, size_t *lo, size_t *hi) {
  const size_t base = h / world, extra = h % world;
  *r0 = rank * base + (rank < extra ? rank : extra);
  *r1 = *r0 + base + (rank < extra ? 1 : 0);
  *lo = rank > 0 ? *r0 - 1 : *r0;
  *hi = rank < world - 1 ? *r1 + 1 : *r1;
}

void test_partition() {
  for (size_t h = 1; h <= 40; ++h)
    for (size_t w = 1; w <= 40; ++w)
      for (int py = 1; py <= 8; ++py)
        for (int px = 1; px <= 8; ++px) {
          const TileCut cut{h, w, py, px};
          TilePlace t;
          if (h < (size_t)py || w < (size_t)px) {
            for (int r = 0; r < py * px; ++r) CHECK(!tile_place(cut, r, &t), "%zux%zu in %dx%d rank %d accepted", h, w, py, px, r);
            continue;
          }
          CHECK(!tile_place(cut, -1, &t) && !tile_place(cut, py * px, &t), "a rank outside the grid accepted");
          std::vector<int> owner(h * w, -1);
          std::vector<TilePlace> all((size_t)(py * px));
          for (int r = 0; r < py * px; ++r) {
            CHECK(tile_place(cut, r, &all[(size_t)r]), "%zux%zu in %dx%d rank %d refused", h, w, py, px, r);
            const TilePlace &p = all[(size_t)r];
            CHECK(p.r1 > p.r0 && p.c1 > p.c0, "rank %d owns nothing", r);
            for (size_t y = p.r0; y < p.r1; ++y)
              for (size_t x = p.c0; x < p.c1; ++x) {
                CHECK(owner[y * w + x] == -1, "pixel (%zu, %zu) owned twice", y, x);
                owner[y * w + x] = r;
              }
            // held = owned + one pixel on every side that has a neighbour
            CHECK(p.lo == p.r0 - (p.nb[0] >= 0 ? 1 : 0) && p.hi == p.r1 + (p.nb[1] >= 0 ? 1 : 0), "held rows of rank %d", r);
            CHECK(p.clo == p.c0 - (p.nb[2] >= 0 ? 1 : 0) && p.chi == p.c1 + (p.nb[3] >= 0 ? 1 : 0), "held columns of rank %d", r);
            CHECK(p.h == p.hi - p.lo && p.w == p.chi - p.clo && p.own_at() == (p.r0 - p.lo) * p.w + (p.c0 - p.clo), "block of rank %d", r);
            CHECK((p.nb[0] < 0) == (p.r0 == 0) && (p.nb[1] < 0) == (p.r1 == h) && (p.nb[2] < 0) == (p.c0 == 0) && (p.nb[3] < 0) == (p.c1 == w),
                  "rank %d: a neighbour exactly where the field goes on", r);
          }
          for (size_t i = 0; i < h * w; ++i) CHECK(owner[i] >= 0, "pixel %zu owned by nobody", i);
          for (int r = 0; r < py * px; ++r) {
            const TilePlace &p = all[(size_t)r];
            const int back[4] = {1, 0, 3, 2};
            for (int d = 0; d < 4; ++d) {
              if (p.nb[d] < 0) continue;
              CHECK(p.nb[d] < py * px && all[(size_t)p.nb[d]].nb[back[d]] == r, "rank %d side %d: the neighbour does not point back", r, d);
              const TilePlace &q = all[(size_t)p.nb[d]];      // ... and shares the edge: same columns above / below, same rows left / right
              if (d < 2) CHECK(q.c0 == p.c0 && q.c1 == p.c1 && (d == 0 ? q.r1 == p.r0 : q.r0 == p.r1), "rank %d side %d: not adjacent", r, d);
              else CHECK(q.r0 == p.r0 && q.r1 == p.r1 && (d == 2 ? q.c1 == p.c0 : q.c0 == p.c1), "rank %d side %d: not adjacent", r, d);
            }
          }
          if (px == 1)
            for (int r = 0; r < py; ++r) {
              size_t r0, r1, lo, hi;
              tile_rows_py(h, (size_t)r, (size_t)py, &r0, &r1, &lo, &hi);
              const TilePlace &p = all[(size_t)r];
              CHECK(p.r0 == r0 && p.r1 == r1 && p.lo == lo && p.hi == hi && p.c0 == 0 && p.c1 == w && p.clo == 0 && p.chi == w && p.nb[2] < 0 && p.nb[3] < 0,
                    "%zu rows over %d ranks, rank %d: not the row cut", h, py, r);
            }
        }
  // row blocks of a field without columns are still blocks; tiles of one are not
  TilePlace t;
  CHECK(tile_place(TileCut{5, 0, 2, 1}, 1, &t) && t.w == 0 && t.h == 3, "row blocks of a field of no columns");
  CHECK(!tile_place(TileCut{5, 0, 1, 2}, 0, &t) && !tile_place(TileCut{0, 5, 1, 1}, 0, &t), "an empty cut accepted");
}

void test_gather_layout() {
  for (size_t h = 1; h <= 12; ++h)
    for (size_t w = 1; w <= 12; ++w)
      for (int py = 1; py <= 4 && (size_t)py <= h; ++py)
        for (int px = 1; px <= 4 && (size_t)px <= w; ++px) {
          GatherLayout l;
          CHECK(gather_layout(TileCut{h, w, py, px}, &l), "layout refused");
          const size_t world = (size_t)(py * px);
          CHECK(l.place.size() == world && l.at.size() == world + 1 && l.at[0] == 0 && l.at[1] == 0, "rank 0 sends nothing to itself");
          size_t sum = 0;
          for (size_t r = 1; r < world; ++r) {
            TilePlace t;
            tile_place(TileCut{h, w, py, px}, (int)r, &t);
            CHECK(l.at[r] == sum, "offset of rank %zu", r);
            sum += t.own_h() * t.own_w();
            CHECK(l.place[r].r0 == t.r0 && l.place[r].c1 == t.c1, "place of rank %zu", r);
          }
          CHECK(l.at[world] == sum && sum == h * w - l.place[0].own_h() * l.place[0].own_w(), "the table holds every pixel rank 0 does not own");
        }
  GatherLayout l;
  CHECK(!gather_layout(TileCut{3, 9, 4, 1}, &l), "a layout of a field that is too small");
}

void test_image_window() {
  for (int edge = 0; edge < 2; ++edge)
    for (size_t h = 1; h <= 9; ++h)
      for (size_t w = 1; w <= 9; ++w)
        for (int py = 1; py <= 6; ++py)
          for (int px = 1; px <= 4; ++px) {
            const size_t o = (size_t)edge, ph = h + 2 * o, pw = w + 2 * o;
            if (ph < (size_t)py || pw < (size_t)px) continue;
            // plane pixel -> (image pixel + 1) as the owning rank's block holds it after the window is copied in; 0: ring
            std::vector<size_t> plane(ph * pw, (size_t)-1);
            for (int r = 0; r < py * px; ++r) {
              TilePlace t;
              CHECK(tile_place(TileCut{ph, pw, py, px}, r, &t), "place");
              const ImageWindow v = image_window(t, h, w, edge != 0);
              std::vector<size_t> block(t.h * t.w, 0);
              CHECK(v.rows * v.cols == 0 || (v.dst_r + v.rows <= t.h && v.dst_c + v.cols <= t.w && v.src_r + v.rows <= h && v.src_c + v.cols <= w),
                    "the window leaves the block or the image");
              for (size_t y = 0; y < v.rows; ++y)
                for (size_t x = 0; x < v.cols; ++x) block[(v.dst_r + y) * t.w + v.dst_c + x] = (v.src_r + y) * w + v.src_c + x + 1;
              // every held pixel of the block is right, halo included
              for (size_t y = t.lo; y < t.hi; ++y)
                for (size_t x = t.clo; x < t.chi; ++x) {
                  const bool ring = y < o || y >= h + o || x < o || x >= w + o;
                  const size_t want = ring ? 0 : (y - o) * w + (x - o) + 1;
                  CHECK(block[(y - t.lo) * t.w + (x - t.clo)] == want, "edge %d %zux%zu %dx%d rank %d: plane pixel (%zu, %zu)", edge, h, w, py, px, r, y, x);
                }
              for (size_t y = t.r0; y < t.r1; ++y)
                for (size_t x = t.c0; x < t.c1; ++x) {
                  CHECK(plane[y * pw + x] == (size_t)-1, "owned twice");
                  plane[y * pw + x] = block[(y - t.lo) * t.w + (x - t.clo)];
                }
            }
            for (size_t y = 0; y < h; ++y)
              for (size_t x = 0; x < w; ++x) CHECK(plane[(y + o) * pw + x + o] == y * w + x + 1, "image pixel (%zu, %zu) is not at (r + o, c + o)", y, x);
            size_t from_image = 0;
            for (size_t v : plane) from_image += v != 0;
            CHECK(from_image == h * w, "a ring pixel holds an image pixel");
          }
  // rank 0 owns only the ring row: 3 image rows padded to 5 over 5 ranks
  TilePlace t;
  CHECK(tile_place(TileCut{5, 6, 5, 1}, 0, &t) && t.r0 == 0 && t.r1 == 1 && t.hi == 2, "place");
  const ImageWindow v = image_window(t, 3, 4, true);      // its halo row is image row 0
  CHECK(v.rows == 1 && v.cols == 4 && v.src_r == 0 && v.src_c == 0 && v.dst_r == 1 && v.dst_c == 1, "the ring-row rank's window");
  CHECK(tile_place(TileCut{5, 6, 5, 1}, 4, &t), "place");
  const ImageWindow u = image_window(t, 3, 4, true);
  CHECK(u.rows == 1 && u.src_r == 2 && u.dst_r == 0 && u.dst_c == 1, "the last ring-row rank's window");
}

using Pairs = std::multimap<std::pair<uint32_t, uint32_t>, uint32_t>;      // (local row, local column) -> colour

Pairs pairs_of(const SeedDeal &d) {
  Pairs p;
  for (size_t k = 0; k < d.n(); ++k) p.insert({{d.loc[2 * k], d.loc[2 * k + 1]}, d.explicit_colours ? d.col[k] : d.first_colour + (uint32_t)k});
  return p;
}

void check_deal(const char *name, const std::vector<uint64_t> &seeds, size_t ph, size_t pw, size_t shift, bool expect_sorted) {
  const size_t n = seeds.size() / 2;
  bool sorted = false;
  CHECK(first_seed_outside(seeds.data(), n, ph, pw, shift, &sorted) == n, "%s: a seed refused", name);
  CHECK(sorted == expect_sorted, "%s: rows_sorted", name);
  for (int py = 1; py <= 4; ++py)
    for (int px = 1; px <= 3; ++px) {
      std::vector<size_t> times(n, 0);
      for (int r = 0; r < py * px; ++r) {
        TilePlace t;
        CHECK(tile_place(TileCut{ph, pw, py, px}, r, &t), "%s: place", name);
        const SeedDeal by_seed = deal_seeds(seeds.data(), n, shift, t, false);
        CHECK(by_seed.explicit_colours && by_seed.col.size() == by_seed.n(), "%s: explicit colours", name);
        // exactly the seeds on the held block, at their local pixel, coloured index + 1, in list order
        size_t k = 0;
        for (size_t i = 0; i < n; ++i) {
          const size_t y = seeds[2 * i] + shift, x = seeds[2 * i + 1] + shift;
          if (y < t.lo || y >= t.hi || x < t.clo || x >= t.chi) continue;
          ++times[i];
          CHECK(k < by_seed.n() && by_seed.loc[2 * k] == y - t.lo && by_seed.loc[2 * k + 1] == x - t.clo && by_seed.col[k] == i + 1, "%s: seed %zu on rank %d", name, i, r);
          ++k;
        }
        CHECK(k == by_seed.n(), "%s: rank %d got a seed that is not on its block", name, r);
        if (sorted && px == 1) {
          const SeedDeal range = deal_seeds(seeds.data(), n, shift, t, true);
          CHECK(!range.explicit_colours && range.col.empty(), "%s: the range form carries colours", name);
          CHECK(pairs_of(range) == pairs_of(by_seed), "%s: the two forms differ on rank %d of %d", name, r, py);
          for (size_t j = 0; j < range.n(); ++j) CHECK(range.first_colour + j == by_seed.col[j], "%s: first_colour + position != index + 1", name);
        }
      }
      for (size_t i = 0; i < n; ++i) {      // a seed on a halo row or column belongs to every rank that holds it
        const size_t y = seeds[2 * i] + shift, x = seeds[2 * i + 1] + shift;
        size_t holders = 0;
        for (int r = 0; r < py * px; ++r) {
          TilePlace t;
          tile_place(TileCut{ph, pw, py, px}, r, &t);
          holders += y >= t.lo && y < t.hi && x >= t.clo && x < t.chi;
        }
        CHECK(times[i] == holders && holders >= 1, "%s: seed %zu dealt %zu times, held by %zu", name, i, times[i], holders);
      }
    }
}

void test_seed_dealing() {
  // a 12 x 7 plane; over 4 row blocks the seams lie at rows 3, 6, 9: rows 2, 3 (5, 6; 8, 9) are held by two ranks
  check_deal("sorted", {0, 1, 2, 6, 3, 0, 3, 5, 6, 2, 8, 1, 11, 6}, 12, 7, 0, true);
  check_deal("sorted with duplicates", {1, 1, 1, 1, 2, 3, 2, 3, 2, 0, 9, 4, 9, 4}, 12, 7, 0, true);
  check_deal("unsorted", {9, 4, 0, 0, 3, 3, 2, 6, 11, 1, 3, 3}, 12, 7, 0, false);
  check_deal("empty", {}, 12, 7, 0, true);
  check_deal("every row, seams and halos", {0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 0, 8, 1, 9, 2, 10, 3, 11, 4}, 12, 7, 0, true);
  check_deal("shifted", {0, 0, 1, 4, 2, 2, 4, 0, 7, 4, 9, 4}, 12, 7, 1, true);      // a 10 x 5 image in its ring
  check_deal("shifted, unsorted", {9, 4, 0, 0, 4, 1}, 12, 7, 1, false);
  // refusals: the raw coordinate against ph - shift
  bool sorted;
  const uint64_t wrap[] = {0, 0, UINT64_MAX, 0}, wrap_c[] = {0, UINT64_MAX}, at_edge[] = {11, 0}, at_edge_c[] = {0, 6}, last[] = {10, 5};
  CHECK(first_seed_outside(wrap, 2, 12, 7, 1, &sorted) == 1, "row 2^64 - 1 with shift 1 passes");
  CHECK(first_seed_outside(wrap_c, 1, 12, 7, 1, &sorted) == 0, "column 2^64 - 1 with shift 1 passes");
  CHECK(first_seed_outside(at_edge, 1, 12, 7, 1, &sorted) == 0 && first_seed_outside(at_edge_c, 1, 12, 7, 1, &sorted) == 0, "a coordinate of ph - shift passes");
  CHECK(first_seed_outside(at_edge, 1, 12, 7, 0, &sorted) == 1 && first_seed_outside(last, 1, 12, 7, 1, &sorted) == 1, "the last pixel is refused");
  // 2^31-scale coordinates: whatever passes on the largest plane is below 2^31 after the shift, so the narrowing to u32 is exact;
  // 2^31 and 2^32 + 5 (which would alias pixel 5) never reach it
  const size_t big = TILE_MAX_SIDE;
  for (size_t shift = 0; shift < 2; ++shift) {
    const uint64_t inside[] = {big - shift - 1, 5}, out31[] = {(uint64_t)1 << 31, 5}, alias[] = {((uint64_t)1 << 32) + 5, 5}, alias_c[] = {5, ((uint64_t)1 << 32) + 5};
    CHECK(first_seed_outside(inside, 1, big, big, shift, &sorted) == 1 && inside[0] + shift < ((uint64_t)1 << 31), "the largest coordinate");
    CHECK(first_seed_outside(out31, 1, big, big, shift, &sorted) == 0 && first_seed_outside(alias, 1, big, big, shift, &sorted) == 0 &&
          first_seed_outside(alias_c, 1, big, big, shift, &sorted) == 0, "a coordinate of 2^31 or more passes");
    TilePlace t;
    CHECK(tile_place(TileCut{big, big, 4, 1}, 3, &t), "place");
    for (int by_range = 0; by_range < 2; ++by_range) {
      const SeedDeal d = deal_seeds(inside, 1, shift, t, by_range != 0);
      CHECK(d.n() == 1 && d.loc[0] == (uint32_t)(big - 1 - t.lo) && d.loc[1] == 5 + shift && (by_range ? d.first_colour : d.col[0]) == 1, "the last row of the largest plane");
    }
  }
}

}  // namespace

int main() {
  test_partition();
  test_gather_layout();
  test_image_window();
  test_seed_dealing();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("tile plan ok\n");
  return 0;
}
