// ws_tile_plan.hpp -- how a field is cut over the ranks of a group: the arithmetic of the tiled transforms (ws_tiled.hip).
//
// Plain C++17, no HIP: pure functions of the cut.  A field is cut into py x px tiles (rank = ty * px + tx); row blocks are the
// cut with px = 1.  A rank OWNS a rectangle and HOLDS it plus a halo of one pixel on every side that has a neighbour.  Here:
// the place of a rank, the layout of the gather on rank 0, the window of the caller's image that lands in a held block under
// edge correction, and the dealing of a host seed list.  tests/cpp/test_tile_plan.cpp runs all of it on a CPU.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace wsapi {

struct TileCut {
  size_t field_h = 0, field_w = 0;
  int py = 1, px = 1;
  int world() const { return py * px; }
};

struct TilePlace {
  size_t r0 = 0, r1 = 0, c0 = 0, c1 = 0;          // owned: rows [r0, r1), columns [c0, c1) of the field
  size_t lo = 0, hi = 0, clo = 0, chi = 0;        // held: the owned rectangle and its halo
  size_t h = 0, w = 0;                            // the held block; its planes have pitch w
  int nb[4] = {-1, -1, -1, -1};                   // the ranks above, below, left and right (-1: the field's edge)
  size_t own_h() const { return r1 - r0; }
  size_t own_w() const { return c1 - c0; }
  size_t own_at() const { return (r0 - lo) * w + (c0 - clo); }      // the first owned word of a held plane
};

// Part k of n rows (or columns) split into `parts`: owned [a0, a1), held [lo, hi).  False: no such part, or fewer rows than parts
// (a part without rows would hand a halo row on as if it were its own).
inline bool tile_split(size_t n, int k, int parts, size_t *a0, size_t *a1, size_t *lo, size_t *hi) {
  if (parts < 1 || k < 0 || k >= parts || n < (size_t)parts) return false;
  const size_t base = n / (size_t)parts, extra = n % (size_t)parts, r = (size_t)k;
  *a0 = r * base + std::min(r, extra);
  *a1 = *a0 + base + (r < extra ? 1 : 0);
  *lo = k > 0 ? *a0 - 1 : *a0;
  *hi = k < parts - 1 ? *a1 + 1 : *a1;
  return true;
}

// Where `rank` sits.  Row blocks (px = 1) hold the whole width, a width of 0 included: a field of no columns is still a field.
inline bool tile_place(const TileCut &c, int rank, TilePlace *t) {
  if (c.py < 1 || c.px < 1 || rank < 0 || rank >= c.world()) return false;
  const int ty = rank / c.px, tx = rank % c.px;
  if (!tile_split(c.field_h, ty, c.py, &t->r0, &t->r1, &t->lo, &t->hi)) return false;
  if (c.px == 1) { t->c0 = t->clo = 0; t->c1 = t->chi = c.field_w; }
  else if (!tile_split(c.field_w, tx, c.px, &t->c0, &t->c1, &t->clo, &t->chi)) return false;
  t->h = t->hi - t->lo;
  t->w = t->chi - t->clo;
  t->nb[0] = ty > 0 ? rank - c.px : -1;
  t->nb[1] = ty < c.py - 1 ? rank + c.px : -1;
  t->nb[2] = tx > 0 ? rank - 1 : -1;
  t->nb[3] = tx < c.px - 1 ? rank + 1 : -1;
  return true;
}

// The gather on rank 0: every rank's place, and where its packed owned rectangle lands in the table rank 0 receives into
// (at[r], in words; rank 0 sends nothing to itself, so at[0] = at[1] = 0 and at[world] is the table's size).
struct GatherLayout {
  std::vector<TilePlace> place;
  std::vector<size_t> at;
};

inline bool gather_layout(const TileCut &c, GatherLayout *l) {
  if (c.py < 1 || c.px < 1) return false;
  const size_t world = (size_t)c.world();
  l->place.assign(world, TilePlace{});
  l->at.assign(world + 1, 0);
  for (size_t r = 0; r < world; ++r) {
    if (!tile_place(c, (int)r, &l->place[r])) return false;
    l->at[r + 1] = l->at[r] + (r ? l->place[r].own_h() * l->place[r].own_w() : 0);
  }
  return true;
}

// The caller's h x w image against a held block of the plane the ranks cut (the image itself or, under edge correction, the image
// inside a ring of one pixel): rows x cols pixels from image pixel (src_r, src_c) land at (dst_r, dst_c) of the block, the rest is ring.
struct ImageWindow {
  size_t rows = 0, cols = 0, src_r = 0, src_c = 0, dst_r = 0, dst_c = 0;
};

inline ImageWindow image_window(const TilePlace &t, size_t h, size_t w, bool edge_correction) {
  const size_t o = edge_correction ? 1 : 0;      // plane pixel (p, q) holds image pixel (p - o, q - o)
  const size_t p0 = std::max(t.lo, o), p1 = std::min(t.hi, h + o), q0 = std::max(t.clo, o), q1 = std::min(t.chi, w + o);
  if (p1 <= p0 || q1 <= q0) return ImageWindow{};
  return ImageWindow{p1 - p0, q1 - q0, p0 - o, q0 - o, p0 - t.lo, q0 - t.clo};
}

// ---- a host seed list, dealt to the ranks ------------------------------------------------------------------------------------

constexpr size_t TILE_MAX_SIDE = 0x7FFFFFF0ull;      // of a (padded) plane: a coordinate inside one fits 31 bits

// The index of the first seed outside the ph x pw plane, n_seeds if there is none; *rows_sorted: the rows never decrease.
// The RAW coordinate is compared against ph - shift: coordinate + shift wraps to 0 at 2^64 - 1 and would pass.  What passes on a
// plane within TILE_MAX_SIDE is below 2^31 with the shift, so deal_seeds never narrows a wrapped or an aliasing value.
inline size_t first_seed_outside(const uint64_t *seeds_rc, size_t n_seeds, size_t ph, size_t pw, size_t shift, bool *rows_sorted) {
  *rows_sorted = true;
  for (size_t i = 0; i < n_seeds; ++i) {
    if (seeds_rc[2 * i] >= ph - shift || seeds_rc[2 * i + 1] >= pw - shift) return i;
    if (i && seeds_rc[2 * i] < seeds_rc[2 * i - 2]) *rows_sorted = false;
  }
  return n_seeds;
}

struct SeedDeal {
  std::vector<uint32_t> loc;       // (row, column) in the held block, a pair per seed
  std::vector<uint32_t> col;       // its colours (list index + 1); empty in the range form
  uint32_t first_colour = 1;       // range form: seed k of loc has colour first_colour + k
  bool explicit_colours = false;
  size_t n() const { return loc.size() / 2; }
};

// The seeds that fall on a rank's held block (halo included: a seed on a halo row belongs to both ranks), of a list that passed
// first_seed_outside.  by_range: the list's rows never decrease and the block spans the plane's width (row blocks), so the
// rank's seeds are ONE contiguous range, found by binary search; otherwise seed by seed with explicit colours.
inline SeedDeal deal_seeds(const uint64_t *seeds_rc, size_t n_seeds, size_t shift, const TilePlace &t, bool by_range) {
  SeedDeal d;
  d.explicit_colours = !by_range;
  if (by_range) {
    auto lower = [&](uint64_t row) {      // first list index whose (shifted) row is >= row
      size_t a = 0, b = n_seeds;
      while (a < b) { const size_t m = (a + b) / 2; if (seeds_rc[2 * m] + shift < row) a = m + 1; else b = m; }
      return a;
    };
    const size_t i0 = lower(t.lo), i1 = lower(t.hi);
    d.loc.resize(2 * (i1 - i0));
    for (size_t i = i0; i < i1; ++i) {
      d.loc[2 * (i - i0)] = (uint32_t)(seeds_rc[2 * i] + shift - t.lo);
      d.loc[2 * (i - i0) + 1] = (uint32_t)(seeds_rc[2 * i + 1] + shift - t.clo);
    }
    d.first_colour = (uint32_t)i0 + 1u;
    return d;
  }
  for (size_t i = 0; i < n_seeds; ++i) {
    const uint64_t row = seeds_rc[2 * i] + shift, cc = seeds_rc[2 * i + 1] + shift;
    if (row < t.lo || row >= t.hi || cc < t.clo || cc >= t.chi) continue;
    d.loc.push_back((uint32_t)(row - t.lo));
    d.loc.push_back((uint32_t)(cc - t.clo));
    d.col.push_back((uint32_t)i + 1u);
  }
  return d;
}

}  // namespace wsapi
