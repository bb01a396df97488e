// ws_merge_final.hip -- gfx950 kernels of the merging transform's final labels alone (see ws_merge.hpp for the maths): no
// levels, no stamps -- a pixel is coloured exactly when its label is not 0.  The blocks of a tiled field, the whole image by
// 64 x 64 tiles (the one-lake tile route and the general one), the final relabel, and a stack of slices.  The union-find is
// ws_uf.hpp's; the level loop's kernels are ws_merge.hip.
#include "ws_uf.hpp"

namespace wsk {

// ---- merging across the row blocks of a tiled field (third row) -----------------------------------------
//
// Final labels only.  Every rank holds a union-find over ALL seed colours of the field and joins the touching colours of
// its own block: every horizontal pair of its rows and every vertical pair (r, r + 1), seam pairs to its halo rows
// included, under find_merge's rule that one pixel of a pair is interior IN THE WHOLE FIELD (lib.rs:411-434; `row0` is
// the field row of the block's first local row).  A lake that spans several blocks is a chain of such local pieces
// linked at boundary colours, so it is enough that every rank tells every other, for each colour c on its two boundary
// rows and its halo rows, the root of c in ITS forest: k_block_colour_roots writes the pairs (c, root(c)), one
// all-gather, and every rank joins all gathered pairs into its own forest (union_edges).  Roots are class minima
// (union-by-min), so the merged root is the smallest seed colour of the whole lake: the canonical id.
// (col0, W: a tile of a field cut in both directions holds the field's columns [col0, col0 + w); a row block: col0 = 0, W = w)
__global__ __launch_bounds__(256) void k_block_union_pixels(const uint32_t *__restrict__ labels, int h, int w, int row0, int H,
                                                            uint32_t *parent, int col0, int W) {
  const size_t n = (size_t)h * w;
  size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; p < n; p += step) {
    const uint32_t lp = labels[p];
    if (lp == 0u) continue;                              // at the final level a pixel is coloured iff its label is not 0
    const int y = (int)(p / (size_t)w), x = (int)(p - (size_t)y * w);
    const bool ip = interior(row0 + y, col0 + x, H, W);
    if (x + 1 < w) {
      const uint32_t lq = labels[p + 1];
      if (lq != 0u && lq != lp && (ip || interior(row0 + y, col0 + x + 1, H, W))) (void)uf_union(parent, lp, lq);
    }
    if (y + 1 < h) {
      const uint32_t lq = labels[p + w];
      if (lq != 0u && lq != lp && (ip || interior(row0 + y + 1, col0 + x, H, W))) (void)uf_union(parent, lp, lq);
    }
  }
}

hipError_t block_union_pixels(hipStream_t s, const uint32_t *labels, int h, int w, int row0, int H, uint32_t *parent, int col0, int W) {
  if (h == 0 || w == 0) return hipSuccess;
  const size_t n = (size_t)h * w;
  k_block_union_pixels<<<clamped_grid(n, 256, 8192), 256, 0, s>>>(labels, h, w, row0, H, parent, col0, W < 0 ? w : W);
  return hipGetLastError();
}

// ... and of a tile: its two outermost rows AND columns on every side (4 w + 4 h pairs, then (0, 0) up to n_pairs: tiles of
// a grid differ by a row or a column, an all-gather wants equal parts)
__global__ void k_block_colour_roots2d(const uint32_t *__restrict__ labels, int h, int w, uint32_t *parent, uint2 *pairs, size_t n_pairs) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pairs) return;
  uint32_t c = 0;
  if (i < (size_t)4 * w) {
    const int k = (int)(i / (size_t)w), x = (int)(i - (size_t)k * w);
    const int rows[4] = {0, min(1, h - 1), max(h - 2, 0), h - 1};
    c = labels[(size_t)rows[k] * w + x];
  } else if (i < (size_t)4 * w + (size_t)4 * h) {
    const size_t j = i - (size_t)4 * w;
    const int k = (int)(j / (size_t)h), y = (int)(j - (size_t)k * h);
    const int cols[4] = {0, min(1, w - 1), max(w - 2, 0), w - 1};
    c = labels[(size_t)y * w + cols[k]];
  }
  pairs[i] = c ? make_uint2(c, uf_find(parent, c)) : make_uint2(0u, 0u);
}

hipError_t block_colour_roots2d(hipStream_t s, const uint32_t *labels, int h, int w, uint32_t *parent, uint2 *pairs, size_t n_pairs) {
  if (n_pairs == 0) return hipSuccess;
  k_block_colour_roots2d<<<(unsigned)((n_pairs + 255) / 256), 256, 0, s>>>(labels, h, w, parent, pairs, n_pairs);
  return hipGetLastError();
}

// pairs[i] = (colour, root of colour) for the pixels of local rows 0, 1, h - 2, h - 1 (4 w pairs; (0, 0) where uncoloured)
__global__ void k_block_colour_roots(const uint32_t *__restrict__ labels, int h, int w, uint32_t *parent, uint2 *pairs) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)4 * w) return;
  const int k = (int)(i / (size_t)w), x = (int)(i - (size_t)k * w);
  const int rows[4] = {0, min(1, h - 1), max(h - 2, 0), h - 1};
  const uint32_t c = labels[(size_t)rows[k] * w + x];
  pairs[i] = c ? make_uint2(c, uf_find(parent, c)) : make_uint2(0u, 0u);
}

hipError_t block_colour_roots(hipStream_t s, const uint32_t *labels, int h, int w, uint32_t *parent, uint2 *pairs) {
  if (h == 0 || w == 0) return hipSuccess;
  k_block_colour_roots<<<(unsigned)((4 * (size_t)w + 255) / 256), 256, 0, s>>>(labels, h, w, parent, pairs);
  return hipGetLastError();
}

// ---- the whole image: the general tiles ----------------------------------------------------

// One launch, 64x64 tiles.  Joining every crossing pixel pair in the global forest costs ~60 M
// unions that all end at the one surviving root; instead each tile first joins its own coloured
// pixels in an LDS union-find (adjacency rule of find_merge: one endpoint of a pair must be an
// interior pixel, lib.rs:411-434), takes the smallest colour of every local component, and only then
// touches the global forest: once per colour REGION of a component (its top-left pixels) and once
// per crossing pair on the tile's right / bottom edge -- ~6x fewer global unions, most of them local.
constexpr int UT = 64;                                   // tile side
constexpr int UT_PX = UT * UT / 256;                     // pixels per thread (16): column strips as in k_resolve_local

__device__ __forceinline__ uint32_t lds_find(uint32_t *P, uint32_t x) {
  for (;;) {
    const uint32_t p = P[x];
    if (p == x) return x;
    const uint32_t g = P[p];
    if (g == p) return p;
    atomicMin(&P[x], g);
    x = g;
  }
}
__device__ __forceinline__ void lds_union(uint32_t *P, uint32_t a, uint32_t b) {
  for (;;) {
    a = lds_find(P, a);
    b = lds_find(P, b);
    if (a == b) return;
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicCAS(&P[b], b, a);
    if (old == b) return;
    b = old;
  }
}

__global__ __launch_bounds__(256) void k_union_tiles(const uint32_t *__restrict__ labels, int H, int W, int tilesX, uint32_t *parent,
                                                     const uint32_t *__restrict__ tile_min) {
  if (tile_min[blockIdx.x] != 0u) return;          // a one-lake tile: k_tile_scan and k_union_seeds deal with it
  __shared__ uint32_t sP[UT * UT];        // local forest over the tile's pixels
  __shared__ uint32_t sMin[UT * UT];      // smallest colour of a local component, kept at its root
  const int tile_x = blockIdx.x % tilesX, tile_y = blockIdx.x / tilesX;
  const int tid = threadIdx.x, lane = tid & 63, strip = tid >> 6;
  const int x0 = tile_x * UT, y0 = tile_y * UT;
  const int gx = x0 + lane, gy0 = y0 + strip * UT_PX;
  const int gxc = min(gx, W - 1);

  uint32_t col[UT_PX], colR[UT_PX];       // colour of the pixel / of its right neighbour; 0 = uncoloured or outside
  uint32_t colD_last;                     // colour below the strip's last pixel
#pragma unroll
  for (int i = 0; i < UT_PX; ++i) {
    const int gy = gy0 + i, gyc = min(gy, H - 1);
    const size_t g = (size_t)gyc * W + gxc;
    // final level: a pixel is coloured exactly when its label is non-zero (the stamps are not read)
    const uint32_t l = labels[g];
    const uint32_t lr = labels[(size_t)gyc * W + min(gx + 1, W - 1)];
    col[i] = (gy < H && gx < W) ? l : 0u;
    colR[i] = (gy < H && gx + 1 < W) ? lr : 0u;
    sP[(strip * UT_PX + i) * UT + lane] = (uint32_t)((strip * UT_PX + i) * UT + lane);
    sMin[(strip * UT_PX + i) * UT + lane] = 0xFFFFFFFFu;
  }
  {
    const int gy = gy0 + UT_PX, gyc = min(gy, H - 1);
    const uint32_t l = labels[(size_t)gyc * W + gxc];
    colD_last = (gy < H && gx < W) ? l : 0u;
  }
  __syncthreads();

  // local unions: right and down neighbours inside the tile (any colours: touching lakes merge)
#pragma unroll
  for (int i = 0; i < UT_PX; ++i) {
    if (col[i] == 0u) continue;
    const int ly = strip * UT_PX + i, gy = gy0 + i;
    const bool ip = interior(gy, gx, H, W);
    const uint32_t cell = (uint32_t)(ly * UT + lane);
    if (lane + 1 < UT && colR[i] != 0u && (ip || interior(gy, gx + 1, H, W))) lds_union(sP, cell, cell + 1);
    const uint32_t cd = i == UT_PX - 1 ? colD_last : col[i + 1];
    if (ly + 1 < UT && cd != 0u && (ip || interior(gy + 1, gx, H, W))) lds_union(sP, cell, cell + UT);
  }
  __syncthreads();
  uint32_t root[UT_PX];
#pragma unroll
  for (int i = 0; i < UT_PX; ++i) {
    root[i] = col[i] ? lds_find(sP, (uint32_t)((strip * UT_PX + i) * UT + lane)) : 0u;
    if (col[i]) atomicMin(&sMin[root[i]], col[i]);
  }
  __syncthreads();

  // colour of the left neighbour, fetched with every lane active (a shuffle under a divergent
  // branch would read inactive lanes)
  uint32_t colL[UT_PX];
#pragma unroll
  for (int i = 0; i < UT_PX; ++i) {
    const uint32_t v = __shfl_up(col[i], 1, 64);
    colL[i] = lane > 0 ? v : 0u;
  }

  // global unions
#pragma unroll
  for (int i = 0; i < UT_PX; ++i) {
    if (col[i] == 0u) continue;
    const int ly = strip * UT_PX + i, gy = gy0 + i;
    const uint32_t cmin = sMin[root[i]];
    // (a) one union per colour region of the component: the pixel has no same-coloured pixel of its
    //     own tile to the left, nor above inside this thread's strip (a region's top-left pixel
    //     always qualifies; the strip above belongs to another wave and counts as "different")
    const uint32_t cu = i > 0 ? col[i - 1] : 0u;
    if (col[i] != cmin && colL[i] != col[i] && cu != col[i]) uf_union(parent, col[i], cmin);
    // (b) crossing pairs over the tile's right and bottom edge
    const bool ip = interior(gy, gx, H, W);
    if (lane == UT - 1 && colR[i] != 0u && colR[i] != col[i] && (ip || interior(gy, gx + 1, H, W))) uf_union(parent, col[i], colR[i]);
    if (ly == UT - 1 && colD_last != 0u && colD_last != col[i] && (ip || interior(gy + 1, gx, H, W))) uf_union(parent, col[i], colD_last);
  }
}

// the four corner pixels of the image touch border pixels only: a seed there never joins anything
__device__ __forceinline__ bool image_corner(int y, int x, int H, int W) { return (y == 0 || y == H - 1) && (x == 0 || x == W - 1); }

// ---- one-lake tiles -------------------------------------------------------------------------
//
// At the final level of an ordinary field nearly every 64 x 64 tile is a single lake: every pixel of it
// that is an interior pixel of the image is coloured.  (Those pixels form a rectangle, so they are
// 4-connected; a coloured pixel of the image border joins through its inward neighbour, which the
// adjacency rule of find_merge allows: one endpoint interior, lib.rs:411-434.)  For such a tile nothing
// has to be discovered locally, and two such tiles that share an edge are always joined across it.
// What remains is bookkeeping, split so that no thread idles behind another's union latency and no
// crowd of unions walks the same chain at once:
//   k_tile_scan    per tile: "one lake?" and its smallest colour cmin -> tile_min (0 = no)
//   k_tile_links   per tile: joins cmin with the cmin of the one-lake tile to the right / below;
//                  k_tile_roots then replaces every tile's cmin by the root of its lake
//   k_union_seeds  per SEED: colour i+1 joins the cmin of the tile its seed pixel lies in
//   k_tile_edges   per tile edge pixel: a colour a tile holds WITHOUT its seed came in over an edge; if from a
//                  one-lake tile, the two tiles are joined and that tile holds the colour already (induction
//                  along the colour's region); if from a general tile, the colour joins cmin here, as do the
//                  colours across the right / bottom edge when the tile there is general
//   k_union_tiles  the general path (LDS union-find) for the tiles k_tile_scan turned down
// preclassified: the resolve kernel has filled tile_min already; only its "undecided" tiles are looked at
__global__ __launch_bounds__(256) void k_tile_scan(const uint32_t *__restrict__ labels, int H, int W, int tilesX, uint32_t *tile_min,
                                                   int preclassified) {
  __shared__ uint32_t sWaveMin[4];
  if (preclassified && tile_min[blockIdx.x] != 0xFFFFFFFFu) return;
  const int tile_x = blockIdx.x % tilesX, tile_y = blockIdx.x / tilesX;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = tile_x * UT, y0 = tile_y * UT;
  // 16 pixels per thread: patch (tid & 15, tid >> 4); one 16-byte load per row when the rows are aligned and
  // the patch lies inside the plane
  const int gx0 = x0 + (tid & 15) * 4, gy0 = y0 + (tid >> 4) * 4;
  const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 15u) == 0 && gx0 + 4 <= W;
  uint32_t tmin1 = 0xFFFFFFFFu;      // smallest (colour - 1): an uncoloured pixel (0) wraps to the top and never wins
  bool ok = true;                    // every in-plane image-interior pixel seen is coloured
  bool any_interior = false;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gy = gy0 + r, gyc = min(gy, H - 1);
    uint32_t v[4];
    if (vec) {
      const u32x4_m q = *reinterpret_cast<const u32x4_m *>(labels + (size_t)gyc * W + gx0);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c) v[c] = labels[(size_t)gyc * W + min(gx0 + c, W - 1)];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int gx = gx0 + c;
      const bool in_plane = gy < H && gx < W;
      const bool inter = in_plane && interior(gy, gx, H, W);
      if (in_plane && !image_corner(gy, gx, H, W)) tmin1 = min(tmin1, v[c] - 1u);
      ok = ok && (!inter || v[c] != 0u);
      any_interior = any_interior || inter;
    }
  }
  const bool one_lake = __syncthreads_and(ok) != 0 && __syncthreads_or(any_interior) != 0;
  for (int o = 32; o > 0; o >>= 1) tmin1 = min(tmin1, (uint32_t)__shfl_xor(tmin1, o, 64));
  if (lane == 0) sWaveMin[wave] = tmin1;
  __syncthreads();
  if (tid == 0) tile_min[blockIdx.x] = one_lake ? min(min(sWaveMin[0], sWaveMin[1]), min(sWaveMin[2], sWaveMin[3])) + 1u : 0u;
}

// Every pair of one-lake tiles that share an edge must end in one set.  One union per pair (32 k of them at 8192^2, nearly
// all into the same set) was 43 us of CAS retries on a few hot roots.  Instead: along a row, a RUN of one-lake tiles is
// tied together by a segmented min-scan in the wave -- tile i joins the smallest colour of the run's tiles before it, a
// child slot of its own and a chain a few hooks deep (the prefix minima of the run) -- and two runs in consecutive rows
// are joined once, at the leftmost column they share (the head of one of them).
__global__ void k_tile_links(const uint32_t *__restrict__ tile_min, int tilesX, int tilesY, uint32_t *parent) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool in = t < tilesX * tilesY;
  const int tx = in ? t % tilesX : 0, ty = in ? t / tilesX : 0;
  const uint32_t m = in ? tile_min[t] : 0u;
  const uint32_t left = in && tx > 0 ? tile_min[t - 1] : 0u;
  const uint32_t md = in && ty + 1 < tilesY ? tile_min[t + tilesX] : 0u;
  const uint32_t md_left = in && ty + 1 < tilesY && tx > 0 ? tile_min[t + tilesX - 1] : 0u;
  const bool head = m != 0u && left == 0u, md_head = md != 0u && md_left == 0u;
  // inclusive min over the run, from its first tile IN THIS WAVE to this lane (a tile that is not one lake is a segment
  // of its own: its value is never used)
  uint32_t v = m != 0u ? m : 0xFFFFFFFFu;
  bool f = head || m == 0u || lane == 0;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t pv = (uint32_t)__shfl_up((int)v, d, 64);
    const int pf = __shfl_up((int)f, d, 64);
    if (lane >= d && !f) { v = min(v, pv); f = pf != 0; }
  }
  const uint32_t before = (uint32_t)__shfl_up((int)v, 1, 64);      // the run's smallest colour up to the tile on the left
  if (m == 0u) return;
  if (!head) {
    const uint32_t join = lane == 0 ? left : before;               // (lane 0: the run goes on from the wave before)
    if (join != m) uf_union(parent, m, join);
  }
  if (md != 0u && md != m && (head || md_head)) uf_union(parent, m, md);
}

// after the links: every one-lake tile remembers the ROOT of its lake instead of its own smallest colour, so
// that the 450 seeds of a tile find a root in one load instead of all walking (and compressing) the same chain
// (a plain walk: the forest is at rest between two launches, and 16 k halving finds on the links' few chains were 29 us
// of atomics on the same words against 6 us for the walk)
// mark (optional, zeroed, one word per colour): mark[c] = 1 for every colour the tile links have touched -- a tile's
// smallest colour or a lake's root; every other colour is still its own root and nobody's parent
__global__ void k_tile_roots(uint32_t *tile_min, int ntiles, uint32_t *parent, uint32_t *mark) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= ntiles) return;
  const uint32_t m = tile_min[t];
  if (m != 0u && m != 0xFFFFFFFFu) {
    const uint32_t r = uf_root(parent, m);
    tile_min[t] = r;
    if (mark) { mark[r] = 1u; mark[m] = 1u; }
  }
}

// Nearly every seed is a colour nobody has touched yet (its own root, no child: k_tile_roots marks the colours the tile
// links have touched) that goes under its tile's root, a smaller colour: for those the hook is a PLAIN store, without
// reading the slot -- nobody else reads or writes it in this launch: a union names a colour only as the seed's own (this
// thread) or as a tile root (marked), and a find only passes through colours that something was hooked under.  Every
// other case takes the union.  (54 -> 45 us at 8192^2: what is left is the 16 B per seed the kernel moves.)
// A list entry whose pixel a LATER entry names again has lost its colour (the later one overwrites it, lib.rs:1670-1677):
// colour i + 1 exists nowhere in the plane and must not become a lake's id.  Hooked under a smaller root it is harmless -- no
// pixel carries it -- so only the case that would hook the tile's root under it (i + 1 < root) looks: at the final level a
// seed pixel's label is the colour painted last, one load of `labels` decides, and the plain-store path above keeps its
// argument (an overwritten colour is unmarked, its own root and nobody's parent, like any untouched one).
__global__ void k_union_seeds(const uint32_t *__restrict__ labels, const uint32_t *__restrict__ seeds_rc, size_t n_seeds, int H, int W,
                              int tilesX, const uint32_t *__restrict__ tile_min, uint32_t *parent,
                              const uint32_t *__restrict__ tile_root_mark) {
  // (four seeds per thread and round, each stage's loads in flight together: the kernel is three dependent loads and a
  // store per seed, and with one seed per thread it was 54 us of waiting for them)
  constexpr int SU = 4;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i0 = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < n_seeds; i0 += SU * step) {
    uint2 rc[SU];
    uint32_t cmin[SU], mark[SU];
    bool ok[SU];
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const size_t i = i0 + u * step;
      rc[u] = reinterpret_cast<const uint2 *>(seeds_rc)[i < n_seeds ? i : n_seeds - 1];
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const size_t i = i0 + u * step;
      // (a seed outside the plane: the transform has reported it; here it only must not index outside tile_min)
      ok[u] = i < n_seeds && rc[u].x < (uint32_t)H && rc[u].y < (uint32_t)W;
      const size_t me = ok[u] ? i + 1 : 0;
      cmin[u] = tile_min[ok[u] ? (size_t)(rc[u].x / UT) * tilesX + rc[u].y / UT : 0];
      mark[u] = tile_root_mark ? tile_root_mark[me] : 1u;
    }
#pragma unroll
    for (int u = 0; u < SU; ++u) {
      const uint32_t me = (uint32_t)(i0 + u * step + 1);
      if (!ok[u] || cmin[u] == 0u || cmin[u] == me || image_corner((int)rc[u].x, (int)rc[u].y, H, W)) continue;
      if (cmin[u] < me && mark[u] == 0u) parent[me] = cmin[u];      // (unmarked: parent[me] == me still, see k_tile_roots)
      else if (cmin[u] < me || labels[(size_t)rc[u].x * W + rc[u].y] == me) uf_union(parent, me, cmin[u]);      // (ok[u]: the pixel is in the plane)
    }
  }
}

// wave = edge of the tile (0 bottom, 1 right, 2 top, 3 left), lane = position along it
__global__ __launch_bounds__(256) void k_tile_edges(const uint32_t *__restrict__ labels, int H, int W, int tilesX, int tilesY,
                                                    const uint32_t *__restrict__ tile_min, uint32_t *parent) {
  const uint32_t cmin = tile_min[blockIdx.x];
  if (cmin == 0u) return;
  const int tile_x = blockIdx.x % tilesX, tile_y = blockIdx.x / tilesX;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // the tile across this wave's edge (none at the image border).  Only a GENERAL tile there gives this wave
  // anything to do -- checked before a single pixel is loaded: a tile edge is one pixel per row, a cache line
  // fetched for each (the kernel moved 400 MB to look at 16 MB of pixels and find, on an ordinary field, nothing).
  const int nb = wave == 0 ? (tile_y + 1 < tilesY ? (int)blockIdx.x + tilesX : -1)
               : wave == 1 ? (tile_x + 1 < tilesX ? (int)blockIdx.x + 1 : -1)
               : wave == 2 ? (tile_y > 0 ? (int)blockIdx.x - tilesX : -1)
                           : (tile_x > 0 ? (int)blockIdx.x - 1 : -1);
  if (nb < 0 || tile_min[nb] != 0u) return;
  const int x0 = tile_x * UT, y0 = tile_y * UT;
  const int ylast = min(y0 + UT, H) - 1, xlast = min(x0 + UT, W) - 1;       // the tile's last row / column inside the plane
  const int ey = wave == 0 ? ylast : (wave == 2 ? y0 : y0 + lane);
  const int ex = wave == 1 ? xlast : (wave == 3 ? x0 : x0 + lane);
  const bool own_ok = ey <= ylast && ex <= xlast;
  const int fy = ey + (wave == 0 ? 1 : 0), fx = ex + (wave == 1 ? 1 : 0);
  const bool far_ok = own_ok && wave < 2 && fy < H && fx < W;
  // unconditional loads on clamped addresses (ws_relax.hip)
  const uint32_t own_v = labels[(size_t)min(ey, H - 1) * W + min(ex, W - 1)];
  const uint32_t far_v = labels[(size_t)min(fy, H - 1) * W + min(fx, W - 1)];
  const uint32_t own = own_ok && !image_corner(ey, ex, H, W) ? own_v : 0u, far = far_ok ? far_v : 0u;
  // own colours on this edge join cmin: a colour whose seed lies elsewhere reached this tile over one of its
  // edges, from a one-lake tile (joined with this one by k_tile_links, and holding the colour already, by
  // induction along the colour's region) or from a general one -- this case.  One union per run of equal colours.
  const uint32_t want_own = (own != 0u && own != cmin) ? own : 0u;
  const uint32_t want_own_prev = __shfl_up(want_own, 1, 64);
  if (want_own != 0u && (lane == 0 || want_own != want_own_prev)) uf_union(parent, want_own, cmin);
  // colours across the right / bottom edge (the general tile's own kernel only looks right and down)
  const bool pair_ok = own != 0u && far != 0u && (interior(ey, ex, H, W) || interior(fy, fx, H, W));
  const uint32_t want_far = (wave < 2 && pair_ok && far != cmin) ? far : 0u;
  const uint32_t want_far_prev = __shfl_up(want_far, 1, 64);
  if (want_far != 0u && (lane == 0 || want_far != want_far_prev)) uf_union(parent, want_far, cmin);
}

hipError_t union_image(hipStream_t s, const uint32_t *labels, const uint32_t *seeds_rc, size_t n_seeds, int h, int w,
                       uint32_t *parent, uint32_t *tile_min, bool preclassified, uint32_t *tile_root_mark) {
  if (h == 0 || w == 0) return hipSuccess;
  const int tx = (w + UT - 1) / UT, ty = (h + UT - 1) / UT;
  hipError_t e;
  k_tile_scan<<<tx * ty, 256, 0, s>>>(labels, h, w, tx, tile_min, preclassified ? 1 : 0);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  k_tile_links<<<(tx * ty + 255) / 256, 256, 0, s>>>(tile_min, tx, ty, parent);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  k_tile_roots<<<(tx * ty + 255) / 256, 256, 0, s>>>(tile_min, tx * ty, parent, tile_root_mark);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (n_seeds) {
    const unsigned blocks = clamped_grid(n_seeds, 1024, 16384);      // four seeds per thread
    k_union_seeds<<<blocks, 256, 0, s>>>(labels, seeds_rc, n_seeds, h, w, tx, tile_min, parent, tile_root_mark);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    k_tile_edges<<<tx * ty, 256, 0, s>>>(labels, h, w, tx, ty, tile_min, parent);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  k_union_tiles<<<tx * ty, 256, 0, s>>>(labels, h, w, tx, parent, tile_min);
  return hipGetLastError();
}
size_t union_image_tiles(int h, int w) { return (size_t)((w + UT - 1) / UT) * ((h + UT - 1) / UT); }

// ---- the final relabel ----------------------------------------------------------------------
// After the last union: every colour points straight at its root, so that relabelling is one gather.
__global__ void k_uf_flatten(uint32_t *parent, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint32_t r = uf_find(parent, (uint32_t)i);
    if (r != (uint32_t)i) atomicMin(parent + i, r);
  }
}

// lib.rs:589-592 with the closed, flattened map, final level: uncoloured pixels carry label 0 and parent[0] == 0
__global__ void k_relabel_flat(const uint32_t *__restrict__ labels, const uint32_t *__restrict__ parent, uint32_t *out, size_t n) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
  const size_t nv = vec ? n / 4 : 0;
  for (size_t i = tid; i < nv; i += step) {
    const u32x4_m l = reinterpret_cast<const u32x4_m *>(labels)[i];
    reinterpret_cast<u32x4_m *>(out)[i] = u32x4_m{parent[l.x], parent[l.y], parent[l.z], parent[l.w]};
  }
  for (size_t i = nv * 4 + tid; i < n; i += step) out[i] = parent[labels[i]];
}

// The same tile by tile, for a plane whose 64 x 64 tiles union_image has classified: a one-lake tile strictly inside the
// image (every pixel coloured, all of one lake: tile_min = a colour of it) is FILLED with its root -- no label is read;
// every other tile takes the gather (of roots: uf_root).  At the final level of a map that floods completely nearly every tile is one lake:
// 8192^2 bench field 121 -> ~60 us (the gather reads and writes the plane, 537 MB; the fill writes 268 MB).
__global__ __launch_bounds__(256) void k_relabel_tiles(const uint32_t *__restrict__ labels, const uint32_t *__restrict__ parent,
                                                       const uint32_t *__restrict__ tile_min, uint32_t *out, int H, int W, int tilesX) {
  const int tile_x = blockIdx.x % tilesX, tile_y = blockIdx.x / tilesX;
  const int x0 = tile_x * UT, y0 = tile_y * UT;
  const int gx0 = x0 + (threadIdx.x & 15) * 4, gy0 = y0 + (threadIdx.x >> 4) * 4;
  const uint32_t cm = tile_min[blockIdx.x];
  const bool inside = x0 >= 1 && x0 + UT <= W - 1 && y0 >= 1 && y0 + UT <= H - 1;      // workgroup uniform
  const bool vec = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0;
  if (cm != 0u && cm != 0xFFFFFFFFu && inside && vec) {
    const uint32_t r = cm;      // (a root: relabel_final_u32 runs k_tile_roots first)
#pragma unroll
    for (int k = 0; k < 4; ++k) *reinterpret_cast<u32x4_m *>(out + (size_t)(gy0 + k) * W + gx0) = u32x4_m{r, r, r, r};
    return;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int gy = gy0 + k;
    if (gy >= H) break;
    if (vec && gx0 + 4 <= W) {
      const u32x4_m l = *reinterpret_cast<const u32x4_m *>(labels + (size_t)gy * W + gx0);
      *reinterpret_cast<u32x4_m *>(out + (size_t)gy * W + gx0) = u32x4_m{uf_root(parent, l.x), uf_root(parent, l.y), uf_root(parent, l.z), uf_root(parent, l.w)};
    } else {
      for (int c = 0; c < 4; ++c)
        if (gx0 + c < W) out[(size_t)gy * W + gx0 + c] = uf_root(parent, labels[(size_t)gy * W + gx0 + c]);
    }
  }
}

hipError_t relabel_final_u32(hipStream_t s, const uint32_t *labels, uint32_t *parent, size_t n_colours, uint32_t *out, size_t n,
                             uint32_t *tile_min, int h, int w) {
  if (n == 0) return hipSuccess;
  if (tile_min && (size_t)h * w == n) {
    // (no flattening pass over the 7 M colours first -- k_uf_flatten was 21 us at 8192^2: a one-lake tile needs ONE root,
    // found once per tile by k_tile_roots -- the seeds' unions hook the lake's root under ever smaller colours, a chain
    // ~ln(n) hooks deep that every tile would otherwise walk -- and the other tiles walk what path halving left)
    const int tx = (w + UT - 1) / UT, ty = (h + UT - 1) / UT;
    k_tile_roots<<<(tx * ty + 255) / 256, 256, 0, s>>>(tile_min, tx * ty, parent, nullptr);
    hipError_t e0 = hipGetLastError();
    if (e0 != hipSuccess) return e0;
    k_relabel_tiles<<<tx * ty, 256, 0, s>>>(labels, parent, tile_min, out, h, w, tx);
    return hipGetLastError();
  }
  const unsigned fb = clamped_grid(n_colours, 256, 8192);
  k_uf_flatten<<<fb > 0 ? fb : 1, 256, 0, s>>>(parent, n_colours);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int blocks = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  k_relabel_flat<<<blocks, 256, 0, s>>>(labels, parent, out, n);
  return hipGetLastError();
}

// ---- a stack of slices (ws_merge_batch_device) -------------------------------------------------------------------------------
// Final level of the merging transform over a stack: every pair of touching pixels with different labels, at least one of
// them interior to its slice, joins the two stack colours (as union_image on one plane; a pixel is coloured exactly when its
// label is non-zero).  No pair crosses a slice border.
__global__ __launch_bounds__(256) void k_union_stack(const uint32_t *__restrict__ labels, int slice_h, int W, size_t n,
                                                     const uint32_t *__restrict__ base, uint32_t *parent) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint32_t a = labels[p];
    if (!a) continue;
    const int x = (int)(p % W);
    const size_t row = p / W;
    const int ys = (int)(row % slice_h);
    const uint32_t add = base[row / slice_h];
    const bool ip = interior(ys, x, slice_h, W);
    if (x + 1 < W) {
      const uint32_t b = labels[p + 1];
      if (b && b != a && (ip || interior(ys, x + 1, slice_h, W))) uf_union(parent, a + add, b + add);
    }
    if (ys + 1 < slice_h) {
      const uint32_t b = labels[p + W];
      if (b && b != a && (ip || interior(ys + 1, x, slice_h, W))) uf_union(parent, a + add, b + add);
    }
  }
}

// labels[p] = root(labels[p] + base[slice]) - base[slice] in place: the smallest seed colour of the lake, in the slice's numbering
__global__ __launch_bounds__(256) void k_relabel_stack(uint32_t *labels, size_t plane, size_t n, const uint32_t *__restrict__ base,
                                                       const uint32_t *__restrict__ parent) {
  for (size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (size_t)gridDim.x * blockDim.x) {
    const uint32_t a = labels[p];
    if (!a) continue;
    const uint32_t add = base[p / plane];
    labels[p] = parent[a + add] - add;
  }
}

hipError_t merge_stack(hipStream_t s, uint32_t *labels, int slice_h, int w, size_t n_slices, const uint32_t *base, uint32_t *parent,
                       size_t n_colours) {
  const size_t n = (size_t)slice_h * w * n_slices;
  if (n == 0) return hipSuccess;
  const unsigned blocks = clamped_grid(n, 256, 16384);
  k_union_stack<<<blocks, 256, 0, s>>>(labels, slice_h, w, n, base, parent);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned fb = clamped_grid(n_colours, 256, 8192);
  k_uf_flatten<<<fb > 0 ? fb : 1, 256, 0, s>>>(parent, n_colours);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  k_relabel_stack<<<blocks, 256, 0, s>>>(labels, (size_t)slice_h * w, n, base, parent);
  return hipGetLastError();
}

}  // namespace wsk
