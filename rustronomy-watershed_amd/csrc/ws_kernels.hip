// ws_kernels.hip -- hand-written gfx950 (CDNA4, wave64) kernels of the watershed engine.
//
// No MFMA anywhere: the path is integer min/max/compare work on u8 / u32 planes.  The
// rules that matter are coalesced HBM rows, LDS-resident tiles, conflict-free LDS rows
// (lanes run along x) and wave-level reductions for convergence.
#include "ws_common.hpp"

#include <algorithm>
#include <cstdlib>

namespace wsk {

// ---------------------------------------------------------------- small utilities ----

__global__ void k_fill_u32(uint32_t *p, size_t n, uint32_t v) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) p[i] = v;
}

hipError_t fill_u32(hipStream_t s, uint32_t *p, size_t n, uint32_t v) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192);
  k_fill_u32<<<blocks, 256, 0, s>>>(p, n, v);
  return hipGetLastError();
}

// Zeroes a plane and two small arrays in ONE launch: the prologue of a fused transform clears the
// label plane, the tile-edge stamps and the flag words, and every separate memset is a launch plus
// a dependency gap (~10 us each).
typedef uint32_t u32x4_z __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2_z __attribute__((ext_vector_type(2)));
__global__ void k_zero3(uint32_t *a, size_t na, uint32_t *b, size_t nb, uint32_t *c, size_t nc) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  size_t head = (size_t)((16u - (unsigned)(reinterpret_cast<uintptr_t>(a) & 15u)) & 15u) >> 2;   // words up to 16-byte alignment
  if (head > na) head = na;
  const size_t body = (na - head) >> 2;
  u32x4_z *a4 = reinterpret_cast<u32x4_z *>(a + head);
  for (size_t i = tid; i < body; i += step) a4[i] = u32x4_z{0u, 0u, 0u, 0u};
  if (tid < head) a[tid] = 0u;
  for (size_t i = head + body * 4 + tid; i < na; i += step) a[i] = 0u;
  for (size_t i = tid; i < nb; i += step) b[i] = 0u;
  for (size_t i = tid; i < nc; i += step) c[i] = 0u;
}

hipError_t zero3(hipStream_t s, uint32_t *a, size_t na, uint32_t *b, size_t nb, uint32_t *c, size_t nc) {
  const size_t most = std::max(std::max(na / 4, nb), std::max(nc, (size_t)1));
  const int blocks = (int)std::min<size_t>((most + 255) / 256, 4096);
  k_zero3<<<blocks, 256, 0, s>>>(a, na, b, nb, c, nc);
  return hipGetLastError();
}

__device__ __forceinline__ uint64_t mix64(uint64_t x) {
  uint64_t z = x + 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__global__ void k_random_field(uint8_t *img, size_t stride, int h, int w, uint64_t base) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t n = (size_t)h * w, step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const size_t r = i / (size_t)w, c = i % (size_t)w;
    img[r * stride + c] = (uint8_t)(mix64(base + i) % 254u);
  }
}

hipError_t random_field(hipStream_t s, uint8_t *img, size_t stride, int h, int w, uint64_t seed) {
  const size_t n = (size_t)h * w;
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 16384 ? (n + 1023) / 1024 : 16384);
  k_random_field<<<blocks, 256, 0, s>>>(img, stride, h, w, seed << 40);
  return hipGetLastError();
}

// lib.rs:1670-1677: colour i+1 at seed i; a later duplicate overwrites an earlier one, i.e. the
// LARGEST colour painted on a pixel wins.  One atomicMax per seed costs ~35 ns of memory-side atomic
// each (7.3 M seeds: 250 us), so the painting is split: plain stores first (duplicates race, any of
// them lands), then a fix-up pass in which a seed whose colour is larger than what it finds there
// raises the pixel with atomicMax -- only duplicate seeds ever issue an atomic.
__global__ void k_scatter_seeds(const uint32_t *__restrict__ seeds_rc, const uint32_t *__restrict__ colours, size_t n, int ph,
                                int pw, uint32_t *labels, uint32_t *keys, uint32_t *err_flag, uint32_t *unsorted_flag) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint2 rc = reinterpret_cast<const uint2 *>(seeds_rc)[i];
    if (rc.x >= (uint32_t)ph || rc.y >= (uint32_t)pw) { atomicExch(err_flag, 1u); continue; }
    const size_t p = (size_t)rc.x * pw + rc.y;
    labels[p] = colours ? colours[i] : (uint32_t)(i + 1);
    if (keys) keys[p] = 0u;
    // a strictly increasing (row-major) list -- what find_local_minima returns -- cannot hold duplicates;
    // anything else arms the fix-up pass (plain idempotent store)
    if (i + 1 < n) {
      const uint2 nx = reinterpret_cast<const uint2 *>(seeds_rc)[i + 1];
      if ((size_t)nx.x * pw + nx.y <= p) *unsorted_flag = 1u;
    }
  }
}

__global__ void k_scatter_fixup(const uint32_t *__restrict__ seeds_rc, const uint32_t *__restrict__ colours, size_t n, int ph,
                                int pw, uint32_t *labels, const uint32_t *unsorted_flag) {
  if (*unsorted_flag == 0u) return;          // no duplicates possible: nothing to fix
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint2 rc = reinterpret_cast<const uint2 *>(seeds_rc)[i];
    if (rc.x >= (uint32_t)ph || rc.y >= (uint32_t)pw) continue;
    const size_t p = (size_t)rc.x * pw + rc.y;
    const uint32_t mine = colours ? colours[i] : (uint32_t)(i + 1);
    if (labels[p] < mine) atomicMax(&labels[p], mine);
  }
}

// err_flag points at two consecutive words: [0] seed out of bounds, [1] seed list not strictly increasing
hipError_t scatter_seeds(hipStream_t s, const uint32_t *seeds_rc, const uint32_t *colours, size_t n, int ph, int pw,
                         uint32_t *labels, uint32_t *keys, uint32_t *err_flag) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
  k_scatter_seeds<<<blocks, 256, 0, s>>>(seeds_rc, colours, n, ph, pw, labels, keys, err_flag, err_flag + 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_scatter_fixup<<<blocks, 256, 0, s>>>(seeds_rc, colours, n, ph, pw, labels, err_flag + 1);
  return hipGetLastError();
}

// ---- painting a whole label plane in one pass ------------------------------------------------
//
// memset + scatter writes the plane twice (the scatter's 4-byte stores dirty nearly every line of it
// again).  When the seed list is sorted by pixel index -- what find_local_minima returns -- a wave can
// instead FIND the seeds of its own 4096-pixel chunk (64-ary lower bound: 4 dependent probes for
// 7 M seeds) and walk down the list from there: per 256-pixel segment the seeds' colours are dropped
// into a 1 KiB LDS row and the segment is written once, 16 B per lane.
// Nothing is assumed: every wave also checks a slice of the list for order (and every seed for
// bounds); if any consecutive pair is out of order `unsorted` is raised and k_scatter_fixup, which
// runs next, raises every seed pixel to its largest seed index with atomicMax.  That is exact
// whatever the wave walks found, because a painted pixel always holds 0 or the colour of one of its
// own seeds.
constexpr int PAINT_SEG = 256;       // pixels per step of a wave: one 16-byte store per lane
constexpr int PAINT_STEPS = 16;      // consecutive segments per wave: one search, then a walk down the list
constexpr int PAINT_WAVES = 4;       // waves per workgroup

__device__ __forceinline__ unsigned long long seed_pos(uint2 rc, int pw) { return (unsigned long long)rc.x * (unsigned)pw + rc.y; }

// order and bounds of one wave's slice of the list.  flags: [0] seed out of bounds, [1] list not
// sorted, [2] list not strictly increasing
__device__ __forceinline__ void check_seed_slice(const uint2 *__restrict__ seeds, size_t n, int ph, int pw, size_t slice,
                                                 size_t nslices, int lane, uint32_t *flags) {
  const size_t per = (n + nslices - 1) / nslices;
  const size_t lo = slice * per, hi = lo + per < n ? lo + per : n;
  for (size_t j = lo + lane; j < hi; j += 64) {
    const uint2 a = seeds[j];
    if (a.x >= (uint32_t)ph || a.y >= (uint32_t)pw) atomicExch(&flags[0], 1u);
    if (j + 1 < n) {
      const unsigned long long pa = seed_pos(a, pw), pb = seed_pos(seeds[j + 1], pw);
      if (pb < pa) flags[1] = 1u;
      if (pb <= pa) flags[2] = 1u;
    }
  }
}

// 64-ary lower bound, one probe per lane and round: smallest j with pos(j) >= p0 (4 rounds for 7 M seeds).
// Terminates and stays inside [0, n] whatever the order of the list.
__device__ __forceinline__ size_t seed_lower_bound(const uint2 *__restrict__ seeds, size_t n, int pw, unsigned long long p0, int lane) {
  size_t lo = 0, hi = n;
  while (hi - lo > 64) {
    const size_t step = (hi - lo + 63) / 64;
    const size_t j = lo + (size_t)lane * step;
    const bool before = j < hi && seed_pos(seeds[j], pw) < p0;
    const int c = __popcll(__builtin_amdgcn_ballot_w64(before));
    if (c == 0) { hi = lo; break; }
    const size_t nlo = lo + (size_t)(c - 1) * step + 1, nhi = lo + (size_t)c * step;
    hi = nhi < hi ? nhi : hi;
    lo = nlo;
  }
  if (hi > lo) {
    const size_t j = lo + lane;
    const bool before = j < hi && seed_pos(seeds[j], pw) < p0;
    lo += __popcll(__builtin_amdgcn_ballot_w64(before));
  }
  return lo;
}

// Two lower bounds (pa <= pb) in one walk: the probes of both searches are in flight together, so a wave that needs both
// ends of its chunk pays the dependent round trips of one search (k_seed_tables is little else: 8 of its ~12).
__device__ __forceinline__ void seed_lower_bound2(const uint2 *__restrict__ seeds, size_t n, int pw, unsigned long long pa,
                                                  unsigned long long pb, int lane, size_t &out_a, size_t &out_b) {
  if (n == 0) { out_a = out_b = 0; return; }      // (no list to probe)
  size_t lo[2] = {0, 0}, hi[2] = {n, n};
  const unsigned long long p[2] = {pa, pb};
  while (hi[0] - lo[0] > 64 || hi[1] - lo[1] > 64) {
    size_t step[2], j[2];
    uint2 probe[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      step[k] = (hi[k] - lo[k] + 63) / 64;
      j[k] = lo[k] + (size_t)lane * step[k];
      probe[k] = seeds[j[k] < hi[k] ? j[k] : n - 1];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      if (hi[k] - lo[k] <= 64) continue;      // uniform
      const bool before = j[k] < hi[k] && seed_pos(probe[k], pw) < p[k];
      const int c = __popcll(__builtin_amdgcn_ballot_w64(before));
      if (c == 0) { hi[k] = lo[k]; continue; }
      const size_t nlo = lo[k] + (size_t)(c - 1) * step[k] + 1, nhi = lo[k] + (size_t)c * step[k];
      hi[k] = nhi < hi[k] ? nhi : hi[k];
      lo[k] = nlo;
    }
  }
  uint2 last[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) last[k] = seeds[lo[k] + lane < hi[k] ? lo[k] + lane : n - 1];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const bool before = hi[k] > lo[k] && lo[k] + lane < hi[k] && seed_pos(last[k], pw) < p[k];
    lo[k] += __popcll(__builtin_amdgcn_ballot_w64(before));
  }
  out_a = lo[0];
  out_b = lo[1];
}

__global__ __launch_bounds__(64 * PAINT_WAVES) void k_paint_sorted(const uint32_t *__restrict__ seeds_rc, size_t n, int ph, int pw,
                                                                  uint32_t *labels, size_t npx, size_t nchunk, int steps,
                                                                  uint32_t *err_flag,
                                                                  uint32_t *zero_a, size_t n_zero_a, uint32_t *zero_b, size_t n_zero_b) {
  __shared__ __attribute__((aligned(16))) uint32_t sRow[PAINT_WAVES][PAINT_SEG];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint2 *seeds = reinterpret_cast<const uint2 *>(seeds_rc);
  {   // side job: the small arrays the transform wants zeroed (tile-edge stamps, flag words)
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < n_zero_a; i += step) zero_a[i] = 0u;
    for (size_t i = tid; i < n_zero_b; i += step) zero_b[i] = 0u;
  }
  const size_t chunk = (size_t)blockIdx.x * PAINT_WAVES + wave;       // `steps` consecutive segments
  if (chunk >= nchunk) return;
  uint32_t *row = sRow[wave];
  const bool vec_ok = (reinterpret_cast<uintptr_t>(labels) & 15u) == 0;
  check_seed_slice(seeds, n, ph, pw, chunk, nchunk, lane, err_flag);      // independent loads, issued first
  unsigned long long p0 = (unsigned long long)chunk * (unsigned long long)(PAINT_SEG * steps);
  const size_t lo = seed_lower_bound(seeds, n, pw, p0, lane);

  // ---- walk: the list from `lo` on is cut into fixed windows of 64 seeds, one per lane; `off` is the
  // first lane of the current window that has not been painted yet.  A segment paints the run of
  // in-segment seeds from `off` on, across as many windows as it takes.  The window after the current
  // one is always in flight already, so no load latency is exposed after the first.
  size_t wbase = lo;                                   // list index of lane 0 of the current window
  int off = 0;
  uint2 cur = make_uint2(0u, 0u), nxt = make_uint2(0u, 0u);
  if (n) {
    cur = seeds[wbase + lane < n ? wbase + lane : n - 1];
    nxt = seeds[wbase + 64 + lane < n ? wbase + 64 + lane : n - 1];
  }
  for (int sgm = 0; sgm < steps && p0 < npx; ++sgm, p0 += PAINT_SEG) {
    const unsigned long long p1 = p0 + PAINT_SEG < npx ? p0 + PAINT_SEG : npx;
    *reinterpret_cast<u32x4_z *>(&row[lane * 4]) = u32x4_z{0u, 0u, 0u, 0u};
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the zeroed row before the colours
    for (;;) {
      const size_t j = wbase + lane;
      const unsigned long long pos = seed_pos(cur, pw);
      const bool ok = j < n && pos >= p0 && pos < p1;
      // lanes below `off` count as done; the run ends at the first lane from `off` on that is not in the segment
      const unsigned long long m = __builtin_amdgcn_ballot_w64(ok) | ((1ull << off) - 1ull);
      const int end = m == ~0ull ? 64 : __builtin_ctzll(~m);
      if (lane >= off && lane < end && cur.x < (uint32_t)ph && cur.y < (uint32_t)pw)
        atomicMax(&row[(uint32_t)(pos - p0)], (uint32_t)(j + 1));
      off = end;
      if (off < 64) break;
      wbase += 64;                                       // window exhausted: the prefetched one becomes current
      off = 0;
      cur = nxt;
      if (n) nxt = seeds[wbase + 64 + lane < n ? wbase + 64 + lane : n - 1];
      if (wbase >= n) break;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    // one 16-byte store per lane
    const u32x4_z v = *reinterpret_cast<const u32x4_z *>(&row[lane * 4]);
    const unsigned long long q = p0 + (unsigned long long)lane * 4;
    if (q + 4 <= npx && vec_ok) {
      *reinterpret_cast<u32x4_z *>(labels + q) = v;
    } else {
      const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) if (q + k < npx) labels[q + k] = e[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the row is read before it is zeroed again
  }
}

// The side tables of a STRICTLY increasing seed list: one bit per pixel ("is a seed") and, per
// 32-pixel word, the list index of the first seed of the word.  The colour of seed pixel p is then
//     word_base[p / 32] + popcount(mask[p / 32] & ((1 << p % 32) - 1)) + 1,
// 16 MiB of tables instead of a painted 256 MiB plane at 8192^2.  A wave owns TAB_WORDS words
// (8192 pixels): lower bound of the chunk start, then every window of 64 seeds drops its bits into a
// 1 KiB LDS row (no per-segment ordering: windows stream through four at a time), one wave scan of
// the word popcounts gives the bases.  Nothing here repairs a list that is not strictly increasing:
// flags[2] tells the caller, who repeats the transform with paint_labels.
constexpr int TAB_WORDS = 256;       // mask words per wave (8192 pixels): four per lane
constexpr int TAB_WIN = 4;           // windows of 64 list entries in flight per round of the walk

__global__ __launch_bounds__(64 * PAINT_WAVES) void k_seed_tables(const uint32_t *__restrict__ seeds_rc, size_t n, int ph, int pw,
                                                                 uint32_t *mask, uint32_t *word_base, size_t npx, size_t nchunk,
                                                                 uint32_t *flags,
                                                                 uint32_t *zero_a, size_t n_zero_a, uint32_t *zero_b, size_t n_zero_b,
                                                                 const uint32_t *__restrict__ slice_first, size_t slice_px, uint32_t colour_bias) {
  __shared__ __attribute__((aligned(16))) uint32_t sRow[PAINT_WAVES][TAB_WORDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint2 *seeds = reinterpret_cast<const uint2 *>(seeds_rc);
  {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < n_zero_a; i += step) zero_a[i] = 0u;
    for (size_t i = tid; i < n_zero_b; i += step) zero_b[i] = 0u;
  }
  const size_t chunk = (size_t)blockIdx.x * PAINT_WAVES + wave;
  if (chunk >= nchunk) return;
  uint32_t *row = sRow[wave];
  *reinterpret_cast<u32x4_z *>(&row[lane * 4]) = u32x4_z{0u, 0u, 0u, 0u};
  const unsigned long long p0 = (unsigned long long)chunk * (TAB_WORDS * 32);
  const unsigned long long p1 = p0 + TAB_WORDS * 32 < npx ? p0 + TAB_WORDS * 32 : npx;
  // The list is read ONCE, and the walk is also the proof that it is strictly increasing and in bounds: the wave takes
  // the list range [lo, hi) between the lower bounds of its chunk's two ends and checks that every seed in it lies in
  // the chunk, in the plane, and after its predecessor.  Neighbouring waves compute the bound they share by the same
  // search on the same list, so the ranges tile [0, n) whatever the list looks like (the last wave takes what is left);
  // if every range passes, the whole list is strictly increasing.  Anything else raises flags[2] (and flags[0] for a
  // seed outside the plane) and the caller repeats the transform with paint_labels, whose own checks name the fault.
  // (A separate pass over the list for these checks was 58 of the kernel's 161 MB.)
  size_t lo, hi;
  seed_lower_bound2(seeds, n, pw, p0, p1, lane, lo, hi);
  if (chunk + 1 == nchunk) hi = n;
  bool bad = hi < lo || hi - lo > (size_t)TAB_WORDS * 32;      // more seeds than pixels: not worth walking
  if (bad) hi = lo;
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the zeroed row before the bits

  // TAB_WIN windows of 64 seeds per round, all their loads in flight together (sixteen windows a round -- a chunk of the
  // bench field holds ~890 seeds -- changed nothing: of the kernel's 30 us the two searches are 9, the rest is the list
  // streaming through; profiles/r2_v7_chase_ab.log)
  unsigned long long prev_last = 0;      // position of the seed before the round's first (none: the first of the range)
  bool have_prev = false;
  for (size_t wbase = lo; wbase < hi; wbase += 64 * TAB_WIN) {
    uint2 win[TAB_WIN];
#pragma unroll
    for (int k = 0; k < TAB_WIN; ++k) {
      const size_t j = wbase + 64 * k + lane;
      win[k] = seeds[j < hi ? j : hi - 1];
    }
#pragma unroll
    for (int k = 0; k < TAB_WIN; ++k) {
      const size_t j = wbase + 64 * k + lane;
      const unsigned long long pos = seed_pos(win[k], pw);
      const bool mine = j < hi;
      const bool inside = win[k].x < (uint32_t)ph && win[k].y < (uint32_t)pw;
      // predecessor: the lane below, or the last lane of the window before (a clamped lane repeats the last seed: ignored)
      unsigned long long before = __shfl_up(pos, 1, 64);
      if (lane == 0) before = prev_last;
      const bool first_of_range = lane == 0 && !have_prev;
      if (mine && !inside) atomicExch(&flags[0], 1u);
      if (mine && (!inside || pos < p0 || pos >= p1 || (!first_of_range && pos <= before))) bad = true;
      if (mine && inside && pos >= p0 && pos < p1) {
        const uint32_t b = (uint32_t)(pos - p0);
        atomicOr(&row[b >> 5], 1u << (b & 31u));
      }
      prev_last = __shfl(pos, 63, 64);
      have_prev = true;
    }
  }
  if (__builtin_amdgcn_ballot_w64(bad) != 0ull && lane == 0) { flags[1] = 1u; flags[2] = 1u; }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");

  // lane l owns words 4l .. 4l+3 of the chunk: exclusive scan of their popcounts = seeds before them
  const u32x4_z w = *reinterpret_cast<const u32x4_z *>(&row[lane * 4]);
  const uint32_t c0 = __popc(w.x), c1 = __popc(w.y), c2 = __popc(w.z), cnt = c0 + c1 + c2 + __popc(w.w);
  const uint32_t incl = wave_inclusive_sum(cnt);
  uint32_t b0 = (uint32_t)lo + incl - cnt;
  // a stack of slices (slice_px % 128 == 0: a lane's four words lie in one slice): list indices count from the slice's first seed
  if (slice_first) {      // (clamped twice over for lists that are not what they should be: the slice index and the difference)
    const size_t npx_slices = (size_t)((npx + slice_px - 1) / slice_px);
    const uint32_t sf = slice_first[min((size_t)((p0 + 128ull * (unsigned)lane) / slice_px), npx_slices)];
    b0 = b0 >= sf ? b0 - sf : 0u;
  }
  // a row block of a larger field: its seeds are entries [g0, g0 + n) of the caller's list, so colours start at g0 + 1
  b0 += colour_bias;
  const u32x4_z bases = u32x4_z{b0, b0 + c0, b0 + c0 + c1, b0 + c0 + c1 + c2};
  const size_t wi = (size_t)(p0 >> 5) + 4 * lane, nwords = (npx + 31) / 32;
  if (wi + 4 <= nwords && ((reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(word_base)) & 15u) == 0) {
    *reinterpret_cast<u32x4_z *>(mask + wi) = w;
    *reinterpret_cast<u32x4_z *>(word_base + wi) = bases;
  } else {
    const uint32_t wv[4] = {w.x, w.y, w.z, w.w}, bv[4] = {bases.x, bases.y, bases.z, bases.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) if (wi + k < nwords) { mask[wi + k] = wv[k]; word_base[wi + k] = bv[k]; }
  }
}

// ---- the same tables in LIST order: one read of the list, no search on the way to it ----------------
//
// k_seed_tables gives a wave 8192 pixels, so the wave must FIND its seeds: two 64-ary lower bounds, 4-5 dependent round
// trips before the first useful load.  For a dense list ownership can go by list position instead: a wave takes the
// STREAM_E entries [i0, i0 + STREAM_E), all their loads in flight at once, plus entry i0 - 1 and 32 entries of look-ahead.
//   - a mask word belongs to the wave whose window holds the word's FIRST seed: the wave skips its leading entries that
//     fall into the word of entry i0 - 1 and takes from the look-ahead the entries of its own last word (a word holds at
//     most 32 seeds, so it is shared by two windows at the most);
//   - a run of empty words belongs to the wave that holds the next seed after it, the run behind the last seed to the
//     last wave; the base of an empty word is the number of seeds before it, as in k_seed_tables (k_resolve_local reads
//     `first` from such words);
//   - the wave walks its span of words in pieces of STREAM_ROW words through an LDS row (bits by atomicOr, one wave scan of
//     the popcounts); a run of empty words before the next seed is written straight from registers, (0, base).
// One window may own a very long run (all seeds in one half of the plane), which one wave would write alone.  So every
// aligned chunk of STREAM_BIG words that lies wholly inside one run is left to the plane waves of the same launch: one wave
// per chunk, the first blocks of the grid, each with one double lower bound (equal ends: the chunk is empty, and the bound
// is its base).  Chunks that the list waves reach through their rows are written twice, with the same words.
// The walk is the proof of the list, as in k_seed_tables: every entry is tested once for "in the plane" and "after its
// predecessor", across windows through entry i0 - 1.  A wave that sees anything else raises the error words and writes
// nothing; a word index is only ever formed from a position inside the plane, and every fill is bounded by nwords.
constexpr int STREAM_E = 1024;            // list entries per wave: sixteen 8-byte loads per lane
constexpr int STREAM_K = STREAM_E / 64;
constexpr int STREAM_ROW = 512;           // words of a wave's LDS row: eight per lane
constexpr uint32_t STREAM_BIG = 4096;     // words of a chunk that a plane wave fills when no seed lies in it
constexpr size_t STREAM_PX_PER_SEED = 16; // seed_tables' rule: this kernel for lists of one seed per so many pixels, or denser

// The wave's steps across lanes without LDS (a __shfl is a ds_bpermute; with some eighty of them per wave the CU's one LDS
// pipe was a good part of the kernel): a lane's value as a scalar, the value of the lane below by a DPP wave shift, the
// minimum by the DPP row shifts and row broadcasts of wave_inclusive_sum.
__device__ __forceinline__ uint32_t lane_value(uint32_t v, int l) { return (uint32_t)__builtin_amdgcn_readlane((int)v, l); }

// lane l: the value of lane l - 1; lane 0: `first`
__device__ __forceinline__ uint32_t lane_below_or(uint32_t v, uint32_t first) {
  return (uint32_t)__builtin_amdgcn_update_dpp((int)first, (int)v, 0x138, 0xF, 0xF, false);      // wave_shr:1
}

__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) {
#define WS_DPP_MIN(ctrl, rows) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)v, ctrl, rows, 0xF, false))
  WS_DPP_MIN(0x111, 0xF);      // row_shr:1
  WS_DPP_MIN(0x112, 0xF);      // row_shr:2
  WS_DPP_MIN(0x114, 0xF);      // row_shr:4
  WS_DPP_MIN(0x118, 0xF);      // row_shr:8
  WS_DPP_MIN(0x142, 0xA);      // row_bcast:15
  WS_DPP_MIN(0x143, 0xC);      // row_bcast:31
#undef WS_DPP_MIN
  return lane_value(v, 63);      // lane 63 holds the minimum of all
}

// the value again, but new to the compiler: what is computed from it inside a loop stays inside (sixteen words and sixteen
// bit masks hoisted out of the walk below cost the kernel its eighth wave)
__device__ __forceinline__ uint32_t opaque_u32(uint32_t v) {
  asm volatile("" : "+v"(v));
  return v;
}

struct TableOut {
  uint32_t *mask, *word_base;
  bool vec_ok;                          // both 16-byte aligned
  const uint32_t *slice_first;          // stack of slices (slice_px % 128 == 0: an aligned quad of words lies in one slice)
  uint32_t slice_quads, nslices;        // quads of words per slice (npx < 2^32), slices
  uint32_t colour_bias;
};

// the base of the first word of the aligned quad q, from the number of list entries before it: exactly k_seed_tables' rule
__device__ __forceinline__ uint32_t table_base(const TableOut &t, uint32_t before, uint32_t q) {
  if (t.slice_first) {
    const uint32_t sf = t.slice_first[min((q >> 2) / t.slice_quads, t.nslices)];
    before = before >= sf ? before - sf : 0u;
  }
  return before + t.colour_bias;
}

// words q .. q + 3 (q % 4 == 0) of both tables: those inside [lo, hi] only
__device__ __forceinline__ void store_quad(const TableOut &t, uint32_t q, uint32_t lo, uint32_t hi, u32x4_z m, u32x4_z b) {
  if (q >= lo && q + 3 <= hi && t.vec_ok) {
    *reinterpret_cast<u32x4_z *>(t.mask + q) = m;
    *reinterpret_cast<u32x4_z *>(t.word_base + q) = b;
  } else {
    const uint32_t mv[4] = {m.x, m.y, m.z, m.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) if (q + k >= lo && q + k <= hi) { t.mask[q + k] = mv[k]; t.word_base[q + k] = bv[k]; }
  }
}

// empty words [a, b) with `before` list entries before them; b <= nwords
__device__ __forceinline__ void fill_empty(const TableOut &t, uint32_t a, uint32_t b, uint32_t before, int lane) {
  if (a >= b) return;
  for (uint32_t q = (a & ~3u) + 4u * lane; q < b; q += 256u) {
    const uint32_t v = table_base(t, before, q);
    store_quad(t, q, a, b - 1, u32x4_z{0u, 0u, 0u, 0u}, u32x4_z{v, v, v, v});
  }
}

__global__ __launch_bounds__(64 * PAINT_WAVES) void k_seed_tables_stream(const uint32_t *__restrict__ seeds_rc, size_t n, int ph, int pw,
                                                                        uint32_t *mask, uint32_t *word_base, size_t npx, uint32_t nwords,
                                                                        uint32_t plane_blocks, uint32_t *flags,
                                                                        uint32_t *zero_a, size_t n_zero_a, uint32_t *zero_b, size_t n_zero_b,
                                                                        const uint32_t *__restrict__ slice_first, uint32_t slice_quads, uint32_t nslices,
                                                                        uint32_t colour_bias) {
  __shared__ __attribute__((aligned(16))) uint32_t sRow[PAINT_WAVES][STREAM_ROW];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint2 *seeds = reinterpret_cast<const uint2 *>(seeds_rc);
  {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < n_zero_a; i += step) zero_a[i] = 0u;
    for (size_t i = tid; i < n_zero_b; i += step) zero_b[i] = 0u;
  }
  if (n == 0) return;      // (seed_tables never sends an empty list here)
  TableOut t;
  t.mask = mask; t.word_base = word_base;
  t.vec_ok = ((reinterpret_cast<uintptr_t>(mask) | reinterpret_cast<uintptr_t>(word_base)) & 15u) == 0;
  t.slice_first = slice_first; t.slice_quads = slice_quads; t.nslices = nslices;
  t.colour_bias = colour_bias;

  if (blockIdx.x < plane_blocks) {      // ---- a plane wave: one aligned chunk of STREAM_BIG words, filled if it holds no seed
    const uint32_t c = blockIdx.x * PAINT_WAVES + wave;
    if (c >= (nwords + STREAM_BIG - 1) / STREAM_BIG) return;
    const uint32_t a = c * STREAM_BIG, b = min(a + STREAM_BIG, nwords);
    const unsigned long long p0 = (unsigned long long)a * 32u, p1 = min((unsigned long long)b * 32u, (unsigned long long)npx);
    size_t lo, hi;
    seed_lower_bound2(seeds, n, pw, p0, p1, lane, lo, hi);      // inside [0, n] whatever the list
    if (lo == hi) fill_empty(t, a, b, (uint32_t)lo, lane);
    return;
  }

  // ---- a list wave.  Its loads go through a buffer descriptor over entries [i0 - 1, i0 + STREAM_E + 32) of the list, cut at
  // its end: the hardware's range check is the clamp (a load behind the end returns zeros, and `mine` drops it), and one
  // 32-bit offset per lane serves all seventeen loads -- with sixteen 64-bit addresses the kernel held 84 VGPRs.
  const size_t i0 = ((size_t)(blockIdx.x - plane_blocks) * PAINT_WAVES + (size_t)__builtin_amdgcn_readfirstlane(wave)) * STREAM_E;
  if (i0 >= n) return;
  const bool last = i0 + STREAM_E >= n;
  const uint32_t here = (uint32_t)min(n - i0, (size_t)STREAM_E);      // entries of this window
  const uint32_t lead = i0 ? 1u : 0u;                                  // entry i0 - 1 in front
  const uint32_t reach = lead + (uint32_t)min(n - i0, (size_t)(STREAM_E + 32));
  // (the descriptor from wave-uniform words, said so to the compiler: otherwise every load sits in a loop over lanes)
  const uintptr_t bp = reinterpret_cast<uintptr_t>(seeds + (i0 - lead));
  const uintptr_t bu = ((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(bp >> 32)) << 32) |
                       (uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bp);
  const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(
      reinterpret_cast<void *>(bu), 0, __builtin_amdgcn_readfirstlane((int)(reach * 8u)), 0x00020000);
  const uint32_t off = (lead + (uint32_t)lane) * 8u;
  uint2 ent[STREAM_K];
#pragma unroll
  for (int k = 0; k < STREAM_K; ++k) {
    const u32x2_z v = __builtin_amdgcn_raw_buffer_load_b64(rsrc, off + 512u * k, 0, 0);
    ent[k] = make_uint2(v.x, v.y);
  }
  // lanes 0 .. 31: the look-ahead; lane 63: entry i0 - 1 (offset 0; the list's first entry, not used, in the first window)
  const u32x2_z vx = __builtin_amdgcn_raw_buffer_load_b64(rsrc, lane < 32 ? off + 8u * STREAM_E : 0u, 0, 0);
  const uint2 ex = make_uint2(vx.x, vx.y);
  // positions in 32 bits (npx < 2^32: seed_tables' rule; word p >> 5, bit p & 31), ~0 for an entry outside the plane or behind
  // the end of the list: that is the word 2^27 - 1, behind every plane, and never "after" anything
  const uint32_t x32 = ex.x < (uint32_t)ph && ex.y < (uint32_t)pw ? (uint32_t)seed_pos(ex, pw) : 0xFFFFFFFFu;
  const uint32_t prev32 = lane_value(x32, 63);

  uint32_t p32[STREAM_K];
  uint32_t bad = 0u;      // bit 0: not after its predecessor; bit 1: outside the plane
  uint32_t carry = prev32;      // the entry before lane 0's (uniform)
#pragma unroll
  for (int k = 0; k < STREAM_K; ++k) {
    const bool mine = 64u * k + lane < here;
    const bool inside = ent[k].x < (uint32_t)ph && ent[k].y < (uint32_t)pw;
    const uint32_t p = mine && inside ? (uint32_t)seed_pos(ent[k], pw) : 0xFFFFFFFFu;
    const uint32_t before = lane_below_or(p, carry);
    const bool has_pred = lane > 0 || k > 0 || i0 > 0;
    bad |= (mine && has_pred && p <= before ? 1u : 0u) | (mine && !inside ? 2u : 0u);      // (a predecessor outside the plane: ~0, "not after" too)
    carry = lane_value(p, 63);
    p32[k] = p;
  }
  if (__builtin_amdgcn_ballot_w64(bad != 0u) != 0ull) {      // not a strictly increasing in-plane window: nothing is written
    if (bad & 2u) atomicExch(&flags[0], 1u);
    if (lane == 0) { flags[1] = 1u; flags[2] = 1u; }
    return;
  }
  if (i0 > 0 && prev32 == 0xFFFFFFFFu) return;      // (entry i0 - 1 outside the plane: its own window has raised the words)

  // from here on the window is strictly increasing, in the plane, and after entry i0 - 1
  const uint32_t Wf = i0 ? (prev32 >> 5) + 1u : 0u;                                        // first owned word
  const uint32_t Wl = last ? nwords - 1u : lane_value(p32[STREAM_K - 1], 63) >> 5;      // last owned word
  if (Wl < Wf) return;      // the whole window in the word of entry i0 - 1: only a list that another wave refuses
  const bool x_ok = !last && lane < 32 && i0 + STREAM_E + lane < n && (x32 >> 5) == Wl;
  uint32_t nskip = 0;      // (uniform: popcounts of ballots)
#pragma unroll
  for (int k = 0; k < STREAM_K; ++k)
    nskip += (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((p32[k] >> 5) < Wf));

  uint32_t *row = sRow[wave];
  uint32_t ws = Wf, running = (uint32_t)i0 + nskip;      // words before ws are done; `running` list entries lie before ws
  while (ws <= Wl) {
    uint32_t m = x_ok ? Wl : 0xFFFFFFFFu;      // the next word that holds a seed
#pragma unroll
    for (int k = 0; k < STREAM_K; ++k) {
      const uint32_t w = opaque_u32(p32[k]) >> 5;
      if (w >= ws && w <= Wl) m = min(m, w);
    }
    m = wave_min_u32(m);
    const uint32_t g = m == 0xFFFFFFFFu ? Wl + 1u : m;
    {      // the empty run [ws, g), without the aligned STREAM_BIG chunks wholly inside it (the plane waves')
      const uint32_t cs = (ws + STREAM_BIG - 1u) & ~(STREAM_BIG - 1u), ce = g & ~(STREAM_BIG - 1u);
      const bool cut = cs < ce;
#pragma unroll 1
      for (int part = 0; part < (cut ? 2 : 1); ++part) fill_empty(t, part ? ce : ws, part || !cut ? g : cs, running, lane);
    }
    if (g > Wl) break;
    const uint32_t rb = g & ~3u;                                     // the row starts at an aligned quad; words [g, pe] are written
    const uint32_t pe = min(rb + (uint32_t)STREAM_ROW - 1u, Wl);
    *reinterpret_cast<u32x4_z *>(&row[lane * 8]) = u32x4_z{0u, 0u, 0u, 0u};
    *reinterpret_cast<u32x4_z *>(&row[lane * 8 + 4]) = u32x4_z{0u, 0u, 0u, 0u};
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the zeroed row before the bits
#pragma unroll
    for (int k = 0; k < STREAM_K; ++k) {
      const uint32_t p = opaque_u32(p32[k]), w = p >> 5;
      if (w >= g && w <= pe) atomicOr(&row[w - rb], 1u << (p & 31u));
    }
    if (x_ok && Wl <= pe) atomicOr(&row[Wl - rb], 1u << (x32 & 31u));
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    const u32x4_z wa = *reinterpret_cast<const u32x4_z *>(&row[lane * 8]);
    const u32x4_z wb = *reinterpret_cast<const u32x4_z *>(&row[lane * 8 + 4]);
    const uint32_t a0 = __popc(wa.x), a1 = __popc(wa.y), a2 = __popc(wa.z), ca = a0 + a1 + a2 + __popc(wa.w);
    const uint32_t b0 = __popc(wb.x), b1 = __popc(wb.y), b2 = __popc(wb.z), cnt = ca + b0 + b1 + b2 + __popc(wb.w);
    const uint32_t incl = wave_inclusive_sum(cnt);
    const uint32_t before = running + incl - cnt;      // list entries before this lane's eight words
    const uint32_t q = rb + 8u * lane;
    const uint32_t ba = table_base(t, before, q), bb = table_base(t, before + ca, q + 4u);
    store_quad(t, q, g, pe, wa, u32x4_z{ba, ba + a0, ba + a0 + a1, ba + a0 + a1 + a2});
    store_quad(t, q + 4u, g, pe, wb, u32x4_z{bb, bb + b0, bb + b0 + b1, bb + b0 + b1 + b2});
    running += lane_value(incl, 63);
    ws = pe + 1u;
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the row is read before it is zeroed again
  }
}

static int paint_steps() {
  static const int steps = [] {
    const char *e = tuning_env("WS_PAINT_STEPS");      // tuning knob, tools/ only
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : PAINT_STEPS;
  }();
  return steps;
}

// Paints colour i + 1 at seed i over a zeroed plane, later duplicates winning (lib.rs:1672-1677), in
// one pass over the plane plus a fix-up that only works when the list is not sorted.  Also zeroes two
// small arrays.  err_flag points at three consecutive words (out of bounds, unsorted, not strictly
// increasing); they must be zero.
hipError_t paint_labels(hipStream_t s, const uint32_t *seeds_rc, size_t n, int ph, int pw, uint32_t *labels,
                        uint32_t *err_flag, uint32_t *zero_a, size_t n_zero_a, uint32_t *zero_b, size_t n_zero_b) {
  const size_t npx = (size_t)ph * pw;
  const int steps = paint_steps();
  const size_t per_wave = (size_t)PAINT_SEG * steps;
  const size_t nchunk = (npx + per_wave - 1) / per_wave;
  const size_t blocks = std::max<size_t>((nchunk + PAINT_WAVES - 1) / PAINT_WAVES, 1);
  k_paint_sorted<<<(unsigned)blocks, 64 * PAINT_WAVES, 0, s>>>(seeds_rc, n, ph, pw, labels, npx, nchunk, steps, err_flag,
                                                              zero_a, n_zero_a, zero_b, n_zero_b);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n == 0) return e;
  const int fb = (int)((n + 255) / 256 < 16384 ? (n + 255) / 256 : 16384);
  k_scatter_fixup<<<fb, 256, 0, s>>>(seeds_rc, nullptr, n, ph, pw, labels, err_flag + 1);
  return hipGetLastError();
}

// `mask` and `word_base` hold (ph * pw + 31) / 32 words each.  The caller reads err_flag[2] ("not strictly
// increasing") back and, if it is raised, repeats the transform with paint_labels.
hipError_t seed_tables(hipStream_t s, const uint32_t *seeds_rc, size_t n, int ph, int pw, uint32_t *mask, uint32_t *word_base,
                       uint32_t *err_flag, uint32_t *zero_a, size_t n_zero_a, uint32_t *zero_b, size_t n_zero_b,
                       const uint32_t *slice_first, size_t slice_px, uint32_t colour_bias) {
  const size_t npx = (size_t)ph * pw;
  // Which builder: from what the host knows, n and the plane (fixed for a captured graph, which is replayed only when
  // buffers and n repeat).  The list-order kernel for lists of one seed per STREAM_PX_PER_SEED pixels or denser; an
  // empty or sparser list keeps the searches, which are cheap on a short list and spread the empty words over the device
  // (profiles/seed_stream_density.txt).
  static const int forced = [] { const char *e = tuning_env("WS_SEED_STREAM"); return e ? atoi(e) : -1; }();      // A/B knob for tools/
  bool stream = n > 0 && n < ((size_t)1 << 32) && npx < ((size_t)1 << 32) && n * STREAM_PX_PER_SEED >= npx;
  if (forced >= 0) stream = forced > 0 && n > 0 && n < ((size_t)1 << 32) && npx < ((size_t)1 << 32);
  if (stream) {
    const uint32_t nwords = (uint32_t)((npx + 31) / 32);
    const uint32_t plane_blocks = ((nwords + STREAM_BIG - 1) / STREAM_BIG + PAINT_WAVES - 1) / PAINT_WAVES;
    const size_t list_blocks = ((n + STREAM_E - 1) / STREAM_E + PAINT_WAVES - 1) / PAINT_WAVES;
    // slices in quads of words (slice_px % 128 == 0), and their number: k_seed_tables' clamp of the slice index
    const uint32_t slice_quads = slice_first ? (uint32_t)std::max<size_t>(std::min<size_t>(slice_px / 128, 0xFFFFFFFFu), 1) : 1u;
    const uint32_t nslices = slice_first ? (uint32_t)((npx + slice_px - 1) / slice_px) : 0u;
    k_seed_tables_stream<<<(unsigned)(plane_blocks + list_blocks), 64 * PAINT_WAVES, 0, s>>>(
        seeds_rc, n, ph, pw, mask, word_base, npx, nwords, plane_blocks, err_flag, zero_a, n_zero_a, zero_b, n_zero_b, slice_first,
        slice_quads, nslices, colour_bias);
    return hipGetLastError();
  }
  const size_t per_wave = (size_t)TAB_WORDS * 32;
  const size_t nchunk = (npx + per_wave - 1) / per_wave;
  const size_t blocks = std::max<size_t>((nchunk + PAINT_WAVES - 1) / PAINT_WAVES, 1);
  k_seed_tables<<<(unsigned)blocks, 64 * PAINT_WAVES, 0, s>>>(seeds_rc, n, ph, pw, mask, word_base, npx, nchunk, err_flag,
                                                             zero_a, n_zero_a, zero_b, n_zero_b, slice_first, slice_px, colour_bias);
  return hipGetLastError();
}

// Seed i of a batch belongs to the slice k with slice_first[k] <= i < slice_first[k + 1]; in the stacked plane it sits
// k * slice_h rows further down.  A seed outside its own slice must not land in a neighbour: it becomes (~0, ~0), which
// every seed kernel reports as out of bounds.
__global__ void k_stack_seeds(const uint2 *__restrict__ seeds, size_t n, const uint32_t *__restrict__ slice_first, size_t n_slices,
                              int slice_h, int pw, uint2 *out, uint32_t shift) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    size_t lo = 0, hi = n_slices;            // largest k with slice_first[k] <= i
    while (hi - lo > 1) {
      const size_t mid = (lo + hi) / 2;
      if (slice_first[mid] <= i) lo = mid; else hi = mid;
    }
    uint2 rc = seeds[i];
    // shift: seed_shift with edge correction (ws_hip.h); compared before the add, so that ~0 cannot wrap into the plane
    const bool ok = rc.x < (uint32_t)slice_h - shift && rc.y < (uint32_t)pw - shift;
    rc.x += shift; rc.y += shift;
    out[i] = ok ? make_uint2(rc.x + (uint32_t)lo * (uint32_t)slice_h, rc.y) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  }
}

hipError_t stack_seeds(hipStream_t s, const uint32_t *seeds_rc, size_t n, const uint32_t *slice_first, size_t n_slices,
                       int slice_h, int pw, uint32_t *stacked_rc, uint32_t shift) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
  k_stack_seeds<<<blocks, 256, 0, s>>>(reinterpret_cast<const uint2 *>(seeds_rc), n, slice_first, n_slices, slice_h, pw,
                                       reinterpret_cast<uint2 *>(stacked_rc), shift);
  return hipGetLastError();
}

// seed_shift (ws_hip.h): every seed moves by (+shift, +shift); a coordinate that cannot move without wrapping becomes ~0,
// which every seed kernel reports as out of bounds
__global__ void k_shift_seeds(const uint2 *__restrict__ src, size_t n, uint32_t shift, uint2 *dst) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint2 rc = src[i];
    const bool ok = rc.x < 0xFFFFFFFFu - shift && rc.y < 0xFFFFFFFFu - shift;
    dst[i] = ok ? make_uint2(rc.x + shift, rc.y + shift) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  }
}

hipError_t shift_seeds(hipStream_t s, const uint32_t *src, size_t n, uint32_t shift, uint32_t *dst) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
  k_shift_seeds<<<blocks, 256, 0, s>>>(reinterpret_cast<const uint2 *>(src), n, shift, reinterpret_cast<uint2 *>(dst));
  return hipGetLastError();
}

// The host ABI's seeds are pairs of 64-bit words (Rust's (usize, usize)); the engine's are 32-bit.  A coordinate outside
// the (padded) plane -- the reference panics there, lib.rs:1675-1677 -- becomes ~0, which every seed kernel reports
// as out of bounds.  (This loop used to run on the host: 5 ms for the 7.3 M seeds of the bench field.)
__global__ void k_narrow_seeds(const uint64_t *__restrict__ src, size_t n, uint64_t ph, uint64_t pw, uint2 *dst, uint64_t shift) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint64_t r = src[2 * i], c = src[2 * i + 1];      // (ph, pw >= shift: the plane is padded whenever shift is 1)
    dst[i] = (r < ph - shift && c < pw - shift) ? make_uint2((uint32_t)(r + shift), (uint32_t)(c + shift)) : make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
  }
}

hipError_t narrow_seeds(hipStream_t s, const uint64_t *src, size_t n, size_t ph, size_t pw, uint32_t *dst, uint32_t shift) {
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 8192);
  k_narrow_seeds<<<blocks, 256, 0, s>>>(src, n, ph, pw, reinterpret_cast<uint2 *>(dst), shift);
  return hipGetLastError();
}

__global__ void k_widen(const uint32_t *src, uint64_t *dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) dst[i] = src[i];
}

hipError_t widen_labels(hipStream_t s, const uint32_t *src, uint64_t *dst, size_t n) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192);
  k_widen<<<blocks, 256, 0, s>>>(src, dst, n);
  return hipGetLastError();
}

hipError_t widen_pairs(hipStream_t s, const uint32_t *src, uint64_t *dst, size_t n_values) {
  return widen_labels(s, src, dst, n_values);
}

// ... and back: 64-bit words that are known to fit 32 bits (lake records: a colour and an area of a plane below 2^31 pixels), so
// that they cross the bus as half the bytes and are widened again by the host's threads (ws_hostcopy.hip)
__global__ void k_narrow_words(const uint64_t *__restrict__ src, uint32_t *__restrict__ dst, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) dst[i] = (uint32_t)src[i];
}

hipError_t narrow_words(hipStream_t s, const uint64_t *src, uint32_t *dst, size_t n) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192);
  k_narrow_words<<<blocks, 256, 0, s>>>(src, dst, n);
  return hipGetLastError();
}

// Label plane as the reference's hook sees it after `level` (lib.rs:1796-1804): a pixel
// is coloured once its arrival level is <= level; segmenting colours never change later.
__global__ void k_snapshot(const uint32_t *keys, const uint32_t *labels, uint64_t *dst, size_t n,
                           uint32_t level) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint32_t k = keys[i];
    dst[i] = (k != KEY_INF && (k >> 24) <= level) ? (uint64_t)labels[i] : 0ull;
  }
}

// the same into a u32 plane on the device (ws_level_snapshot_device): 16-byte accesses where the planes allow
__global__ void k_snapshot_u32(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, uint32_t *dst, size_t n, uint32_t level) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint32_t k = keys[i];
    dst[i] = (k != KEY_INF && (k >> 24) <= level) ? labels[i] : 0u;
  }
}

hipError_t snapshot_level_u32(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *dst, size_t n, uint32_t level) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 16384 ? (n + 1023) / 1024 : 16384);
  k_snapshot_u32<<<blocks, 256, 0, s>>>(keys, labels, dst, n, level);
  return hipGetLastError();
}

hipError_t snapshot_level(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint64_t *dst,
                          size_t n, uint32_t level) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192);
  k_snapshot<<<blocks, 256, 0, s>>>(keys, labels, dst, n, level);
  return hipGetLastError();
}

// (the flag words a replayed graph sends to the host's pinned mirror: no kernel of their own any more -- inside a graph two
// device-to-host copy nodes were blit kernels with barriers around them, then one small launch here, idle time at the end
// of every transform either way; k_resolve_chase copies them now, ResolveJob::read_back)

typedef uint32_t u32x4_r __attribute__((ext_vector_type(4)));

// ------------------------------------------------ sweep engine: one flood step -------
//
// lib.rs:196-257 one-to-one: every interior pixel that is flooded (img <= level),
// uncoloured and has a coloured 4-neighbour takes the first coloured neighbour in
// down,right,left,up order; reads only the previous plane (lin), writes the next (lout).

// first coloured neighbour in down, right, left, up order (lib.rs:190, 237-248 with col0)
__device__ __forceinline__ uint32_t pick_drlu(uint32_t d, uint32_t r, uint32_t l, uint32_t u) {
  return d ? d : (r ? r : (l ? l : u));
}

// scalar form: any width / alignment.  All loads unconditional on clamped addresses; the "something
// was coloured" word is a plain idempotent store (one shared atomic per workgroup would serialise).
__global__ __launch_bounds__(256) void k_flood_step(const uint8_t *__restrict__ img, size_t img_stride,
                                                    const uint32_t *__restrict__ lin, uint32_t *__restrict__ lout,
                                                    int H, int W, uint32_t level, uint32_t *counter, int pad, int y0) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = y0 + blockIdx.y * 4 + (threadIdx.x >> 6);
  const int xc = min(x, W - 1), yc = min(y, H - 1);
  const int xm = max(xc - 1, 0), xp = min(xc + 1, W - 1), ym = max(yc - 1, 0), yp = min(yc + 1, H - 1);
  const uint32_t c = lin[(size_t)yc * W + xc];
  const uint32_t d = lin[(size_t)yp * W + xc], r = lin[(size_t)yc * W + xp];
  const uint32_t l = lin[(size_t)yc * W + xm], u = lin[(size_t)ym * W + xc];
  const uint32_t v = img[pad ? padded_img_index(yc, xc, W, H, img_stride) : (size_t)yc * img_stride + xc];      // pad: virtual ring of zeros (ws_common.hpp)
  const bool floodable = c == 0u && y >= 1 && y < H - 1 && x >= 1 && x < W - 1 && v <= level;   // lib.rs:224-226
  const uint32_t pick = floodable ? pick_drlu(d, r, l, u) : 0u;
  if (x < W && y < H) lout[(size_t)y * W + x] = c ? c : pick;
  if (pick && x < W && y < H) *counter = 1u;
}

// vector form (W % 4 == 0, image rows dword aligned): a thread owns 4 consecutive pixels; labels move
// as 16-byte vectors, the image as one dword; a workgroup covers 1024 pixels of one row
__global__ __launch_bounds__(256) void k_flood_step4(const uint8_t *__restrict__ img, size_t img_stride,
                                                     const uint32_t *__restrict__ lin, uint32_t *__restrict__ lout,
                                                     int H, int W, uint32_t level, uint32_t *counter, int y0) {
  const int y = y0 + blockIdx.y;
  const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (x0 >= W) return;
  const int ym = max(y - 1, 0), yp = min(y + 1, H - 1);
  const u32x4_r c = *reinterpret_cast<const u32x4_r *>(lin + (size_t)y * W + x0);
  const u32x4_r dn = *reinterpret_cast<const u32x4_r *>(lin + (size_t)yp * W + x0);
  const u32x4_r up = *reinterpret_cast<const u32x4_r *>(lin + (size_t)ym * W + x0);
  const uint32_t lft = lin[(size_t)y * W + max(x0 - 1, 0)], rgt = lin[(size_t)y * W + min(x0 + 4, W - 1)];
  const uint32_t iv = *reinterpret_cast<const uint32_t *>(img + (size_t)y * img_stride + x0);
  const bool row_int = y >= 1 && y < H - 1;
  const uint32_t cc[4] = {c.x, c.y, c.z, c.w}, dd[4] = {dn.x, dn.y, dn.z, dn.w}, uu[4] = {up.x, up.y, up.z, up.w};
  const uint32_t ll[4] = {lft, c.x, c.y, c.z}, rr[4] = {c.y, c.z, c.w, rgt};
  uint32_t out[4], any = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int x = x0 + k;
    const bool floodable = cc[k] == 0u && row_int && x >= 1 && x < W - 1 && ((iv >> (8 * k)) & 0xFFu) <= level;
    const uint32_t pick = floodable ? pick_drlu(dd[k], rr[k], ll[k], uu[k]) : 0u;
    out[k] = cc[k] ? cc[k] : pick;
    any |= pick;
  }
  *reinterpret_cast<u32x4_r *>(lout + (size_t)y * W + x0) = u32x4_r{out[0], out[1], out[2], out[3]};
  if (any) *counter = 1u;
}

// (gridDim.y holds at most GRID_Y_MAX rows -- row groups of four in the scalar form: a taller plane goes in runs of rows, every
// run the same kernel from its first row y0 on; a plane below that height is one launch as before)
hipError_t flood_step(hipStream_t s, const uint8_t *img, size_t img_stride, const uint32_t *lin,
                      uint32_t *lout, int h, int w, uint32_t level, uint32_t *counter, bool padded) {
  if (h == 0 || w == 0) return hipSuccess;
  if (!padded && (w & 3) == 0 && ((reinterpret_cast<uintptr_t>(img) | img_stride) & 3u) == 0) {
    for (long long y0 = 0; y0 < h; y0 += GRID_Y_MAX) {
      dim3 grid((w / 4 + 255) / 256, (unsigned)std::min<long long>(h - y0, GRID_Y_MAX));
      k_flood_step4<<<grid, 256, 0, s>>>(img, img_stride, lin, lout, h, w, level, counter, (int)y0);
    }
  } else {
    for (long long y0 = 0; y0 < h; y0 += 4 * GRID_Y_MAX) {
      dim3 grid((w + 63) / 64, (unsigned)((std::min<long long>(h - y0, 4 * GRID_Y_MAX) + 3) / 4));
      k_flood_step<<<grid, 256, 0, s>>>(img, img_stride, lin, lout, h, w, level, counter, padded ? 1 : 0, (int)y0);
    }
  }
  return hipGetLastError();
}

// ---------------------------------------------------------- find_local_minima --------
//
// lib.rs:1178-1197: interior pixels whose 8 neighbours are all strictly smaller, emitted in row-major order.
// Two launches: the COUNT pass looks at the image once and leaves the 4-bit answer of every 4-pixel group in a nibble plane
// and every row's place in the list (row counts, scanned by its last workgroup); the WRITE pass turns nibbles into list
// entries -- and, when asked, into the seed side tables of that list (k_seed_tables' layout) -- without reading the image again.
//
// The count pass is vector-issue work (8192^2 random bytes: 73 us when every pixel took the max of its eight neighbours
// byte by byte, ~37 instructions a pixel), so it computes in packed 16-bit pairs and reuses row maxima:
//     h3[y][x] = max(r[y][x-1], r[y][x], r[y][x+1])      m2[y][x] = max(r[y][x-1], r[y][x+1])
//     strict maximum at (y, x)  <=>  r[y][x] > max(h3[y-1][x], h3[y+1][x], m2[y][x])
// a thread owns 4 columns of MIN_RS rows: per row 3 loads, 5 byte permutes, 6 packed maxima for h3 / m2 and 11 more
// operations for the four answers -- ~6 a pixel.  Rows and columns outside the image are CLAMPED to the nearest one inside:
// a pixel on the image border then meets its own value among its "neighbours" and can never be a strict maximum, which is
// the reference's "interior only" (3 x 3 windows, lib.rs:1183) without a single mask.

constexpr int SEG = 1024;            // pixels per workgroup step: 256 threads x 4
constexpr int MIN_RS = 8;            // rows per workgroup of the count pass
static_assert(MIN_RS == 8, "k_minima_count's strip sum and k_minima_write's offsets assume strips of eight rows");

size_t minima_segments(int h, int w) { return (size_t)h + (h + MIN_RS - 1) / MIN_RS + 1; }     // one count per row, one per strip of MIN_RS rows
size_t minima_mask_bytes(int h, int w) { return (size_t)h * ((w + SEG - 1) / SEG) * 256; }    // one nibble byte per 4-pixel group

typedef unsigned short u16x2_m __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2_m, a), __builtin_bit_cast(u16x2_m, b)));
}
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2_m, a), __builtin_bit_cast(u16x2_m, b)));
}
__device__ __forceinline__ uint32_t pk_sub_sat(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2_m, a), __builtin_bit_cast(u16x2_m, b)));
}

// One row's contribution for the columns x0 .. x0+3: h3 and m2 of the pairs (x0, x0+1) and (x0+2, x0+3), and the pixels
// themselves, every value in a 16-bit half.
struct MinRow { uint32_t h01, h23, m01, m23, c01, c23; };

// ALIGNED (kernel uniform: dword-aligned rows, W % 4 == 0): three dword loads at clamped offsets, unconditional -- a branch
// per row between them made every row's loads wait for the row before (ten dependent round trips per thread: 50 us of
// the kernel's 53) -- and the three groups that need other bytes (the row's first, its last, any beyond its end) patch
// them in afterwards.
struct MinRaw { uint32_t L, M, R; };      // the dwords left of, at and right of x0: bytes b0 = L[3], b1..b4 = M, b5 = R[0]

template <bool ALIGNED>
__device__ __forceinline__ MinRaw minima_load(const uint8_t *row, int W, int x0) {
  MinRaw v;
  if (ALIGNED) {
    const uint32_t last = (uint32_t)(W - 4), o = min((uint32_t)x0, last);
    v.L = *reinterpret_cast<const uint32_t *>(row + (o >= 4u ? o - 4u : 0u));
    v.M = *reinterpret_cast<const uint32_t *>(row + o);
    v.R = *reinterpret_cast<const uint32_t *>(row + min(o + 4u, last));
  } else {
    auto at = [&](int x) { return (uint32_t)row[min(max(x, 0), W - 1)]; };
    v.L = at(x0 - 1) << 24;
    v.M = at(x0) | (at(x0 + 1) << 8) | (at(x0 + 2) << 16) | (at(x0 + 3) << 24);
    v.R = at(x0 + 4);
  }
  return v;
}

template <bool ALIGNED>
__device__ __forceinline__ MinRow minima_row(MinRaw v, int W, int x0) {
  uint32_t L = v.L, M = v.M, R = v.R;
  if (ALIGNED) {
    if (x0 == 0) L = M << 24;                                // the pixel left of the row's first: itself
    if ((uint32_t)x0 >= (uint32_t)(W - 4)) R = M >> 24;      // ... right of its last: itself
    if (x0 >= W) { L = 0u; M = 0u; R = 0u; }                 // a group beyond the row: all equal, no maximum
  }
  // pairs of neighbouring bytes, one per 16-bit half (v_perm_b32: selector 0-3 = bytes of the second operand, 4-7 = of the first, 0x0c = zero)
  const uint32_t A = __builtin_amdgcn_perm(L, M, 0x0C000C07u);      // (b0, b1)
  const uint32_t B = __builtin_amdgcn_perm(M, M, 0x0C010C00u);      // (b1, b2): the pixels x0, x0+1
  const uint32_t C = __builtin_amdgcn_perm(M, M, 0x0C020C01u);      // (b2, b3)
  const uint32_t D = __builtin_amdgcn_perm(M, M, 0x0C030C02u);      // (b3, b4): the pixels x0+2, x0+3
  const uint32_t E = __builtin_amdgcn_perm(R, M, 0x0C040C03u);      // (b4, b5)
  MinRow r;
  r.m01 = pk_max(A, C);
  r.m23 = pk_max(C, E);
  r.h01 = pk_max(r.m01, B);
  r.h23 = pk_max(r.m23, D);
  r.c01 = B;
  r.c23 = D;
  return r;
}

// bit k: pixel x0 + k of row `mid` is a strict maximum of its 3 x 3 window
__device__ __forceinline__ uint32_t minima_nibble(const MinRow &above, const MinRow &mid, const MinRow &below) {
  const uint32_t n01 = pk_max(pk_max(above.h01, below.h01), mid.m01), n23 = pk_max(pk_max(above.h23, below.h23), mid.m23);
  const uint32_t g01 = pk_min(pk_sub_sat(mid.c01, n01), 0x00010001u), g23 = pk_min(pk_sub_sat(mid.c23, n23), 0x00010001u);      // 1 where centre > neighbours
  const uint32_t t = g01 | (g23 << 2);      // bits 0, 16, 2, 18
  return (t | (t >> 15)) & 0xFu;
}

// A workgroup: MIN_RS rows of one 1024-pixel segment (a row strip per workgroup, all segments in turn: 16 waves per CU in
// flight and 73 -> 53 us; this way 8192 workgroups at 8192^2).  Row counts are added up in counts[y], strip counts in
// counts[H + strip]: eight atomics per address.
template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_minima_count(const uint8_t *__restrict__ img, size_t stride, int H, int W,
                                                      uint32_t *__restrict__ counts, uint8_t *__restrict__ nibbles) {
  __shared__ uint32_t s_wave[4 * MIN_RS];
  const int segs = (W + SEG - 1) / SEG;
  const int seg = blockIdx.x % segs, y0 = (blockIdx.x / segs) * MIN_RS;
  auto row_ptr = [&](int y) { return img + (size_t)min(max(y, 0), H - 1) * stride; };      // (workgroup uniform)
  const int x0 = seg * SEG + threadIdx.x * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // every load of the strip first (thirty dwords in flight per thread), then the arithmetic, then the stores
  MinRaw raw[MIN_RS + 2];
#pragma unroll
  for (int r = 0; r < MIN_RS + 2; ++r) raw[r] = minima_load<ALIGNED>(row_ptr(y0 + r - 1), W, x0);
  MinRow above = minima_row<ALIGNED>(raw[0], W, x0), mid = minima_row<ALIGNED>(raw[1], W, x0);
  uint32_t mine = 0;      // lane r ends up with the wave's count of row y0 + r
  uint32_t nib[MIN_RS];
#pragma unroll
  for (int r = 0; r < MIN_RS; ++r) {
    const MinRow below = minima_row<ALIGNED>(raw[r + 2], W, x0);
    const uint32_t m = minima_nibble(above, mid, below);
    nib[r] = m;
    const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 1u) != 0u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 2u) != 0u)) +
                       (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 4u) != 0u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 8u) != 0u));      // (scalar: the wave's count)
    if (lane == r) mine = c;
    above = mid;
    mid = below;
  }
#pragma unroll
  for (int r = 0; r < MIN_RS; ++r)      // (a group beyond the row's end: 0)
    if (y0 + r < H) nibbles[((size_t)(y0 + r) * segs + seg) * 256 + threadIdx.x] = (uint8_t)nib[r];
  if (lane < MIN_RS) s_wave[wave * MIN_RS + lane] = mine;
  __syncthreads();
  if (threadIdx.x < MIN_RS) {
    const uint32_t c = y0 + (int)threadIdx.x < H ? s_wave[threadIdx.x] + s_wave[MIN_RS + threadIdx.x] + s_wave[2 * MIN_RS + threadIdx.x] + s_wave[3 * MIN_RS + threadIdx.x] : 0u;
    if (c) atomicAdd(&counts[y0 + threadIdx.x], c);
    uint32_t strip = c;      // (MIN_RS == 8 lanes: three steps)
#pragma unroll
    for (int off = MIN_RS / 2; off > 0; off >>= 1) strip += __shfl_down(strip, off, 64);
    if (threadIdx.x == 0 && strip) atomicAdd(&counts[H + y0 / MIN_RS], strip);
  }
}

// counts: minima_segments(h, w) words, zeroed here: [y] row y's count, [h + k] the count of rows 8k .. 8k+7 (minima_write
// turns them into list positions itself: a scan launch of their own cost 8 us, a "last workgroup scans" counter that all
// 8192 workgroups add to 330 -- atomics to ONE address run at ~25 M/s on this chip)
hipError_t minima_count(hipStream_t s, const uint8_t *img, size_t stride, int h, int w, uint32_t *counts, uint8_t *nibbles) {
  if (h == 0 || w == 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(counts, 0, minima_segments(h, w) * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const int segs = (w + SEG - 1) / SEG;
  const unsigned grid = (unsigned)(((h + MIN_RS - 1) / MIN_RS) * segs);
  if (((reinterpret_cast<uintptr_t>(img) | stride) & 3u) == 0 && (w & 3) == 0 && w >= 4)
    k_minima_count<true><<<grid, 256, 0, s>>>(img, stride, h, w, counts, nibbles);
  else
    k_minima_count<false><<<grid, 256, 0, s>>>(img, stride, h, w, counts, nibbles);
  return hipGetLastError();
}

// The write pass: one WAVE per row, no barrier.  A lane takes the nibbles of 32 consecutive pixels (8 bytes) per step, 64 such
// groups a step; a wave scan of their counts gives every group its place in the list.
// mask / word_base (optional, W % 32 == 0): the seed side tables of this very list (k_seed_tables builds them from a list
// it has to search and check; here they fall out of the compaction: a group IS a mask word, its place in the list the
// word's base).  With them the kernel also zeroes the two small arrays that k_seed_tables zeroes for the transform.
// out_rc may then be null: a transform seeded by the image's own minima needs no list.
template <bool LIST>
__global__ __launch_bounds__(256) void k_minima_write(const uint8_t *__restrict__ nibbles, int H, int W,
                                                      const uint32_t *__restrict__ counts, uint32_t *out_rc, size_t cap,
                                                      uint32_t *mask, uint32_t *word_base,
                                                      uint32_t *zero_a, size_t n_zero_a, uint32_t *zero_b, size_t n_zero_b, uint32_t *total) {
  __shared__ uint32_t s_part[4];
  __shared__ uint2 s_stage[LIST ? 4 : 1][LIST ? 1024 : 1];      // (32 KiB: a step's list entries per wave; none for the tables alone)
  {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
    for (size_t i = tid; i < n_zero_a; i += step) zero_a[i] = 0u;
    for (size_t i = tid; i < n_zero_b; i += step) zero_b[i] = 0u;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, y0 = blockIdx.x * 4, y = y0 + wave;
  // Where the workgroup's first row starts in the list: the strips before its own (counts[H + k]: at most H / 8 words,
  // L2-resident, summed by all 256 threads), then the rows of its own strip before it.
  const int strip0 = y0 / MIN_RS;
  uint32_t part = 0;
  for (int k = (int)threadIdx.x; k < strip0; k += 256) part += counts[H + k];
  if ((int)threadIdx.x < y0 - strip0 * MIN_RS) part += counts[strip0 * MIN_RS + threadIdx.x];
  for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off, 64);
  if (lane == 0) s_part[wave] = part;
  __syncthreads();
  if (y >= H) return;
  size_t pos = (size_t)s_part[0] + s_part[1] + s_part[2] + s_part[3];
  for (int k = 0; k < wave; ++k) pos += counts[y0 + k];
  if (y == H - 1 && lane == 0) *total = (uint32_t)pos + counts[y];
  const int segs = (W + SEG - 1) / SEG, groups = segs * 32;      // 8-byte groups of the row's nibble bytes
  const uint2 *nb = reinterpret_cast<const uint2 *>(nibbles + (size_t)y * segs * 256);
  for (int g0 = 0; g0 < groups; g0 += 64) {
    const int g = g0 + lane;
    const uint2 eight = g < groups ? nb[g] : make_uint2(0u, 0u);
    // eight low nibbles -> one word: bit 4k + j = pixel 32 g + 4k + j
    uint32_t lo = eight.x & 0x0F0F0F0Fu, hi = eight.y & 0x0F0F0F0Fu;
    lo = (lo | (lo >> 4)) & 0x00FF00FFu; hi = (hi | (hi >> 4)) & 0x00FF00FFu;
    lo = (lo | (lo >> 8)) & 0xFFFFu; hi = (hi | (hi >> 8)) & 0xFFFFu;
    uint32_t word = lo | (hi << 16);
    const uint32_t c = __popc(word);
    const uint32_t incl = wave_inclusive_sum(c);
    size_t at = pos + incl - c;
    if (mask && g < groups && g * 32 < W) {      // (W % 32 == 0: the word lies in this row, and in the plane)
      const size_t wi = ((size_t)y * W >> 5) + g;
      mask[wi] = word;
      word_base[wi] = (uint32_t)at;
    }
    const uint32_t step_total = (uint32_t)__shfl((int)incl, 63, 64);
    if (LIST) {
      // the step's entries through LDS: a lane's own are three or four, 28 bytes from its neighbour's -- written where they
      // arise, every store instruction touched dozens of lines; staged, the wave writes them 512 contiguous bytes a time
      // (at most one maximum per 2 x 2 block: 16 a lane, 1024 a step)
      uint2 *stage = s_stage[threadIdx.x >> 6];
      uint32_t k = incl - c;
      while (word) {
        const int b = __builtin_ctz(word);
        word &= word - 1u;
        stage[k++] = make_uint2((uint32_t)y, (uint32_t)(g * 32 + b));
      }
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      for (uint32_t i = (uint32_t)lane; i < step_total; i += 64u)
        if (pos + i < cap) *reinterpret_cast<uint2 *>(out_rc + 2 * (pos + i)) = stage[i];
      __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the stage is read before the next step fills it
    }
    pos += step_total;
  }
}

hipError_t minima_write(hipStream_t s, const uint8_t *nibbles, int h, int w, const uint32_t *counts, uint32_t *total, uint32_t *out_rc, size_t cap,
                        uint32_t *mask, uint32_t *word_base, uint32_t *zero_a, size_t n_zero_a, uint32_t *zero_b, size_t n_zero_b) {
  if (h == 0 || w == 0) return hipMemsetAsync(total, 0, sizeof(uint32_t), s);
  if (out_rc) k_minima_write<true><<<(h + 3) / 4, 256, 0, s>>>(nibbles, h, w, counts, out_rc, cap, mask, word_base, zero_a, n_zero_a, zero_b, n_zero_b, total);
  else k_minima_write<false><<<(h + 3) / 4, 256, 0, s>>>(nibbles, h, w, counts, out_rc, cap, mask, word_base, zero_a, n_zero_a, zero_b, n_zero_b, total);
  return hipGetLastError();
}

// ---- find_local_minima of every slice of a cube (ws_find_local_minima_batch_device) -------------------------------------------------
//
// The same two passes over the STACK of n_slices * h rows, as new kernels: the single plane's above stay as they are.  A slice's rows
// 0 and h - 1 are never maxima (the single plane's row clamp makes them meet their own values): here their nibbles are cleared, for the
// row above local row 0 is another slice's.  Every other row's neighbours are rows of its own slice, so its answer is the single
// plane's.  Strips of MIN_RS rows may straddle slices: positions are global.  The write pass takes a strip's start from the SCANNED
// strip counts (k_minima_strip_scan) -- the single plane's sums every earlier strip in every workgroup, quadratic in the rows -- maps
// its row to (slice, local row), writes local coordinates, and the wave that owns local row 0 of slice k stores offsets[k].

template <bool ALIGNED>
__global__ __launch_bounds__(256) void k_minima_count_stack(const uint8_t *__restrict__ img, size_t stride, size_t slice_stride, int H, int R, int W,
                                                            uint32_t *__restrict__ counts, uint8_t *__restrict__ nibbles) {
  __shared__ uint32_t s_wave[4 * MIN_RS];
  const int segs = (W + SEG - 1) / SEG;
  const int seg = blockIdx.x % segs, y0 = (blockIdx.x / segs) * MIN_RS;
  auto row_ptr = [&](int y) {      // (workgroup uniform) stacked row y, clamped into the stack
    y = min(max(y, 0), R - 1);
    const int k = y / H;
    return img + (size_t)k * slice_stride + (size_t)(y - k * H) * stride;
  };
  const int x0 = seg * SEG + threadIdx.x * 4;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  MinRaw raw[MIN_RS + 2];
#pragma unroll
  for (int r = 0; r < MIN_RS + 2; ++r) raw[r] = minima_load<ALIGNED>(row_ptr(y0 + r - 1), W, x0);
  MinRow above = minima_row<ALIGNED>(raw[0], W, x0), mid = minima_row<ALIGNED>(raw[1], W, x0);
  uint32_t mine = 0;      // lane r ends up with the wave's count of row y0 + r
  uint32_t nib[MIN_RS];
  int ly = y0 % H;        // local row of y0 + r
#pragma unroll
  for (int r = 0; r < MIN_RS; ++r) {
    const MinRow below = minima_row<ALIGNED>(raw[r + 2], W, x0);
    const uint32_t m = (ly == 0 || ly == H - 1) ? 0u : minima_nibble(above, mid, below);      // a slice's border rows: interior never
    nib[r] = m;
    const uint32_t c = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 1u) != 0u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 2u) != 0u)) +
                       (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 4u) != 0u)) + (uint32_t)__popcll(__builtin_amdgcn_ballot_w64((m & 8u) != 0u));
    if (lane == r) mine = c;
    above = mid;
    mid = below;
    ly = ly + 1 == H ? 0 : ly + 1;
  }
#pragma unroll
  for (int r = 0; r < MIN_RS; ++r)
    if (y0 + r < R) nibbles[((size_t)(y0 + r) * segs + seg) * 256 + threadIdx.x] = (uint8_t)nib[r];
  if (lane < MIN_RS) s_wave[wave * MIN_RS + lane] = mine;
  __syncthreads();
  if (threadIdx.x < MIN_RS) {
    const uint32_t c = y0 + (int)threadIdx.x < R ? s_wave[threadIdx.x] + s_wave[MIN_RS + threadIdx.x] + s_wave[2 * MIN_RS + threadIdx.x] + s_wave[3 * MIN_RS + threadIdx.x] : 0u;
    if (c) atomicAdd(&counts[y0 + threadIdx.x], c);
    uint32_t strip = c;
#pragma unroll
    for (int off = MIN_RS / 2; off > 0; off >>= 1) strip += __shfl_down(strip, off, 64);
    if (threadIdx.x == 0 && strip) atomicAdd(&counts[R + y0 / MIN_RS], strip);
  }
}

// starts[k] = the strip counts before strip k, starts[strips] = their total: one workgroup, 16 K strips a round
__global__ __launch_bounds__(1024) void k_minima_strip_scan(const uint32_t *__restrict__ strip_counts, int strips, uint32_t *__restrict__ starts) {
  constexpr int PER = 16;
  __shared__ uint32_t s_wave[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t carry = 0;
  for (int base = 0; base < strips; base += 1024 * PER) {
    const int i0 = base + (int)threadIdx.x * PER;
    uint32_t v[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { v[j] = i0 + j < strips ? strip_counts[i0 + j] : 0u; sum += v[j]; }
    const uint32_t incl = wave_inclusive_sum(sum);
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t run = carry + incl - sum, all = 0;
    for (int k = 0; k < 16; ++k) { if (k < wave) run += s_wave[k]; all += s_wave[k]; }
#pragma unroll
    for (int j = 0; j < PER; ++j) { if (i0 + j < strips) starts[i0 + j] = run; run += v[j]; }
    carry += all;
    __syncthreads();      // s_wave is the next round's
  }
  if (threadIdx.x == 0) starts[strips] = carry;
}

// one WAVE per stacked row, no barrier (k_minima_write's compaction, the list alone)
__global__ __launch_bounds__(256) void k_minima_write_stack(const uint8_t *__restrict__ nibbles, int H, int R, int W, const uint32_t *__restrict__ counts,
                                                            const uint32_t *__restrict__ starts, uint32_t *out_rc, size_t cap, uint32_t *__restrict__ offsets) {
  __shared__ uint2 s_stage[4][1024];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, y = blockIdx.x * 4 + wave;
  if (y >= R) return;
  const int strip = y / MIN_RS;
  size_t pos = starts[strip];
  for (int r = strip * MIN_RS; r < y; ++r) pos += counts[r];
  const int k = y / H, ly = y - k * H;
  const uint32_t mine = counts[y];
  if (lane == 0) {
    if (ly == 0) offsets[k] = (uint32_t)pos;
    if (y == R - 1) offsets[k + 1] = (uint32_t)pos + mine;      // the run's total
  }
  if (mine == 0) return;      // (wave uniform; every slice's border rows)
  const int segs = (W + SEG - 1) / SEG, groups = segs * 32;
  const uint2 *nb = reinterpret_cast<const uint2 *>(nibbles + (size_t)y * segs * 256);
  uint2 *stage = s_stage[wave];
  for (int g0 = 0; g0 < groups; g0 += 64) {
    const int g = g0 + lane;
    const uint2 eight = g < groups ? nb[g] : make_uint2(0u, 0u);
    uint32_t lo = eight.x & 0x0F0F0F0Fu, hi = eight.y & 0x0F0F0F0Fu;
    lo = (lo | (lo >> 4)) & 0x00FF00FFu; hi = (hi | (hi >> 4)) & 0x00FF00FFu;
    lo = (lo | (lo >> 8)) & 0xFFFFu; hi = (hi | (hi >> 8)) & 0xFFFFu;
    uint32_t word = lo | (hi << 16);
    const uint32_t c = __popc(word);
    const uint32_t incl = wave_inclusive_sum(c);
    const uint32_t step_total = (uint32_t)__shfl((int)incl, 63, 64);
    uint32_t at = incl - c;
    while (word) {      // (at most one maximum per 2 x 2 block: 16 a lane, 1024 a step)
      const int b = __builtin_ctz(word);
      word &= word - 1u;
      stage[at++] = make_uint2((uint32_t)ly, (uint32_t)(g * 32 + b));
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    for (uint32_t i = (uint32_t)lane; i < step_total; i += 64u)
      if (pos + i < cap) *reinterpret_cast<uint2 *>(out_rc + 2 * (pos + i)) = stage[i];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");      // the stage is read before the next step fills it
    pos += step_total;
  }
}

// words: [0, R) row counts, [R, R + strips) strip counts, then strips + 1 strip starts, then n_slices + 1 offsets
size_t minima_stack_words(size_t rows, size_t n_slices) {
  const size_t strips = (rows + MIN_RS - 1) / MIN_RS;
  return rows + strips + strips + 1 + n_slices + 1;
}

// n_slices slices of h x w (h, w >= 3; n_slices * h < 2^31 - 15) at cube + k * slice_stride: their lists back to back in out_rc (cut at
// cap; nullable with cap 0), *d_offsets (n_slices + 1 words inside `words`): where each slice's list begins, and the total
hipError_t minima_stack(hipStream_t s, const uint8_t *cube, size_t row_stride, size_t slice_stride, size_t n_slices, int h, int w, uint32_t *words,
                        uint8_t *nibbles, uint32_t *out_rc, size_t cap, uint32_t **d_offsets) {
  const int R = (int)(n_slices * (size_t)h), strips = (R + MIN_RS - 1) / MIN_RS, segs = (w + SEG - 1) / SEG;
  uint32_t *starts = words + (size_t)R + strips, *offsets = starts + strips + 1;
  *d_offsets = offsets;
  hipError_t e = hipMemsetAsync(words, 0, ((size_t)R + strips) * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  const unsigned grid = (unsigned)((size_t)strips * segs);
  if (((reinterpret_cast<uintptr_t>(cube) | row_stride | slice_stride) & 3u) == 0 && (w & 3) == 0 && w >= 4)
    k_minima_count_stack<true><<<grid, 256, 0, s>>>(cube, row_stride, slice_stride, h, R, w, words, nibbles);
  else
    k_minima_count_stack<false><<<grid, 256, 0, s>>>(cube, row_stride, slice_stride, h, R, w, words, nibbles);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  k_minima_strip_scan<<<1, 1024, 0, s>>>(words + R, strips, starts);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  k_minima_write_stack<<<(unsigned)((R + 3) / 4), 256, 0, s>>>(nibbles, h, R, w, words, starts, out_rc, out_rc ? cap : 0, offsets);
  return hipGetLastError();
}

}  // namespace wsk
