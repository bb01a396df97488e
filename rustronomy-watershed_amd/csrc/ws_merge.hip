// ws_merge.hip -- gfx950 kernels of the merging transform (see ws_merge.hpp for the maths).
//
// Union-find over seed colours, lock-free, union-by-min-index: a root only ever gets hooked
// under a SMALLER index (atomicCAS on the root's own slot) and path halving only ever
// lowers a parent (atomicMin), so every parent chain is monotone and a stale read is still
// an ancestor.  All parent updates are device-scope atomics: XCD L2s are not coherent with
// each other, and nothing here relies on a plain store being seen inside a launch.
#include "ws_common.hpp"
#include "ws_merge.hpp"

#include <algorithm>

namespace wsk {

// Reads of the forest may be stale: parents only ever decrease along a chain, so an old value is
// still an ancestor and the CAS that hooks a root returns the true state.  That makes an ordinary
// L1-cached load legal here (workgroup scope = a plain global_load the compiler will not hoist);
// the agent-scope form bypasses L1 and made every find() of the one surviving root an L2 round trip.
__device__ __forceinline__ uint32_t ld_parent(const uint32_t *parent, uint32_t x) {
  return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t uf_find(uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t p = ld_parent(parent, x);
    if (p == x) return x;
    const uint32_t g = ld_parent(parent, p);
    if (g == p) return p;
    atomicMin(parent + x, g);          // path halving; parents only decrease
    x = g;
  }
}

// root of x by a plain walk: no halving, no atomics (for a forest nobody is changing during the launch, or a crowd of
// readers of the same few chains, whose halving atomics would queue up on the same words)
__device__ __forceinline__ uint32_t uf_root(const uint32_t *parent, uint32_t x) {
  for (;;) {
    const uint32_t p = ld_parent(parent, x);
    if (p == x) return x;
    x = p;
  }
}

// returns the node that lost its root status (hooked under a smaller root), or 0xFFFFFFFF
__device__ __forceinline__ uint32_t uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return 0xFFFFFFFFu;
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicCAS(parent + b, b, a);     // b is a root only while parent[b] == b
    if (old == b) return b;
    b = old;                                              // someone hooked b first: continue from there
  }
}

__global__ void k_uf_init(uint32_t *parent, uint32_t *size, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) { parent[i] = (uint32_t)i; size[i] = 0u; }
}

hipError_t uf_init(hipStream_t s, uint32_t *parent, uint32_t *size, size_t n) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192);
  k_uf_init<<<blocks, 256, 0, s>>>(parent, size, n);
  return hipGetLastError();
}

// ---- edge / pixel enumeration shared by the histogram, scatter and whole-image union ------

constexpr int MSEG = 1024;   // pixels per workgroup: one row segment, 4 per thread

struct PixelItems {
  // up to 4 pixels of one row segment and their right / down crossings
  uint32_t px_lvl[4], px_col[4];      // level 0xFFFFFFFF = no item
  uint32_t er_lvl[4], ed_lvl[4];
  uint2 er[4], ed[4];
};

__device__ __forceinline__ bool interior(int y, int x, int H, int W) {
  return y >= 1 && y < H - 1 && x >= 1 && x < W - 1;
}

// Loads first, unconditional and on clamped addresses (a load under a data-dependent branch is waited for before the next is
// issued: 24 dependent round trips per thread in the first form of this function), predicates afterwards.  With W % 4 == 0 and
// planes on 16-byte alignment the four pixels and the four below them are 16-byte loads.
typedef uint32_t u32x4_m __attribute__((ext_vector_type(4)));

// STACK: H rows of slices of slice_h rows each (ws_transform_to_list_batch_device): "interior" and the pixel below are taken
// within the row's slice -- no pair crosses a slice border -- and colours become colour + base[slice], one numbering for the stack
template <bool STACK = false>
__device__ __forceinline__ void gather_items(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                             int H, int W, int y, int x0, PixelItems &it, int slice_h = 0,
                                             const uint32_t *__restrict__ base = nullptr) {
  uint32_t kp[5], lp[5], kd[4], ld[4];      // the row's pixels x0 .. x0 + 4 and the pixels below x0 .. x0 + 3
  const int yd = min(y + 1, H - 1);
  const int ys = STACK ? y % slice_h : y, hs = STACK ? slice_h : H;      // row and height within the slice
  const uint32_t add = STACK ? base[y / slice_h] : 0u;
  // (a caller's planes -- the arrival forms -- may be views off 16-byte alignment: those take the scalar loads)
  const bool aligned = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  if ((W & 3) == 0 && aligned && x0 + 3 < W) {
    const size_t p = (size_t)y * W + x0, q = (size_t)yd * W + x0;
    const u32x4_m a = *reinterpret_cast<const u32x4_m *>(keys + p), b = *reinterpret_cast<const u32x4_m *>(labels + p);
    const u32x4_m c = *reinterpret_cast<const u32x4_m *>(keys + q), d = *reinterpret_cast<const u32x4_m *>(labels + q);
    const size_t pr = (size_t)y * W + min(x0 + 4, W - 1);
    kp[4] = keys[pr]; lp[4] = labels[pr];
    kp[0] = a.x; kp[1] = a.y; kp[2] = a.z; kp[3] = a.w;
    lp[0] = b.x; lp[1] = b.y; lp[2] = b.z; lp[3] = b.w;
    kd[0] = c.x; kd[1] = c.y; kd[2] = c.z; kd[3] = c.w;
    ld[0] = d.x; ld[1] = d.y; ld[2] = d.z; ld[3] = d.w;
  } else {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const size_t p = (size_t)y * W + min(x0 + k, W - 1);
      kp[k] = keys[p]; lp[k] = labels[p];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const size_t q = (size_t)yd * W + min(x0 + k, W - 1);
      kd[k] = keys[q]; ld[k] = labels[q];
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    it.px_lvl[k] = it.er_lvl[k] = it.ed_lvl[k] = 0xFFFFFFFFu;
    const int x = x0 + k;
    const bool here = x < W && kp[k] != KEY_INF;            // uncoloured pixels carry no lake
    const uint32_t vp = kp[k] >> 24;
    if (here) { it.px_lvl[k] = vp; it.px_col[k] = lp[k] + add; }
    const bool ip = interior(ys, x, hs, W);
    // find_merge only sees pairs around a 3x3 window centre (lib.rs:411-434)
    if (here && x + 1 < W && kp[k + 1] != KEY_INF && lp[k + 1] != lp[k] && (ip || interior(ys, x + 1, hs, W))) {
      it.er_lvl[k] = max(vp, kp[k + 1] >> 24);
      it.er[k] = make_uint2(lp[k] + add, lp[k + 1] + add);
    }
    if (here && ys + 1 < hs && kd[k] != KEY_INF && ld[k] != lp[k] && (ip || interior(ys + 1, x, hs, W))) {
      it.ed_lvl[k] = max(vp, kd[k] >> 24);
      it.ed[k] = make_uint2(lp[k] + add, ld[k] + add);
    }
  }
}

// A workgroup takes SEG_RUN consecutive row segments of a large plane (one per step), not one: the 512 level counters are hit once per
// workgroup and level, and with a workgroup per 1024 pixels those same-address atomics (~12 ns each) WERE the kernel --
// 8192^2: 33 M of them on 512 words, 1.4 ms for 0.5 GB of reads.
constexpr int SEG_RUN_MAX = 16;
static int seg_run_for(size_t total) { return (int)std::min<size_t>(std::max<size_t>(total / 4096, 1), SEG_RUN_MAX); }      // small planes keep a workgroup per segment

template <bool STACK>
__global__ __launch_bounds__(256) void k_level_hist(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                    int H, int W, int segs, int SEG_RUN, u64c *hist_px, u64c *hist_edge,
                                                    int slice_h, const uint32_t *__restrict__ base) {
  __shared__ uint32_t s_px[NLEVELS], s_ed[NLEVELS];
  s_px[threadIdx.x] = 0;
  s_ed[threadIdx.x] = 0;
  __syncthreads();
  const size_t total = (size_t)H * segs;
  for (int j = 0; j < SEG_RUN; ++j) {
    const size_t sg = (size_t)blockIdx.x * SEG_RUN + j;
    if (sg >= total) break;
    const int y = (int)(sg / segs), seg = (int)(sg % segs);
    PixelItems it;
    gather_items<STACK>(keys, labels, H, W, y, seg * MSEG + threadIdx.x * 4, it, slice_h, base);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (it.px_lvl[k] != 0xFFFFFFFFu) atomicAdd(&s_px[it.px_lvl[k]], 1u);
      if (it.er_lvl[k] != 0xFFFFFFFFu) atomicAdd(&s_ed[it.er_lvl[k]], 1u);
      if (it.ed_lvl[k] != 0xFFFFFFFFu) atomicAdd(&s_ed[it.ed_lvl[k]], 1u);
    }
  }
  __syncthreads();
  if (s_px[threadIdx.x]) atomicAdd(&hist_px[threadIdx.x], (u64c)s_px[threadIdx.x]);
  if (s_ed[threadIdx.x]) atomicAdd(&hist_edge[threadIdx.x], (u64c)s_ed[threadIdx.x]);
}

hipError_t level_hist(hipStream_t s, const uint32_t *keys, const uint32_t *labels, int h, int w,
                      u64c *hist_px, u64c *hist_edge, int slice_h, const uint32_t *slice_base) {
  if (h == 0 || w == 0) return hipSuccess;
  const int segs = (w + MSEG - 1) / MSEG;
  const size_t total = (size_t)h * segs;
  const int run = seg_run_for(total);
  const unsigned blocks = (unsigned)((total + run - 1) / run);
  if (slice_base) k_level_hist<true><<<blocks, 256, 0, s>>>(keys, labels, h, w, segs, run, hist_px, hist_edge, slice_h, slice_base);
  else k_level_hist<false><<<blocks, 256, 0, s>>>(keys, labels, h, w, segs, run, hist_px, hist_edge, 0, nullptr);
  return hipGetLastError();
}

// Exclusive prefix sums of the two histograms, on the device: off[l] = first item of level l, off[256] = total; the
// scatter cursors start at the same values.  (The host used to do this between two synchronisations.)
__global__ __launch_bounds__(NLEVELS) void k_level_offsets(const u64c *__restrict__ hist_px, const u64c *__restrict__ hist_ed,
                                                           u64c *off_px, u64c *off_ed, u64c *cur_px, u64c *cur_ed) {
  __shared__ u64c s_a[NLEVELS], s_b[NLEVELS];
  const int t = threadIdx.x;
  const u64c a0 = hist_px[t], b0 = hist_ed[t];
  s_a[t] = a0;
  s_b[t] = b0;
  __syncthreads();
  for (int o = 1; o < NLEVELS; o <<= 1) {            // Hillis-Steele inclusive scan
    const u64c a = t >= o ? s_a[t - o] : 0ull, b = t >= o ? s_b[t - o] : 0ull;
    __syncthreads();
    s_a[t] += a;
    s_b[t] += b;
    __syncthreads();
  }
  off_px[t] = cur_px[t] = s_a[t] - a0;
  off_ed[t] = cur_ed[t] = s_b[t] - b0;
  if (t == NLEVELS - 1) { off_px[NLEVELS] = s_a[t]; off_ed[NLEVELS] = s_b[t]; }
}

hipError_t level_offsets(hipStream_t s, const u64c *hist_px, const u64c *hist_ed, u64c *off_px, u64c *off_ed, u64c *cur_px, u64c *cur_ed) {
  k_level_offsets<<<1, NLEVELS, 0, s>>>(hist_px, hist_ed, off_px, off_ed, cur_px, cur_ed);
  return hipGetLastError();
}

// Two walks over the workgroup's SEG_RUN segments: the first counts its items per level in LDS, then ONE reservation per
// (workgroup, level), then the second walk gathers the items again (L2 still holds them) and writes them behind LDS cursors.
template <bool STACK>
__global__ __launch_bounds__(256) void k_level_scatter(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                       int H, int W, int segs, int SEG_RUN, u64c *cursor_px, u64c *cursor_edge,
                                                       uint32_t *px_items, uint2 *edge_items, int slice_h, const uint32_t *__restrict__ base) {
  __shared__ uint32_t s_px[NLEVELS], s_ed[NLEVELS];
  __shared__ u64c s_bpx[NLEVELS], s_bed[NLEVELS];
  s_px[threadIdx.x] = 0;
  s_ed[threadIdx.x] = 0;
  __syncthreads();
  const size_t total = (size_t)H * segs;
  for (int j = 0; j < SEG_RUN; ++j) {
    const size_t sg = (size_t)blockIdx.x * SEG_RUN + j;
    if (sg >= total) break;
    PixelItems it;
    gather_items<STACK>(keys, labels, H, W, (int)(sg / segs), (int)(sg % segs) * MSEG + threadIdx.x * 4, it, slice_h, base);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (it.px_lvl[k] != 0xFFFFFFFFu) atomicAdd(&s_px[it.px_lvl[k]], 1u);
      if (it.er_lvl[k] != 0xFFFFFFFFu) atomicAdd(&s_ed[it.er_lvl[k]], 1u);
      if (it.ed_lvl[k] != 0xFFFFFFFFu) atomicAdd(&s_ed[it.ed_lvl[k]], 1u);
    }
  }
  __syncthreads();
  // one global reservation per (workgroup, level) that has items
  {
    const uint32_t cp = s_px[threadIdx.x], ce = s_ed[threadIdx.x];
    s_bpx[threadIdx.x] = cp ? atomicAdd(&cursor_px[threadIdx.x], (u64c)cp) : 0ull;
    s_bed[threadIdx.x] = ce ? atomicAdd(&cursor_edge[threadIdx.x], (u64c)ce) : 0ull;
  }
  __syncthreads();
  s_px[threadIdx.x] = 0;
  s_ed[threadIdx.x] = 0;
  __syncthreads();
  for (int j = 0; j < SEG_RUN; ++j) {
    const size_t sg = (size_t)blockIdx.x * SEG_RUN + j;
    if (sg >= total) break;
    PixelItems it;
    gather_items<STACK>(keys, labels, H, W, (int)(sg / segs), (int)(sg % segs) * MSEG + threadIdx.x * 4, it, slice_h, base);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (it.px_lvl[k] != 0xFFFFFFFFu) {
        const uint32_t l = it.px_lvl[k];
        px_items[s_bpx[l] + atomicAdd(&s_px[l], 1u)] = it.px_col[k];
      }
      if (it.er_lvl[k] != 0xFFFFFFFFu) {
        const uint32_t l = it.er_lvl[k];
        edge_items[s_bed[l] + atomicAdd(&s_ed[l], 1u)] = it.er[k];
      }
      if (it.ed_lvl[k] != 0xFFFFFFFFu) {
        const uint32_t l = it.ed_lvl[k];
        edge_items[s_bed[l] + atomicAdd(&s_ed[l], 1u)] = it.ed[k];
      }
    }
  }
}

hipError_t level_scatter(hipStream_t s, const uint32_t *keys, const uint32_t *labels, int h, int w,
                         u64c *cursor_px, u64c *cursor_edge, uint32_t *px_items, uint2 *edge_items, int slice_h, const uint32_t *slice_base) {
  if (h == 0 || w == 0) return hipSuccess;
  const int segs = (w + MSEG - 1) / MSEG;
  const size_t total = (size_t)h * segs;
  const int run = seg_run_for(total);
  const unsigned blocks = (unsigned)((total + run - 1) / run);
  if (slice_base)
    k_level_scatter<true><<<blocks, 256, 0, s>>>(keys, labels, h, w, segs, run, cursor_px, cursor_edge, px_items, edge_items, slice_h, slice_base);
  else
    k_level_scatter<false><<<blocks, 256, 0, s>>>(keys, labels, h, w, segs, run, cursor_px, cursor_edge, px_items, edge_items, 0, nullptr);
  return hipGetLastError();
}

// ---- per-level union / sizes / emit -----------------------------------------------------

// range (nullable): {first, end} item indices in device memory -- the level's bucket, whose bounds the host never reads
// death (nullable): death[c] = the level at which colour c stopped being a root (0xFFFFFFFF: still one)
__device__ __forceinline__ void union_body(const uint2 *__restrict__ edges, size_t n, uint32_t *parent, uint32_t *hooked,
                                           uint32_t *hooked_count, const u64c *__restrict__ range, uint32_t *death, uint32_t level,
                                           unsigned nblocks) {
  if (range) { edges += range[0]; n = (size_t)(range[1] - range[0]); }
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)nblocks * blockDim.x;
  for (; i < n; i += step) {
    const uint2 e = edges[i];
    const uint32_t lost = uf_union(parent, e.x, e.y);
    if (lost != 0xFFFFFFFFu) {
      if (hooked) hooked[atomicAdd(hooked_count, 1u)] = lost;
      if (death) death[lost] = level;
    }
  }
}

__global__ void k_union_edges(const uint2 *__restrict__ edges, size_t n, uint32_t *parent, uint32_t *hooked,
                              uint32_t *hooked_count, const u64c *__restrict__ range) {
  union_body(edges, n, parent, hooked, hooked_count, range, nullptr, 0u, gridDim.x);
}

hipError_t union_edges(hipStream_t s, const uint2 *edges, size_t n, uint32_t *parent, uint32_t *hooked,
                       uint32_t *hooked_count) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  k_union_edges<<<blocks, 256, 0, s>>>(edges, n, parent, hooked, hooked_count, nullptr);
  return hipGetLastError();
}

hipError_t union_edges_ranged(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned grid, uint32_t *parent, uint32_t *hooked,
                              uint32_t *hooked_count) {
  k_union_edges<<<grid, 256, 0, s>>>(edge_items, 0, parent, hooked, hooked_count, range);
  return hipGetLastError();
}

// After a level's unions every node hooked in this level hands its accumulated area to its final root, and the areas
// of the pixels arriving at this level go to the lake they arrive in.  Late levels have few lakes, so most lanes of a
// wave add to the SAME word: the wave adds once per distinct root (leader election by ballot) -- same-address atomics
// retire one per ~12 ns, and 4000 of them were the whole kernel.
// Both in one launch (a level of transform_to_list was four dependent launches of a few microseconds each:
// launch gaps are most of its time).  They do not interfere: folding reads the areas of nodes hooked in this level --
// no longer roots, so no arrival is added to them -- and both add to roots.
__global__ void k_fold_and_add(const uint32_t *__restrict__ hooked, const uint32_t *__restrict__ hooked_count,
                               const uint32_t *__restrict__ px_items, size_t n, uint32_t *parent, uint32_t *size,
                               const u64c *__restrict__ range, int split) {
  if (range) { px_items += range[0]; n = (size_t)(range[1] - range[0]); }
  const int lane = threadIdx.x & 63;
  // the upper half of the grid folds, the lower half counts arrivals (`split`): two chains of dependent L2 round trips
  // side by side instead of one after the other
  const unsigned half = split ? gridDim.x / 2 : gridDim.x;
  const bool folds = !split || blockIdx.x >= half, counts = !split || blockIdx.x < half;
  const unsigned bid = split && blockIdx.x >= half ? blockIdx.x - half : blockIdx.x;
  const size_t step = (size_t)half * blockDim.x;
  if (hooked && folds) {
    const uint32_t nh = *hooked_count;
    for (size_t i = (size_t)bid * blockDim.x + threadIdx.x; i < nh; i += step) {
      const uint32_t b = hooked[i];
      const uint32_t area = size[b];
      if (area) atomicAdd(&size[uf_find(parent, b)], area);
    }
  }
  if (!counts) return;
  for (size_t base = (size_t)bid * blockDim.x; base < n; base += step) {      // uniform trip count per wave
    const size_t i = base + threadIdx.x;
    const bool active = i < n;
    const uint32_t r = active ? uf_find(parent, px_items[i]) : 0xFFFFFFFFu;
    unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
    // a few rounds of leader election catch the case that matters (late levels: a handful of lakes, thousands of lanes on
    // the same word); what is left after them -- early levels: every lane another lake -- adds for itself
    for (int round = 0; round < 4 && todo != 0; ++round) {
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);      // (v_readlane: no LDS round trip; leader is wave uniform)
      const unsigned long long same = __builtin_amdgcn_ballot_w64(active && r == r0);
      if (lane == leader) atomicAdd(&size[r0], (uint32_t)__popcll(same));
      todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&size[r], 1u);
  }
}

hipError_t fold_and_add(hipStream_t s, const uint32_t *hooked, const uint32_t *hooked_count, const uint32_t *px_items, size_t n,
                        uint32_t *parent, uint32_t *size) {
  if (!hooked && n == 0) return hipSuccess;
  const size_t want = std::max<size_t>((n + 255) / 256, hooked ? 512 : 1);
  k_fold_and_add<<<(unsigned)std::min<size_t>(want, 4096), 256, 0, s>>>(hooked, hooked_count, px_items, n, parent, size, nullptr, 0);
  return hipGetLastError();
}

hipError_t fold_and_add_ranged(hipStream_t s, const uint32_t *hooked, const uint32_t *hooked_count, const uint32_t *px_items,
                               const u64c *range, unsigned grid, uint32_t *parent, uint32_t *size) {
  k_fold_and_add<<<hooked ? 2 * grid : grid, 256, 0, s>>>(hooked, hooked_count, px_items, 0, parent, size, range, hooked ? 1 : 0);
  return hipGetLastError();
}

// lib.rs:628-635 sparsely: one (colour, area) record per lake with area > 0.  Records of one level are contiguous:
// a record's position is the number of records of the earlier levels -- every workgroup adds up their counters, which
// earlier launches finished -- plus a ticket from this level's own counter, one request per WAVE (its lakes take
// consecutive records).  No cursor is handed from level to level inside the kernel: the "last workgroup publishes the
// total" protocol that did that needs __threadfence(), which on this part writes the XCD's L2 back -- 24 us per level
// for a kernel with 5 us of work, 6 of the 11 ms of a 1024^2 transform_to_list.
constexpr int EMIT_PER_THREAD = 4;      // colours per thread: a workgroup of 256 looks at 1024 colours and asks for ONE ticket range
// death (nullable): a colour is a lake of `level` while death[c] > level -- the test that stays true while the NEXT level's
// unions are already hooking roots (k_union_emit); without it: parent[c] == c.
__device__ __forceinline__ void emit_body(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ size, size_t n_colours,
                                          uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t level,
                                          const uint32_t *__restrict__ death, unsigned bid) {
  __shared__ u64c s_base;
  __shared__ uint32_t s_wave[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 64) {
    u64c before = 0;
    for (uint32_t j = (uint32_t)lane; j < level; j += 64) before += level_counts[j];
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) s_base = before;
  }
  // same-address atomics retire one per ~10 ns: a ticket request per wave (1.8 k per level at 1024^2) was 17 us of this
  // kernel; per workgroup of 1024 colours it is ~1 us
  const size_t i0 = (size_t)bid * (256 * EMIT_PER_THREAD) + 1;      // colour 0 = uncoloured
  uint32_t area[EMIT_PER_THREAD];
  bool lake[EMIT_PER_THREAD];
  unsigned long long m[EMIT_PER_THREAD];
  uint32_t mine = 0;
#pragma unroll
  for (int k = 0; k < EMIT_PER_THREAD; ++k) {
    const size_t i = i0 + (size_t)k * 256 + threadIdx.x;
    area[k] = i < n_colours ? size[i] : 0u;
    lake[k] = i < n_colours && area[k] != 0u && (death ? death[i] > level : parent[i] == (uint32_t)i);
    m[k] = __builtin_amdgcn_ballot_w64(lake[k]);
    mine += (uint32_t)__popcll(m[k]);
  }
  if (lane == 0) s_wave[wave] = mine;
  __syncthreads();
  const uint32_t w0 = s_wave[0], w1 = s_wave[1], w2 = s_wave[2], w3 = s_wave[3];
  const uint32_t block_total = w0 + w1 + w2 + w3;
  if (block_total == 0) return;            // workgroup uniform
  __shared__ u64c s_first;
  if (threadIdx.x == 0) s_first = atomicAdd(level_counts + level, (u64c)block_total);
  __syncthreads();
  u64c pos = s_base + s_first + (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u);
#pragma unroll
  for (int k = 0; k < EMIT_PER_THREAD; ++k) {
    const u64c p = pos + (u64c)__popcll(m[k] & ((1ull << lane) - 1ull));
    if (lake[k] && p < cap) {
      const size_t i = i0 + (size_t)k * 256 + threadIdx.x;
      lakes[2 * p] = (uint64_t)i;
      lakes[2 * p + 1] = (uint64_t)area[k];
    }
    pos += (u64c)__popcll(m[k]);
  }
}

__global__ __launch_bounds__(256) void k_emit_lakes(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ size, size_t n_colours,
                                                    uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t level,
                                                    const uint32_t *__restrict__ death) {
  emit_body(parent, size, n_colours, lakes, cap, level_counts, level, death, blockIdx.x);
}

// The unions of level `level` and the lake records of level `level - 1` in ONE launch (merging transform_to_list: two
// launches per level instead of three).  They do not interfere: the records read the areas (`size`: only the fold
// kernels write it) and decide "was a lake at level - 1" by death[c] > level - 1, which a union of THIS level -- it sets
// death[c] = level -- leaves true; the unions touch parent / hooked / death only.
__global__ __launch_bounds__(256) void k_union_emit(const uint2 *__restrict__ edge_items, const u64c *__restrict__ range, unsigned union_blocks,
                                                    uint32_t *parent, uint32_t *hooked, uint32_t *hooked_count, uint32_t *death, uint32_t level,
                                                    const uint32_t *__restrict__ size, size_t n_colours, unsigned emit_blocks,
                                                    uint64_t *lakes, size_t cap, u64c *level_counts) {
  // different workgroups for the two jobs: both are chains of dependent L2 round trips (find, find, CAS / load, ticket,
  // store), and one workgroup doing one after the other took the sum of the two latencies (8.8 us per launch)
  if (blockIdx.x < union_blocks) union_body(edge_items, 0, parent, hooked, hooked_count, range, death, level, union_blocks);
  else if (level > 0 && blockIdx.x - union_blocks < emit_blocks)
    emit_body(parent, size, n_colours, lakes, cap, level_counts, level - 1, death, blockIdx.x - union_blocks);
}

static size_t emit_blocks_for(size_t n_colours) {
  const size_t per_block = 256 * EMIT_PER_THREAD;
  return n_colours <= 1 ? 1 : (n_colours - 1 + per_block - 1) / per_block;
}

hipError_t union_emit(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned union_grid, uint32_t *parent, uint32_t *hooked,
                      uint32_t *hooked_count, uint32_t *death, uint32_t level, const uint32_t *size, size_t n_colours, uint64_t *lakes,
                      size_t cap, u64c *level_counts) {
  const unsigned eb = (unsigned)emit_blocks_for(n_colours);
  k_union_emit<<<union_grid + (level > 0 ? eb : 0u), 256, 0, s>>>(edge_items, range, union_grid, parent, hooked, hooked_count, death, level,
                                                                        size, n_colours, eb, lakes, cap, level_counts);
  return hipGetLastError();
}

hipError_t emit_lakes(hipStream_t s, const uint32_t *parent, const uint32_t *size, size_t n_colours,
                      uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t level, const uint32_t *death) {
  k_emit_lakes<<<(unsigned)emit_blocks_for(n_colours), 256, 0, s>>>(parent, size, n_colours, lakes, cap, level_counts, level, death);
  return hipGetLastError();
}

// ---- merging transform_to_list at size: records from the list of LIVE lakes ------------------------------------------------
//
// k_emit_lakes looks at every colour at every level: 255 x S visits (8192^2: 1.9 G) for 0.62 G records -- 45 of the 67 ms of a
// transform_to_list there.  A lake of level l was a lake of level l - 1 (every seed's colour holds its seed pixel from the
// start, lib.rs:1670-1677, and lakes only ever merge), so level l's lakes are found among level l - 1's: the kernel below reads
// the list of the lakes alive at the level before (all colours, for level 0), keeps those that are still roots with pixels, and
// writes their records AND the next list in the same positions (one ticket per 4096 candidates).  Work per level: the live lakes.
// sd[c] = (area, death level): one 8-byte gather per candidate.
constexpr int ALIVE_PER_THREAD = 16;
constexpr int ALIVE_CHUNK = 256 * ALIVE_PER_THREAD;

__global__ void k_sd_init(uint2 *sd, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) sd[i] = make_uint2(0u, 0xFFFFFFFFu);
}

hipError_t sd_init(hipStream_t s, uint2 *sd, size_t n) {
  if (n == 0) return hipSuccess;
  k_sd_init<<<(unsigned)std::min<size_t>((n + 1023) / 1024, 8192), 256, 0, s>>>(sd, n);
  return hipGetLastError();
}

// level L's records (and live list) from level L - 1's live list.  bid / nblocks: this job's share of the launch.
__device__ __forceinline__ void emit_alive_body(const uint2 *__restrict__ sd, size_t n_colours, const uint32_t *__restrict__ alive_in,
                                                uint32_t *alive_out, uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t L,
                                                unsigned bid, unsigned nblocks) {
  __shared__ u64c s_base, s_first;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < 64) {      // records of the earlier levels: their counters are final (earlier launches)
    u64c before = 0;
    for (uint32_t j = (uint32_t)lane; j < L; j += 64) before += level_counts[j];
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) s_base = before;
  }
  const size_t n_in = L == 0 ? (n_colours > 0 ? n_colours - 1 : 0) : (size_t)level_counts[L - 1];
  // Candidates are dealt out lane by lane (slab k of a chunk = 256 consecutive candidates: a wave's loads and its sd gathers
  // are coalesced while the list is sorted) and the survivors KEEP THEIR ORDER inside the chunk (chunks draw their tickets in
  // about the order of their indices), so the list stays nearly sorted by colour from level to level.  (Written out in
  // (wave, slab, lane) order the list was reshuffled at every level and level 50's gathers -- 4 M live lakes -- took twice as
  // long as level 0's 7.3 M sequential ones; sixteen CONSECUTIVE candidates per thread kept the order but made every load a
  // 64-line gather: 97 us for level 0 instead of 40.)
  __shared__ uint32_t s_cnt[ALIVE_PER_THREAD][4];
  for (size_t chunk = bid; chunk * ALIVE_CHUNK < n_in; chunk += nblocks) {
    uint32_t col[ALIVE_PER_THREAD], area[ALIVE_PER_THREAD];
    unsigned long long m[ALIVE_PER_THREAD];
#pragma unroll
    for (int k = 0; k < ALIVE_PER_THREAD; ++k) {
      const size_t i = chunk * ALIVE_CHUNK + (size_t)k * 256 + threadIdx.x;
      col[k] = i < n_in ? (L == 0 ? (uint32_t)i + 1u : alive_in[i]) : 0u;      // colour 0 = uncoloured: never a lake
    }
#pragma unroll
    for (int k = 0; k < ALIVE_PER_THREAD; ++k) {
      const uint2 v = sd[col[k]];
      area[k] = v.x;
      m[k] = __builtin_amdgcn_ballot_w64(col[k] != 0u && v.x != 0u && v.y > L);
    }
    __syncthreads();      // (s_cnt / s_first of the previous chunk have been read)
    if (lane < ALIVE_PER_THREAD) {
      unsigned long long mk = m[0];
#pragma unroll
      for (int k = 1; k < ALIVE_PER_THREAD; ++k) mk = lane == k ? m[k] : mk;
      s_cnt[lane][wave] = (uint32_t)__popcll(mk);
    }
    __syncthreads();
    // exclusive prefix over (slab, wave) in that order: where this wave's survivors of slab k start
    uint32_t start[ALIVE_PER_THREAD], run = 0;
#pragma unroll
    for (int k = 0; k < ALIVE_PER_THREAD; ++k) {
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        if (w == wave) start[k] = run;
        run += s_cnt[k][w];
      }
    }
    const uint32_t block_total = run;
    if (block_total == 0) continue;            // workgroup uniform
    if (threadIdx.x == 0) s_first = atomicAdd(level_counts + L, (u64c)block_total);
    __syncthreads();
    const u64c first = s_first;
#pragma unroll
    for (int k = 0; k < ALIVE_PER_THREAD; ++k) {
      if ((m[k] >> lane) & 1ull) {
        const u64c r = first + start[k] + (u64c)__popcll(m[k] & ((1ull << lane) - 1ull));      // position inside the level
        alive_out[r] = col[k];
        const u64c p = s_base + r;
        if (p < cap) {
          lakes[2 * p] = (uint64_t)col[k];
          lakes[2 * p + 1] = (uint64_t)area[k];
        }
      }
    }
  }
}

// the unions of `level` (sd[c].y = level for every root they hook) and, side by side, the records of level - 1
__global__ __launch_bounds__(256) void k_union_emit_alive(const uint2 *__restrict__ edge_items, const u64c *__restrict__ range, unsigned union_blocks,
                                                          uint32_t *parent, uint32_t *hooked, uint32_t *hooked_count, uint2 *sd, uint32_t level,
                                                          size_t n_colours, const uint32_t *__restrict__ alive_in, uint32_t *alive_out,
                                                          uint64_t *lakes, size_t cap, u64c *level_counts) {
  if (blockIdx.x < union_blocks) {
    edge_items += range[0];
    const size_t n = (size_t)(range[1] - range[0]);
    const size_t step = (size_t)union_blocks * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
      const uint2 e = edge_items[i];
      const uint32_t lost = uf_union(parent, e.x, e.y);
      if (lost != 0xFFFFFFFFu) {
        hooked[atomicAdd(hooked_count, 1u)] = lost;
        sd[lost].y = level;
      }
    }
  } else if (level > 0) {
    emit_alive_body(sd, n_colours, alive_in, alive_out, lakes, cap, level_counts, level - 1, blockIdx.x - union_blocks, gridDim.x - union_blocks);
  }
}

__global__ __launch_bounds__(256) void k_emit_alive(const uint2 *__restrict__ sd, size_t n_colours, const uint32_t *__restrict__ alive_in,
                                                    uint32_t *alive_out, uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t L) {
  emit_alive_body(sd, n_colours, alive_in, alive_out, lakes, cap, level_counts, L, blockIdx.x, gridDim.x);
}

// alive: two lists of alive_list_words(n_colours) words; level L reads list (L + 1) & 1 and writes list L & 1
size_t alive_list_words(size_t n_colours) { return (n_colours + 3) & ~(size_t)3; }      // 16-byte aligned lists

hipError_t union_emit_alive(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned union_grid, uint32_t *parent, uint32_t *hooked,
                            uint32_t *hooked_count, uint2 *sd, uint32_t level, size_t n_colours, uint32_t *alive, unsigned emit_grid,
                            uint64_t *lakes, size_t cap, u64c *level_counts) {
  const uint32_t L = level - 1;      // the level whose records ride along (level > 0)
  const size_t stride = alive_list_words(n_colours);
  k_union_emit_alive<<<union_grid + (level > 0 ? emit_grid : 0u), 256, 0, s>>>(edge_items, range, union_grid, parent, hooked, hooked_count, sd, level,
                                                                             n_colours, alive + (size_t)((L + 1) & 1u) * stride,
                                                                             alive + (size_t)(L & 1u) * stride, lakes, cap, level_counts);
  return hipGetLastError();
}

hipError_t emit_alive(hipStream_t s, const uint2 *sd, size_t n_colours, uint32_t *alive, unsigned emit_grid, uint64_t *lakes, size_t cap,
                      u64c *level_counts, uint32_t L) {
  const size_t stride = alive_list_words(n_colours);
  k_emit_alive<<<emit_grid, 256, 0, s>>>(sd, n_colours, alive + (size_t)((L + 1) & 1u) * stride, alive + (size_t)(L & 1u) * stride, lakes, cap,
                                         level_counts, L);
  return hipGetLastError();
}

// k_fold_and_add on sd[].x, for planes where a level brings hundreds of thousands of pixels to a handful of lakes: a wave adds
// up the RUN of items that go to one root (the common case late in the flood: all of them) over its four steps and adds once,
// and the four waves of a workgroup that end on the same root add once together -- a same-address atomic retires every ~12 ns,
// and one per wave and step was 49 of the kernel's 74 us per level at 8192^2.
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {      // total of v over the wave, in every lane
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

constexpr int FOLD_STEPS = 4;      // items per thread of the counting half

__global__ __launch_bounds__(256) void k_fold_and_add_sd(const uint32_t *__restrict__ hooked, const uint32_t *__restrict__ hooked_count,
                                                         const uint32_t *__restrict__ px_items, const u64c *__restrict__ range,
                                                         uint32_t *parent, uint2 *sd) {
  __shared__ uint32_t s_root[4], s_cnt[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned half = gridDim.x / 2;
  uint32_t *size = reinterpret_cast<uint32_t *>(sd);      // area of colour c: size[2 c]
  if (blockIdx.x >= half) {
    // folds: the areas of the roots hooked at this level go to the roots they ended under
    const unsigned bid = blockIdx.x - half;
    const uint32_t nh = *hooked_count;
    for (size_t base = (size_t)bid * 256; base < nh; base += (size_t)half * 256) {
      const size_t i = base + threadIdx.x;
      const bool active = i < nh;
      const uint32_t b = active ? hooked[i] : 0u;
      const uint32_t area = active ? size[2 * (size_t)b] : 0u;
      const uint32_t r = active && area ? uf_find(parent, b) : 0xFFFFFFFFu;
      unsigned long long todo = __builtin_amdgcn_ballot_w64(r != 0xFFFFFFFFu);
      for (int round = 0; round < 2 && todo != 0; ++round) {      // the one or two lakes that swallow most of the others
        const int leader = (int)__builtin_ctzll(todo);
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);
        const bool same = r == r0;
        const uint32_t sum = wave_sum_u32(same ? area : 0u);
        if (lane == leader) atomicAdd(&size[2 * (size_t)r0], sum);
        todo &= ~__builtin_amdgcn_ballot_w64(same);
      }
      if ((todo >> lane) & 1ull) atomicAdd(&size[2 * (size_t)r], area);
    }
    return;
  }
  // arrivals: a workgroup takes 256 * FOLD_STEPS consecutive items
  const u64c first = range[0];
  const size_t n = (size_t)(range[1] - first);
  px_items += first;
  for (size_t base = (size_t)blockIdx.x * (256 * FOLD_STEPS); base < n; base += (size_t)half * (256 * FOLD_STEPS)) {
    uint32_t run_root = 0xFFFFFFFFu, run_cnt = 0;      // wave uniform
#pragma unroll
    for (int st = 0; st < FOLD_STEPS; ++st) {
      const size_t i = base + (size_t)st * 256 + threadIdx.x;
      const bool active = i < n;
      const uint32_t r = active ? uf_find(parent, px_items[i]) : 0xFFFFFFFFu;
      unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
      if (todo != 0) {
        const int leader = (int)__builtin_ctzll(todo);
        const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r, leader);
        const unsigned long long same = __builtin_amdgcn_ballot_w64(active && r == r0);
        if (r0 != run_root) {
          if (run_cnt && lane == 0) atomicAdd(&size[2 * (size_t)run_root], run_cnt);
          run_root = r0;
          run_cnt = 0;
        }
        run_cnt += (uint32_t)__popcll(same);
        todo &= ~same;
        // what is left (early levels: every lane another lake): two more rounds of leader election, then one add per lane
        for (int round = 0; round < 2 && todo != 0; ++round) {
          const int l2 = (int)__builtin_ctzll(todo);
          const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)r, l2);
          const unsigned long long s2 = __builtin_amdgcn_ballot_w64(active && r == r2);
          if (lane == l2) atomicAdd(&size[2 * (size_t)r2], (uint32_t)__popcll(s2));
          todo &= ~s2;
        }
        if ((todo >> lane) & 1ull) atomicAdd(&size[2 * (size_t)r], 1u);
      }
    }
    // the waves' runs: one add per distinct root of the workgroup (all four equal late in the flood)
    __syncthreads();
    if (lane == 0) { s_root[wave] = run_cnt ? run_root : 0xFFFFFFFFu; s_cnt[wave] = run_cnt; }
    __syncthreads();
    if (threadIdx.x < 4 && s_root[threadIdx.x] != 0xFFFFFFFFu) {
      bool first_of_its_root = true;
      uint32_t total = 0;
      for (int k = 0; k < 4; ++k)
        if (s_root[k] == s_root[threadIdx.x]) { if (k < (int)threadIdx.x) first_of_its_root = false; total += s_cnt[k]; }
      if (first_of_its_root) atomicAdd(&size[2 * (size_t)s_root[threadIdx.x]], total);
    }
  }
}

hipError_t fold_and_add_sd(hipStream_t s, const uint32_t *hooked, const uint32_t *hooked_count, const uint32_t *px_items, const u64c *range,
                           unsigned grid, uint32_t *parent, uint2 *sd) {
  k_fold_and_add_sd<<<2 * grid, 256, 0, s>>>(hooked, hooked_count, px_items, range, parent, sd);
  return hipGetLastError();
}

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
  k_block_union_pixels<<<(unsigned)std::min<size_t>((n + 255) / 256, 8192), 256, 0, s>>>(labels, h, w, row0, H, parent, col0, W < 0 ? w : W);
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

// ---- final-only path ---------------------------------------------------------------------

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

typedef uint32_t u32x4_m __attribute__((ext_vector_type(4)));

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

// tile_min: union_image_tiles(h, w) words of scratch
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
    const int blocks = (int)std::min<size_t>((n_seeds + 1023) / 1024, 16384);      // four seeds per thread
    k_union_seeds<<<blocks, 256, 0, s>>>(labels, seeds_rc, n_seeds, h, w, tx, tile_min, parent, tile_root_mark);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    k_tile_edges<<<tx * ty, 256, 0, s>>>(labels, h, w, tx, ty, tile_min, parent);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  k_union_tiles<<<tx * ty, 256, 0, s>>>(labels, h, w, tx, parent, tile_min);
  return hipGetLastError();
}
size_t union_image_tiles(int h, int w) { return (size_t)((w + UT - 1) / UT) * ((h + UT - 1) / UT); }

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
  const int fb = (int)std::min<size_t>((n_colours + 255) / 256, 8192);
  k_uf_flatten<<<fb > 0 ? fb : 1, 256, 0, s>>>(parent, n_colours);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int blocks = (int)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  k_relabel_flat<<<blocks, 256, 0, s>>>(labels, parent, out, n);
  return hipGetLastError();
}

template <typename OutT>
__global__ void k_relabel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, uint32_t *parent,
                          OutT *out, size_t n, uint32_t level) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) {
    const uint32_t k = keys[i];
    OutT v = 0;
    if (k != KEY_INF && (k >> 24) <= level) v = (OutT)uf_find(parent, labels[i]);    // lib.rs:589-592 with the closed map
    out[i] = v;
  }
}

hipError_t relabel_u32(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *parent,
                       uint32_t *out, size_t n, uint32_t level) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192);
  k_relabel<uint32_t><<<blocks, 256, 0, s>>>(keys, labels, parent, out, n, level);
  return hipGetLastError();
}

hipError_t relabel_u64(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *parent,
                       uint64_t *out, size_t n, uint32_t level) {
  if (n == 0) return hipSuccess;
  const int blocks = (int)((n + 1023) / 1024 < 8192 ? (n + 1023) / 1024 : 8192);
  k_relabel<uint64_t><<<blocks, 256, 0, s>>>(keys, labels, parent, out, n, level);
  return hipGetLastError();
}

// ---- transform_history on the device (ws_transform_history_device) --------------------------------------------------------------
//
// The per-level unions leave a level-stamped merge forest beside the union-find: when a CAS hooks root b under a, hook[b] = a
// and death[b] = the level.  parent[] cannot serve: path halving rewrites it in later levels.  The lake of colour c at level L
// is then found by walking hook[] from c while death[x] <= L (DESIGN.md section 4.1 has the argument that the walk ends at the
// lake's smallest colour, the canonical id, whatever order the racing CASes took).

// uf_union that also names the root the loser was hooked under
__device__ __forceinline__ uint32_t uf_union_to(uint32_t *parent, uint32_t a, uint32_t b, uint32_t *winner) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return 0xFFFFFFFFu;
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicCAS(parent + b, b, a);
    if (old == b) { *winner = a; return b; }
    b = old;
  }
}

__global__ __launch_bounds__(256) void k_union_stamped(const uint2 *__restrict__ edge_items, const u64c *__restrict__ range, uint32_t *parent,
                                                       uint32_t *death, uint32_t *hook, uint32_t level) {
  edge_items += range[0];
  const size_t n = (size_t)(range[1] - range[0]);
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const uint2 e = edge_items[i];
    uint32_t a = 0;
    const uint32_t lost = uf_union_to(parent, e.x, e.y, &a);
    if (lost != 0xFFFFFFFFu) {      // once per colour: only the CAS that ends its time as a root gets here
      hook[lost] = a;
      death[lost] = level;
    }
  }
}

hipError_t union_stamped_ranged(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned grid, uint32_t *parent, uint32_t *death,
                                uint32_t *hook, uint32_t level) {
  k_union_stamped<<<grid, 256, 0, s>>>(edge_items, range, parent, death, hook, level);
  return hipGetLastError();
}

// One pass for every requested level: a pixel's stamp and colour are read once, then the levels are walked in ascending order
// and every plane gets its four pixels as one 16-byte store.  The merging colour follows the stamped forest up as L grows:
// the walk only ever moves on, and death[] of the colour it stands on is kept in a register, so a level at which the lake did
// not merge costs no load.
// STACKED (ws_transform_history_batch_device): keys / labels are slices of st.plane pixels, labels in each slice's own colours;
// slice kr's colour c is c + st.base[kr] in the forest, and its planes start at out + kr * st.per_slice * plane_stride.
// st.plane % 4 == 0, so a quad never straddles two slices.
template <bool MERGING, bool STACKED>
__global__ __launch_bounds__(256) void k_render_history(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                        const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook,
                                                        HistoryTable tab, uint32_t *out, size_t plane_stride, size_t n, HistoryStack st) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0 &&
                   (plane_stride & 3u) == 0 && (!STACKED || (st.plane & 3u) == 0);
  const size_t nq = vec ? n / 4 : 0;
  for (size_t q = tid; q < nq; q += step) {
    const u32x4_m k = reinterpret_cast<const u32x4_m *>(keys)[q], l = reinterpret_cast<const u32x4_m *>(labels)[q];
    uint32_t arr[4] = {k.x >> 24, k.y >> 24, k.z >> 24, k.w >> 24};      // arrival level; KEY_INF: 255, above every level
    uint32_t col[4] = {l.x, l.y, l.z, l.w}, d[4];
    size_t o = 0;      // (STACKED) the quad's word in its slice's first plane
    uint32_t b = 0;    // (STACKED, MERGING) the slice's colour base
    if constexpr (STACKED) {
      const uint32_t i = (uint32_t)(4 * q), kr = i / st.plane;
      o = (size_t)kr * st.per_slice * plane_stride + (i - kr * st.plane);
      if constexpr (MERGING) b = st.base[kr];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (col[p] == 0u) arr[p] = 0xFFu;
      if constexpr (STACKED && MERGING) col[p] += b;      // (colour 0 is never shown: arr = 0xFF)
      d[p] = MERGING && arr[p] != 0xFFu ? death[col[p]] : 0xFFFFFFFFu;
    }
    for (uint32_t j = 0; j < tab.n; ++j) {
      const uint32_t e = tab.e[j], L = e & 0xFFu;
      uint32_t v[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (MERGING && arr[p] <= L)
          while (d[p] <= L) { col[p] = hook[col[p]]; d[p] = death[col[p]]; }
        v[p] = arr[p] <= L ? col[p] - b : 0u;
      }
      if constexpr (STACKED)
        *reinterpret_cast<u32x4_m *>(out + (size_t)(e >> 8) * plane_stride + o) = u32x4_m{v[0], v[1], v[2], v[3]};
      else
        reinterpret_cast<u32x4_m *>(out + (size_t)(e >> 8) * plane_stride)[q] = u32x4_m{v[0], v[1], v[2], v[3]};
    }
  }
  for (size_t i = nq * 4 + tid; i < n; i += step) {      // the tail (all of the plane when a pointer or the stride is not 16-byte aligned)
    uint32_t a = keys[i] >> 24, c = labels[i];
    if (c == 0u) a = 0xFFu;
    size_t o = i;
    uint32_t b = 0;
    if constexpr (STACKED) {
      const uint32_t kr = (uint32_t)i / st.plane;
      o = (size_t)kr * st.per_slice * plane_stride + ((uint32_t)i - kr * st.plane);
      if constexpr (MERGING) b = st.base[kr];
      c += b;
    }
    uint32_t dc = MERGING && a != 0xFFu ? death[c] : 0xFFFFFFFFu;
    for (uint32_t j = 0; j < tab.n; ++j) {
      const uint32_t e = tab.e[j], L = e & 0xFFu;
      if (MERGING && a <= L)
        while (dc <= L) { c = hook[c]; dc = death[c]; }
      out[(size_t)(e >> 8) * plane_stride + o] = a <= L ? c - b : 0u;
    }
  }
}

hipError_t render_history(hipStream_t s, bool merging, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                          const HistoryTable &tab, uint32_t *out, size_t plane_stride, size_t n) {
  if (n == 0 || tab.n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  if (merging) k_render_history<true, false><<<blocks, 256, 0, s>>>(keys, labels, death, hook, tab, out, plane_stride, n, HistoryStack{});
  else k_render_history<false, false><<<blocks, 256, 0, s>>>(keys, labels, nullptr, nullptr, tab, out, plane_stride, n, HistoryStack{});
  return hipGetLastError();
}

hipError_t render_history_stack(hipStream_t s, bool merging, const uint32_t *keys, const uint32_t *labels, const uint32_t *death,
                                const uint32_t *hook, const HistoryTable &tab, uint32_t *out, size_t plane_stride, size_t n,
                                const HistoryStack &st) {
  if (n == 0 || tab.n == 0) return hipSuccess;
  if (st.plane == 0 || n % st.plane != 0 || n > 0xFFFFFFFFull) return hipErrorInvalidValue;      // (slice indices are u32 divisions)
  const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  if (merging) k_render_history<true, true><<<blocks, 256, 0, s>>>(keys, labels, death, hook, tab, out, plane_stride, n, st);
  else k_render_history<false, true><<<blocks, 256, 0, s>>>(keys, labels, nullptr, nullptr, tab, out, plane_stride, n, st);
  return hipGetLastError();
}

// ---- merge tree (ws_merge_tree_device) ----------------------------------------------------------------------------------------------
//
// The stamped forest of a merging transform_history run IS the lake hierarchy, up to two things: hook[b] is whatever root the racing
// CAS read, not the canonical id, and nothing has counted pixels.  Three steps turn it into one record per colour:
// canonical parents (one walk per colour), own counts (one pass over the stamps), and a fold up the tree in ascending death level.

constexpr int TREE_PER_THREAD = 16;      // colours per thread of the per-colour kernels: a workgroup adds once per level to 256 shared counters
constexpr int TREE_CHUNK = 256 * TREE_PER_THREAD;

__device__ __forceinline__ uint32_t slice_of_colour(const uint32_t *base, uint32_t g, uint32_t c);      // (with the stack's kernels, below)

// STACKED (ws_merge_tree_batch_device): the forest is that of a stack of st.g slices of st.plane pixels (H = g x slice rows); colour
// c of the forest is colour c - st.base[k] of its slice k, seeds_rc are the stacked seed pairs (flood_stack) and seg holds every
// slice's own colours.  Record 0 of the forest belongs to nobody: every slice's own comes from k_tree_unstack.
template <bool STACKED>
__global__ __launch_bounds__(256) void k_tree_init(const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook,
                                                   const uint32_t *__restrict__ seeds_rc, const uint32_t *__restrict__ seg, int H, int W,
                                                   const u64c *__restrict__ arrived, TreeRec *tree, size_t n_colours, u64c *hist, TreeStack st) {
  __shared__ uint32_t s_h[NLEVELS];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  for (int k = 0; k < TREE_PER_THREAD; ++k) {
    const size_t c = (size_t)blockIdx.x * TREE_CHUNK + (size_t)k * 256 + threadIdx.x;
    if (c >= n_colours) break;
    TreeRec r{0u, TREE_ALIVE, 0u, 0u};
    if (c == 0) {
      if constexpr (!STACKED) r.area = (uint32_t)((u64c)H * (u64c)W - arrived[0]);      // what the last level left uncoloured
    } else {
      const uint32_t y = seeds_rc[2 * (c - 1)], x = seeds_rc[2 * (c - 1) + 1];
      uint32_t own = (uint32_t)c;      // the colour in the plane's own numbering
      if constexpr (STACKED) own -= st.base[slice_of_colour(st.base, st.g, (uint32_t)c)];
      // a later seed on the same pixel overwrites (lib.rs:1670-1677): such a colour never was
      r.n_leaves = y < (uint32_t)H && x < (uint32_t)W && seg[(size_t)y * W + x] == own ? 1u : 0u;
      const uint32_t d = death[c];
      if (d != TREE_ALIVE) {
        uint32_t p = hook[c];
        while (death[p] <= d) p = hook[p];      // <=: a colour that dies at the same level is not that level's root
        r.parent = p;
        r.death_level = d;
        atomicAdd(&s_h[d & (NLEVELS - 1)], 1u);
      }
    }
    tree[c] = r;
  }
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (u64c)s_h[threadIdx.x]);
}

hipError_t tree_init(hipStream_t s, const uint32_t *death, const uint32_t *hook, const uint32_t *seeds_rc, const uint32_t *seg_labels, int h, int w,
                     const u64c *arrived, TreeRec *tree, size_t n_colours, u64c *ws) {
  if (n_colours == 0) return hipSuccess;
  k_tree_init<false><<<(unsigned)((n_colours + TREE_CHUNK - 1) / TREE_CHUNK), 256, 0, s>>>(death, hook, seeds_rc, seg_labels, h, w, arrived, tree, n_colours, ws,
                                                                                           TreeStack{});
  return hipGetLastError();
}

hipError_t tree_init_stack(hipStream_t s, const uint32_t *death, const uint32_t *hook, const uint32_t *stacked_rc, const uint32_t *seg_labels, int h, int w,
                           TreeRec *tree, size_t n_colours, u64c *ws, const TreeStack &st) {
  if (n_colours == 0) return hipSuccess;
  if (st.g == 0 || st.plane == 0 || (size_t)h * (size_t)w != (size_t)st.g * st.plane) return hipErrorInvalidValue;
  k_tree_init<true><<<(unsigned)((n_colours + TREE_CHUNK - 1) / TREE_CHUNK), 256, 0, s>>>(death, hook, stacked_rc, seg_labels, h, w, nullptr, tree, n_colours, ws, st);
  return hipGetLastError();
}

// The seed pixels of a finished transform, from its planes alone (ws_merge_tree_from_arrival_device).  A seed is coloured before
// level 0 (lib.rs:1675-1677) and nothing else is: stamp 0 marks exactly the painted pixels, and the label there is the colour that
// survived the painting.  So every colour that exists has ONE stamp-0 pixel, which writes its (row, col) pair -- no atomics -- and
// a colour that never was keeps the pair the fill left, which k_tree_init reads as "outside the plane".  A plain stream over the
// stamps, 16 bytes a lane; the labels are read only where a stamp is 0.  A label outside 1 .. n_seeds is never an index.
__device__ __forceinline__ void seed_pixel_at(const uint32_t *__restrict__ seg, size_t i, uint32_t W, uint32_t n_seeds, uint2 *out_rc) {
  const uint32_t c = seg[i];
  if (c - 1u < n_seeds) out_rc[c - 1u] = make_uint2((uint32_t)(i / W), (uint32_t)(i % W));
}

__global__ __launch_bounds__(256) void k_seed_pixels(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ seg, size_t n, uint32_t W,
                                                     uint32_t n_seeds, uint2 *out_rc) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const size_t nq = (reinterpret_cast<uintptr_t>(keys) & 15u) == 0 ? n / 4 : 0;
  for (size_t q = tid; q < nq; q += step) {
    const u32x4_m k = reinterpret_cast<const u32x4_m *>(keys)[q];
    if (k.x != 0u && k.y != 0u && k.z != 0u && k.w != 0u) continue;
    if (k.x == 0u) seed_pixel_at(seg, 4 * q, W, n_seeds, out_rc);
    if (k.y == 0u) seed_pixel_at(seg, 4 * q + 1, W, n_seeds, out_rc);
    if (k.z == 0u) seed_pixel_at(seg, 4 * q + 2, W, n_seeds, out_rc);
    if (k.w == 0u) seed_pixel_at(seg, 4 * q + 3, W, n_seeds, out_rc);
  }
  for (size_t i = nq * 4 + tid; i < n; i += step)      // the tail (all of the plane when the stamps are a view off 16-byte alignment)
    if (keys[i] == 0u) seed_pixel_at(seg, i, W, n_seeds, out_rc);
}

hipError_t seed_pixels_from_planes(hipStream_t s, const uint32_t *keys, const uint32_t *seg, int h, int w, size_t n_colours, uint32_t *out_rc) {
  if (n_colours <= 1) return hipSuccess;
  if (n_colours > 0xFFFFFFFFull || (reinterpret_cast<uintptr_t>(out_rc) & 7u) != 0) return hipErrorInvalidValue;
  const size_t n = (size_t)h * (size_t)w, n_seeds = n_colours - 1;
  hipError_t e = hipMemsetAsync(out_rc, 0xFF, 2 * n_seeds * sizeof(uint32_t), s);
  if (e != hipSuccess || n == 0) return e;
  const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  k_seed_pixels<<<blocks, 256, 0, s>>>(keys, seg, n, (uint32_t)w, (uint32_t)n_seeds, reinterpret_cast<uint2 *>(out_rc));
  return hipGetLastError();
}

// Own counts.  Around the percolation level most pixels of the plane land on ONE root, and a same-address atomic retires every ~12 ns:
// a workgroup takes a contiguous run of pixels, counts in an LDS table keyed by root (a wave first adds up the lanes that agree with
// its first lane) and adds to memory once per root it met.  A root that finds no slot within OWN_PROBES adds for itself: exact either way.
constexpr int OWN_SLOTS = 2048, OWN_PROBES = 4;
constexpr uint32_t OWN_EMPTY = 0xFFFFFFFFu;

__device__ __forceinline__ void own_add(uint32_t *s_key, uint32_t *s_cnt, TreeRec *tree, uint32_t r, uint32_t k) {
  const uint32_t h0 = (r * 2654435761u) >> 21;      // 11 bits
  for (int j = 0; j < OWN_PROBES; ++j) {
    const uint32_t slot = (h0 + (uint32_t)j) & (OWN_SLOTS - 1);
    const uint32_t old = atomicCAS(&s_key[slot], OWN_EMPTY, r);
    if (old == OWN_EMPTY || old == r) { atomicAdd(&s_cnt[slot], k); return; }
  }
  atomicAdd(&tree[r].area, k);
}

// STACKED: labels hold every slice's own colours; a quad's slice is i0 / stack.plane (stack.plane % 4 == 0: a quad never straddles two
// slices, a workgroup's runs may) and its colours move to the forest's numbering before the walk, so the table is keyed by forest root.
template <bool STACKED>
__global__ __launch_bounds__(256) void k_tree_own(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                  const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook, TreeRec *tree,
                                                  size_t n, size_t steps, TreeStack stack) {
  __shared__ uint32_t s_key[OWN_SLOTS], s_cnt[OWN_SLOTS];
  for (int j = threadIdx.x; j < OWN_SLOTS; j += 256) { s_key[j] = OWN_EMPTY; s_cnt[j] = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool vec = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t i0 = (((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x) * 4;
    uint32_t arr[4], col[4];
    if (vec && i0 + 3 < n) {
      const u32x4_m k = *reinterpret_cast<const u32x4_m *>(keys + i0), l = *reinterpret_cast<const u32x4_m *>(labels + i0);
      arr[0] = k.x >> 24; arr[1] = k.y >> 24; arr[2] = k.z >> 24; arr[3] = k.w >> 24;
      col[0] = l.x; col[1] = l.y; col[2] = l.z; col[3] = l.w;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool in = i0 + p < n;
        arr[p] = in ? keys[i0 + p] >> 24 : 0xFFu;
        col[p] = in ? labels[i0 + p] : 0u;
      }
    }
    if constexpr (STACKED) {
      const uint32_t b = i0 < n ? stack.base[(uint32_t)i0 / stack.plane] : 0u;      // (n < 2^32: tree_own_counts_stack)
#pragma unroll
      for (int p = 0; p < 4; ++p) col[p] += col[p] != 0u ? b : 0u;
    }
    // the four walks side by side (a walk is a chain of dependent gathers: one after the other they were most of the kernel)
    uint32_t r[4], d[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      r[p] = col[p];
      d[p] = col[p] != 0u && arr[p] != 0xFFu ? death[col[p]] : TREE_ALIVE;      // (as k_render_history: KEY_INF and colour 0 are never shown)
    }
    for (;;) {      // the root at the pixel's arrival level
      bool go[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) go[p] = d[p] <= arr[p];
      if (!(go[0] || go[1] || go[2] || go[3])) break;
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) r[p] = hook[r[p]];
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) d[p] = death[r[p]];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool active = col[p] != 0u && arr[p] != 0xFFu;
      const unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
      if (todo == 0) continue;      // wave uniform
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r[p], leader);
      const unsigned long long same = __builtin_amdgcn_ballot_w64(active && r[p] == r0);
      if (lane == leader) own_add(s_key, s_cnt, tree, r0, (uint32_t)__popcll(same));
      else if (active && r[p] != r0) own_add(s_key, s_cnt, tree, r[p], 1u);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < OWN_SLOTS; j += 256)
    if (s_cnt[j]) atomicAdd(&tree[s_key[j]].area, s_cnt[j]);
}

hipError_t tree_own_counts(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, TreeRec *tree, size_t n) {
  if (n == 0) return hipSuccess;
  // at most two thousand workgroups on a large plane (that many adds reach the surviving lake's word), 1024 pixels a step
  const size_t quads = (n + 1023) / 1024;
  const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
  k_tree_own<false><<<(unsigned)((quads + steps - 1) / steps), 256, 0, s>>>(keys, labels, death, hook, tree, n, steps, TreeStack{});
  return hipGetLastError();
}

hipError_t tree_own_counts_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, TreeRec *tree,
                                 size_t n, const TreeStack &st) {
  if (n == 0) return hipSuccess;
  if (st.plane == 0 || (st.plane & 3u) != 0 || n != (size_t)st.g * st.plane || n > 0xFFFFFFFFull) return hipErrorInvalidValue;      // (slice indices are u32 divisions)
  const size_t quads = (n + 1023) / 1024;
  const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
  k_tree_own<true><<<(unsigned)((quads + steps - 1) / steps), 256, 0, s>>>(keys, labels, death, hook, tree, n, steps, st);
  return hipGetLastError();
}

// bounds of the death levels' buckets (ws + NLEVELS + 1: NLEVELS + 1 words) and the scatter's cursors (behind them), from the counts
__global__ __launch_bounds__(NLEVELS) void k_tree_offsets(u64c *ws) {
  __shared__ u64c s_a[NLEVELS];
  const int t = threadIdx.x;
  const u64c a0 = ws[t];
  s_a[t] = a0;
  __syncthreads();
  for (int o = 1; o < NLEVELS; o <<= 1) {
    const u64c a = t >= o ? s_a[t - o] : 0ull;
    __syncthreads();
    s_a[t] += a;
    __syncthreads();
  }
  u64c *off = ws + NLEVELS + 1, *cur = off + NLEVELS + 1;
  off[t] = cur[t] = s_a[t] - a0;
  if (t == NLEVELS - 1) off[NLEVELS] = s_a[t];
}

// order[]: the dying colours by death level; a workgroup reserves once per level for its TREE_CHUNK colours
__global__ __launch_bounds__(256) void k_tree_scatter(const TreeRec *__restrict__ tree, size_t n_colours, u64c *cursor, uint32_t *order) {
  __shared__ uint32_t s_n[NLEVELS];
  __shared__ u64c s_base[NLEVELS];
  s_n[threadIdx.x] = 0;
  __syncthreads();
  uint32_t d[TREE_PER_THREAD];
#pragma unroll
  for (int k = 0; k < TREE_PER_THREAD; ++k) {
    const size_t c = (size_t)blockIdx.x * TREE_CHUNK + (size_t)k * 256 + threadIdx.x;
    d[k] = c < n_colours ? tree[c].death_level : TREE_ALIVE;
    if (d[k] != TREE_ALIVE) atomicAdd(&s_n[d[k] & (NLEVELS - 1)], 1u);
  }
  __syncthreads();
  {
    const uint32_t cnt = s_n[threadIdx.x];
    s_base[threadIdx.x] = cnt ? atomicAdd(&cursor[threadIdx.x], (u64c)cnt) : 0ull;
  }
  __syncthreads();
  s_n[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TREE_PER_THREAD; ++k) {
    if (d[k] == TREE_ALIVE) continue;
    const uint32_t l = d[k] & (NLEVELS - 1);
    order[s_base[l] + atomicAdd(&s_n[l], 1u)] = (uint32_t)((size_t)blockIdx.x * TREE_CHUNK + (size_t)k * 256 + threadIdx.x);
  }
}

// One death level: every colour of the bucket hands its area and its leaves to its parent.  Late levels hand thousands of lakes to ONE
// parent: a wave adds up the lanes that share a parent (two rounds of leader election) before it adds, as k_fold_and_add_sd does.
// A colour that dies at level 0 never was a lake after a flood: it hands on no pixel (its seed pixel was counted for the root of
// level 0) and keeps area 1, the seed alone.
__global__ __launch_bounds__(256) void k_tree_fold(TreeRec *tree, const uint32_t *__restrict__ order, const u64c *__restrict__ range, uint32_t level) {
  const u64c first = range[0];
  const size_t n = (size_t)(range[1] - first);
  const int lane = threadIdx.x & 63;
  order += first;
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {      // uniform trip count per wave
    const size_t i = base + threadIdx.x;
    const bool active = i < n;
    const uint32_t c = active ? order[i] : 0u;
    uint32_t p = 0xFFFFFFFFu, area = 0, leaves = 0;
    if (active) {
      const TreeRec r = tree[c];
      p = r.parent; area = r.area; leaves = r.n_leaves;
      if (level == 0) tree[c].area = 1u;
    }
    unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
    for (int round = 0; round < 2 && todo != 0; ++round) {
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)p, leader);
      const bool same = active && p == p0;
      const uint32_t sa = wave_sum_u32(same ? area : 0u), sl = wave_sum_u32(same ? leaves : 0u);
      if (lane == leader) {
        if (sa) atomicAdd(&tree[p0].area, sa);
        if (sl) atomicAdd(&tree[p0].n_leaves, sl);
      }
      todo &= ~__builtin_amdgcn_ballot_w64(same);
    }
    if ((todo >> lane) & 1ull) {
      if (area) atomicAdd(&tree[p].area, area);
      if (leaves) atomicAdd(&tree[p].n_leaves, leaves);
    }
  }
}

hipError_t tree_fold(hipStream_t s, TreeRec *tree, size_t n_colours, uint32_t levels, u64c *ws, uint32_t *order) {
  if (n_colours <= 1) return hipSuccess;
  k_tree_offsets<<<1, NLEVELS, 0, s>>>(ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  u64c *off = ws + NLEVELS + 1;
  k_tree_scatter<<<(unsigned)((n_colours + TREE_CHUNK - 1) / TREE_CHUNK), 256, 0, s>>>(tree, n_colours, off + NLEVELS + 1, order);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // a level's bucket is known on the device only: a fixed grid that strides (an even spread would be colours / levels per level)
  const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
  for (uint32_t l = 0; l < levels; ++l) {
    k_tree_fold<<<grid, 256, 0, s>>>(tree, order, off + l, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- lake statistics (ws_merge_tree_stats_device) ------------------------------------------------------------
//
// What carries `area` up the tree carries any commutative per-pixel quantity: five u64 sums, a box, the smallest weight and the
// packed peak (weight << 32 | 0xFFFFFFFF - pixel: its maximum is the FIRST pixel in row-major order that holds the largest weight).
// Sums, minima and maxima of integers do not depend on the order the atomics arrive in: every record is reproducible to the bit.
// The accumulators are planes of n_colours entries (sum: w, wr, wc, r, c, peak; box: r_min, r_max, c_min, c_max, w_min), so that the
// lanes of a wave that update neighbouring colours touch neighbouring words; k_lake_write turns them into the 72-byte records.

constexpr int LAKE_SLOTS = 512, LAKE_PROBES = 4;      // 72 B a slot: 36 KB a workgroup, four workgroups (16 waves) a CU of 160 KB
constexpr uint32_t LAKE_EMPTY = 0xFFFFFFFFu;

struct LakePart {
  u64c w, wr, wc, r, c, peak;
  uint32_t r_min, r_max, c_min, c_max, w_min;
};

__device__ __forceinline__ LakePart lake_none() { return LakePart{0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu}; }

__device__ __forceinline__ LakePart lake_pixel(uint32_t v, uint32_t y, uint32_t x, uint32_t i) {
  return LakePart{(u64c)v, (u64c)v * y, (u64c)v * x, (u64c)y, (u64c)x, (u64c)v << 32 | (u64c)(0xFFFFFFFFu - i), y, y, x, x, v};
}

__device__ __forceinline__ void lake_join(LakePart &a, const LakePart &b) {
  a.w += b.w; a.wr += b.wr; a.wc += b.wc; a.r += b.r; a.c += b.c;
  a.peak = a.peak > b.peak ? a.peak : b.peak;
  a.r_min = min(a.r_min, b.r_min); a.r_max = max(a.r_max, b.r_max);
  a.c_min = min(a.c_min, b.c_min); a.c_max = max(a.c_max, b.c_max);
  a.w_min = min(a.w_min, b.w_min);
}

__device__ __forceinline__ LakePart lake_wave_total(LakePart a) {      // the join over the wave, in every lane
  for (int o = 32; o > 0; o >>= 1) {
    LakePart b;
    b.w = __shfl_xor(a.w, o, 64); b.wr = __shfl_xor(a.wr, o, 64); b.wc = __shfl_xor(a.wc, o, 64);
    b.r = __shfl_xor(a.r, o, 64); b.c = __shfl_xor(a.c, o, 64); b.peak = __shfl_xor(a.peak, o, 64);
    b.r_min = __shfl_xor(a.r_min, o, 64); b.r_max = __shfl_xor(a.r_max, o, 64);
    b.c_min = __shfl_xor(a.c_min, o, 64); b.c_max = __shfl_xor(a.c_max, o, 64);
    b.w_min = __shfl_xor(a.w_min, o, 64);
    lake_join(a, b);
  }
  return a;
}

// entry i of accumulator planes of n entries each (LDS table or memory) takes a part: one atomic a field, none for a sum of 0
__device__ __forceinline__ void lake_apply(u64c *sum, uint32_t *box, size_t n, size_t i, const LakePart &a) {
  if (a.w) atomicAdd(&sum[i], a.w);
  if (a.wr) atomicAdd(&sum[n + i], a.wr);
  if (a.wc) atomicAdd(&sum[2 * n + i], a.wc);
  if (a.r) atomicAdd(&sum[3 * n + i], a.r);
  if (a.c) atomicAdd(&sum[4 * n + i], a.c);
  atomicMax(&sum[5 * n + i], a.peak);
  atomicMin(&box[i], a.r_min);
  atomicMax(&box[n + i], a.r_max);
  atomicMin(&box[2 * n + i], a.c_min);
  atomicMax(&box[3 * n + i], a.c_max);
  atomicMin(&box[4 * n + i], a.w_min);
}

__device__ __forceinline__ LakePart lake_load(const u64c *sum, const uint32_t *box, size_t n, size_t i) {
  return LakePart{sum[i], sum[n + i], sum[2 * n + i], sum[3 * n + i], sum[4 * n + i], sum[5 * n + i],
                  box[i], box[n + i], box[2 * n + i], box[3 * n + i], box[4 * n + i]};
}

__device__ __forceinline__ void lake_store(u64c *sum, uint32_t *box, size_t n, size_t i, const LakePart &a) {
  sum[i] = a.w; sum[n + i] = a.wr; sum[2 * n + i] = a.wc; sum[3 * n + i] = a.r; sum[4 * n + i] = a.c; sum[5 * n + i] = a.peak;
  box[i] = a.r_min; box[n + i] = a.r_max; box[2 * n + i] = a.c_min; box[3 * n + i] = a.c_max; box[4 * n + i] = a.w_min;
}

template <typename T>
__device__ __forceinline__ uint32_t lake_weight(const LakeWeights &wt, uint32_t y, uint32_t x) {
  const uint32_t yy = y - wt.off, xx = x - wt.off;      // (the ring wraps to far above h and w)
  return yy < wt.h && xx < wt.w ? (uint32_t)reinterpret_cast<const T *>(wt.p)[(size_t)yy * wt.stride + xx] : 0u;
}

// ... of slice k of a stack: the same plane, k slice strides on
template <typename T>
__device__ __forceinline__ uint32_t lake_weight_of_slice(const LakeWeights &wt, uint32_t k, uint32_t y, uint32_t x) {
  const uint32_t yy = y - wt.off, xx = x - wt.off;
  return yy < wt.h && xx < wt.w ? (uint32_t)reinterpret_cast<const T *>(wt.p)[(size_t)k * wt.slice_stride + (size_t)yy * wt.stride + xx] : 0u;
}

__global__ __launch_bounds__(256) void k_lake_init(u64c *sum, uint32_t *box, size_t n) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c < n) lake_store(sum, box, n, c, lake_none());
}

// a root's part into the workgroup's table; a root that finds no slot within LAKE_PROBES updates memory itself: exact either way
__device__ __forceinline__ void lake_add(uint32_t *s_key, u64c *s_sum, uint32_t *s_box, uint32_t *s_used, u64c *sum, uint32_t *box, size_t n_colours,
                                         uint32_t r, const LakePart &a) {
  const uint32_t h0 = (r * 2654435761u) >> 23;      // 9 bits
  for (int j = 0; j < LAKE_PROBES; ++j) {
    const uint32_t slot = (h0 + (uint32_t)j) & (LAKE_SLOTS - 1);
    const uint32_t old = atomicCAS(&s_key[slot], LAKE_EMPTY, r);
    if (old == LAKE_EMPTY) atomicAdd(s_used, 1u);
    if (old == LAKE_EMPTY || old == r) { lake_apply(s_sum, s_box, LAKE_SLOTS, slot, a); return; }
  }
  lake_apply(sum, box, n_colours, r, a);
}

// the table into memory, one visit per root it holds, and empty again
__device__ __forceinline__ void lake_flush(uint32_t *s_key, u64c *s_sum, uint32_t *s_box, u64c *sum, uint32_t *box, size_t n_colours) {
  for (int j = threadIdx.x; j < LAKE_SLOTS; j += 256) {
    if (s_key[j] == LAKE_EMPTY) continue;
    lake_apply(sum, box, n_colours, s_key[j], lake_load(s_sum, s_box, LAKE_SLOTS, j));
    s_key[j] = LAKE_EMPTY;
    lake_store(s_sum, s_box, LAKE_SLOTS, j, lake_none());
  }
}

// Own statistics: every pixel to the root of its colour at its arrival level (the walks of k_tree_own), an uncoloured pixel to
// record 0.  Around the percolation level most of the plane lands on ONE root and a pixel brings eleven atomics, not one: a lane
// first joins those of its four pixels that share a root, a wave joins the lanes that agree with its first lane, the workgroup's
// table takes the rest, and memory is touched once per root and workgroup.  The table lives across the workgroup's steps (the big
// lake keeps its slot) until a step leaves it more than half full: below the percolation level a long run meets thousands of small
// roots, and a table they have filled sends every newcomer to memory field by field; it is written out and starts again empty.
// STACKED (lake_stats_stack): labels hold every slice's own colours and the accumulator planes have n_colours = the forest's colours
// + stack.g entries.  A quad's slice is k = i0 / stack.plane (stack.plane % 4 == 0: a quad never straddles two slices, a workgroup's
// step may); its colours move to the forest's numbering before the walk, its uncoloured pixels go to entry n_colours - stack.g + k
// -- the slice's own record 0, which stands in for the root in the lane's join, the wave's and the table -- and rows, columns, the
// pixel index of the peak and the weight plane are those of the slice.
template <typename T, bool STACKED>
__global__ __launch_bounds__(256) void k_lake_own(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                  const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook, LakeWeights wt,
                                                  uint32_t W, u64c *sum, uint32_t *box, size_t n_colours, size_t n, size_t steps,
                                                  TreeStack stack) {
  __shared__ u64c s_sum[6 * LAKE_SLOTS];
  __shared__ uint32_t s_box[5 * LAKE_SLOTS], s_key[LAKE_SLOTS], s_used;
  for (int j = threadIdx.x; j < LAKE_SLOTS; j += 256) {
    s_key[j] = LAKE_EMPTY;
    lake_store(s_sum, s_box, LAKE_SLOTS, j, lake_none());
  }
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool vec = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  uint32_t flushed_at = 0;      // slots taken, over the run, when the table was last written out
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t i0 = (((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x) * 4;
    uint32_t arr[4], col[4];
    if (vec && i0 + 3 < n) {
      const u32x4_m k = *reinterpret_cast<const u32x4_m *>(keys + i0), l = *reinterpret_cast<const u32x4_m *>(labels + i0);
      arr[0] = k.x >> 24; arr[1] = k.y >> 24; arr[2] = k.z >> 24; arr[3] = k.w >> 24;
      col[0] = l.x; col[1] = l.y; col[2] = l.z; col[3] = l.w;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool in = i0 + p < n;
        arr[p] = in ? keys[i0 + p] >> 24 : 0xFFu;
        col[p] = in ? labels[i0 + p] : 0u;
      }
    }
    uint32_t slice = 0, none = 0;      // the quad's slice and where its uncoloured pixels go
    if constexpr (STACKED) {
      slice = i0 < n ? (uint32_t)i0 / stack.plane : 0u;      // (n < 2^32: lake_stats_stack)
      none = (uint32_t)n_colours - stack.g + slice;
      const uint32_t b = stack.base[slice];
#pragma unroll
      for (int p = 0; p < 4; ++p) col[p] += col[p] != 0u ? b : 0u;
    }
    uint32_t r[4], d[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool coloured = col[p] != 0u && arr[p] != 0xFFu;      // (as k_tree_own)
      r[p] = coloured ? col[p] : none;
      d[p] = coloured ? death[col[p]] : TREE_ALIVE;
    }
    for (;;) {      // the root at the pixel's arrival level, four walks side by side
      bool go[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) go[p] = d[p] <= arr[p];
      if (!(go[0] || go[1] || go[2] || go[3])) break;
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) r[p] = hook[r[p]];
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) d[p] = death[r[p]];
    }
    const uint32_t in0 = STACKED ? (uint32_t)i0 - slice * stack.plane : (uint32_t)i0;      // the quad's first pixel within its plane
    uint32_t y = i0 < n ? in0 / W : 0u, x = i0 < n ? in0 % W : 0u;      // (n < 2^32)
    LakePart part[4];
    bool live[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      live[p] = i0 + p < n;
      uint32_t v = 0u;
      if constexpr (STACKED) v = live[p] ? lake_weight_of_slice<T>(wt, slice, y, x) : 0u;
      else v = live[p] ? lake_weight<T>(wt, y, x) : 0u;
      part[p] = lake_pixel(v, y, x, in0 + (uint32_t)p);
      if (++x == W) { x = 0; ++y; }
    }
#pragma unroll
    for (int p = 1; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < p; ++q)
        if (live[p] && live[q] && r[p] == r[q]) { lake_join(part[q], part[p]); live[p] = false; }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned long long todo = __builtin_amdgcn_ballot_w64(live[p]);
      if (todo == 0) continue;      // wave uniform
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r[p], leader);
      const bool same = live[p] && r[p] == r0;
      if (__popcll(__builtin_amdgcn_ballot_w64(same)) > 1) {      // wave uniform
        const LakePart total = lake_wave_total(same ? part[p] : lake_none());
        if (lane == leader) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_colours, r0, total);
        else if (live[p] && !same) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_colours, r[p], part[p]);
      } else if (live[p]) {
        lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_colours, r[p], part[p]);
      }
    }
    __syncthreads();
    const uint32_t used = s_used;      // (nobody inserts between the two barriers: workgroup uniform)
    const bool full = used - flushed_at > LAKE_SLOTS / 2;
    if (full || st + 1 == steps) lake_flush(s_key, s_sum, s_box, sum, box, n_colours);
    if (full) flushed_at = used;
    __syncthreads();
  }
}

// One death level from 1 up: every colour of the bucket joins its record into its parent's (children die strictly before their
// parents: nobody reads a record another lane is adding to).  Lanes that share a parent are joined in the wave first, as k_tree_fold.
__global__ __launch_bounds__(256) void k_lake_fold(const TreeRec *__restrict__ tree, u64c *sum, uint32_t *box, size_t n_colours,
                                                   const uint32_t *__restrict__ order, const u64c *__restrict__ range) {
  const u64c first = range[0];
  const size_t n = (size_t)(range[1] - first);
  const int lane = threadIdx.x & 63;
  order += first;
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {      // uniform trip count per wave
    const size_t i = base + threadIdx.x;
    const bool active = i < n;
    uint32_t p = 0xFFFFFFFFu;
    LakePart part = lake_none();
    if (active) {
      const uint32_t c = order[i];
      p = tree[c].parent;
      part = lake_load(sum, box, n_colours, c);
    }
    unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
    for (int round = 0; round < 2 && todo != 0; ++round) {
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)p, leader);
      const bool same = active && p == p0;
      const unsigned long long with = __builtin_amdgcn_ballot_w64(same);
      if (__popcll(with) > 1) {      // wave uniform
        const LakePart total = lake_wave_total(same ? part : lake_none());
        if (lane == leader) lake_apply(sum, box, n_colours, p0, total);
      } else if (lane == leader) {
        lake_apply(sum, box, n_colours, p0, part);
      }
      todo &= ~with;
    }
    if ((todo >> lane) & 1ull) lake_apply(sum, box, n_colours, p, part);
  }
}

// The records.  A colour that dies at level 0 handed on nothing and was never the root of a pixel: it takes its seed pixel alone.
// STACKED: entry c of the n_colours accumulator entries is forest colour c (1 .. n_colours - stack.g - 1: the record at
// out[c + its slice], its seed pair in stacked rows) or slice k's uncoloured pixels (n_colours - stack.g + k: the record at
// out[base[k] + k]); entry 0 of the forest is nobody's.
template <typename T, bool STACKED>
__global__ __launch_bounds__(256) void k_lake_write(const TreeRec *__restrict__ tree, const uint32_t *__restrict__ seeds_rc, LakeWeights wt, uint32_t W,
                                                    const u64c *__restrict__ sum, const uint32_t *__restrict__ box, size_t n_colours, LakeRec *out,
                                                    TreeStack stack) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_colours) return;
  LakePart a = lake_load(sum, box, n_colours, c);
  size_t at = c;
  if constexpr (STACKED) {
    const size_t forest = n_colours - stack.g;
    if (c == 0) return;
    if (c >= forest) {
      const uint32_t k = (uint32_t)(c - forest);
      at = (size_t)stack.base[k] + k;
    } else {
      const uint32_t k = slice_of_colour(stack.base, stack.g, (uint32_t)c);
      at = c + k;
      const TreeRec t = tree[c];
      if (t.death_level == 0u && t.n_leaves != 0u) {
        const uint32_t y = seeds_rc[2 * (c - 1)] - k * (stack.plane / W), x = seeds_rc[2 * (c - 1) + 1];
        a = lake_pixel(lake_weight_of_slice<T>(wt, k, y, x), y, x, y * W + x);
      }
    }
  } else if (c != 0) {
    const TreeRec t = tree[c];
    if (t.death_level == 0u && t.n_leaves != 0u) {
      const uint32_t y = seeds_rc[2 * (c - 1)], x = seeds_rc[2 * (c - 1) + 1];
      a = lake_pixel(lake_weight<T>(wt, y, x), y, x, y * W + x);
    }
  }
  out[at] = LakeRec{a.w, a.wr, a.wc, a.r, a.c, a.r_min, a.r_max, a.c_min, a.c_max, a.w_min, (uint32_t)(a.peak >> 32),
                    0xFFFFFFFFu - (uint32_t)a.peak, 0u};
}

hipError_t lake_stats(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, const TreeRec *tree,
                      const uint32_t *seeds_rc, size_t n_colours, uint32_t levels, const u64c *ws, const uint32_t *order, const LakeWeights &wt, int h,
                      int w, void *acc, LakeRec *out) {
  if (n_colours == 0) return hipSuccess;
  const size_t n = (size_t)h * (size_t)w;
  if (n > 0xFFFFFFFFull || (reinterpret_cast<uintptr_t>(acc) & 7u) != 0) return hipErrorInvalidValue;      // (rows and columns are u32 divisions)
  u64c *sum = (u64c *)acc;
  uint32_t *box = (uint32_t *)(sum + 6 * n_colours);
  const unsigned per_colour = (unsigned)((n_colours + 255) / 256);
  k_lake_init<<<per_colour, 256, 0, s>>>(sum, box, n_colours);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (n) {      // the grid of tree_own_counts: at most two thousand workgroups, 1024 pixels a step
    const size_t quads = (n + 1023) / 1024;
    const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
    const unsigned grid = (unsigned)((quads + steps - 1) / steps);
    if (wt.u16) k_lake_own<uint16_t, false><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_colours, n, steps, TreeStack{});
    else k_lake_own<uint8_t, false><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_colours, n, steps, TreeStack{});
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_colours > 1) {      // (tree_fold built order[] and its bounds under the same condition)
    const u64c *off = ws + NLEVELS + 1;
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
    for (uint32_t l = 1; l < levels; ++l) {
      k_lake_fold<<<grid, 256, 0, s>>>(tree, sum, box, n_colours, order, off + l);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  if (wt.u16) k_lake_write<uint16_t, false><<<per_colour, 256, 0, s>>>(tree, seeds_rc, wt, (uint32_t)w, sum, box, n_colours, out, TreeStack{});
  else k_lake_write<uint8_t, false><<<per_colour, 256, 0, s>>>(tree, seeds_rc, wt, (uint32_t)w, sum, box, n_colours, out, TreeStack{});
  return hipGetLastError();
}

hipError_t lake_stats_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                            const TreeRec *forest, const uint32_t *stacked_rc, size_t n_colours, uint32_t levels, const u64c *ws,
                            const uint32_t *order, const LakeWeights &wt, const TreeStack &st, int w, void *acc, LakeRec *out) {
  if (n_colours == 0 || st.g == 0) return hipSuccess;
  const size_t n = (size_t)st.g * st.plane, n_acc = n_colours + st.g;      // every slice's record 0 behind the forest's colours
  // (slices, rows and columns are u32 divisions; a quad must not straddle two slices, a row must not either)
  if (n > 0xFFFFFFFFull || n_acc > 0xFFFFFFFFull || st.plane == 0 || (st.plane & 3u) != 0 || w <= 0 || st.plane % (uint32_t)w != 0 ||
      (reinterpret_cast<uintptr_t>(acc) & 7u) != 0)
    return hipErrorInvalidValue;
  u64c *sum = (u64c *)acc;
  uint32_t *box = (uint32_t *)(sum + 6 * n_acc);
  const unsigned per_entry = (unsigned)((n_acc + 255) / 256);
  k_lake_init<<<per_entry, 256, 0, s>>>(sum, box, n_acc);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  {      // the grid of tree_own_counts_stack
    const size_t quads = (n + 1023) / 1024;
    const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
    const unsigned grid = (unsigned)((quads + steps - 1) / steps);
    if (wt.u16) k_lake_own<uint16_t, true><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_acc, n, steps, st);
    else k_lake_own<uint8_t, true><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_acc, n, steps, st);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_colours > 1) {      // ONE launch per level for the whole stack: parents are the forest's, the planes are n_acc long
    const u64c *off = ws + NLEVELS + 1;
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
    for (uint32_t l = 1; l < levels; ++l) {
      k_lake_fold<<<grid, 256, 0, s>>>(forest, sum, box, n_acc, order, off + l);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  if (wt.u16) k_lake_write<uint16_t, true><<<per_entry, 256, 0, s>>>(forest, stacked_rc, wt, (uint32_t)w, sum, box, n_acc, out, st);
  else k_lake_write<uint8_t, true><<<per_entry, 256, 0, s>>>(forest, stacked_rc, wt, (uint32_t)w, sum, box, n_acc, out, st);
  return hipGetLastError();
}

// ---- a stack of slices (ws_transform_to_list_batch_device, ws_merge_batch_device) --------------------------------------------
//
// The slices of a cube flooded as ONE plane of g x slice_h rows (ws_segment.hip, segment_batch_stacked): labels restart at 1 in
// every slice, colour c of slice k is c + base[k] in the stack's numbering (base: g + 1 words, base[g] = the stack's colours).

// slice of a stack colour (1 .. base[g]): the k with base[k] < c <= base[k + 1] (a seedless slice has base[k] == base[k + 1])
__device__ __forceinline__ uint32_t slice_of_colour(const uint32_t *base, uint32_t g, uint32_t c) {
  uint32_t lo = 0, hi = g - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (base[mid] < c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// level of record i: the l in [lo, hi] with off[l] <= i < off[l + 1] (off: prefix sums of the levels' record counts)
__device__ __forceinline__ uint32_t level_of_record(const u64c *__restrict__ off, uint32_t lo, uint32_t hi, u64c i) {
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Per (slice, level): pixels that arrive (their stamp's level), hist[k * NLEVELS + level].  Workgroup (x, k) walks a part of
// slice k, counts in LDS and adds once per level it saw.
__global__ __launch_bounds__(256) void k_slice_arrivals(const uint32_t *__restrict__ keys, size_t plane, u64c *hist) {
  __shared__ uint32_t s_h[NLEVELS];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  const size_t k = blockIdx.y, nv = plane / 4;      // plane % 4 == 0 (stacks have plane % 128 == 0)
  const u32x4_m *kv = reinterpret_cast<const u32x4_m *>(keys + k * plane);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
    const u32x4_m v = kv[i];
    if (v.x != KEY_INF) atomicAdd(&s_h[v.x >> 24], 1u);
    if (v.y != KEY_INF) atomicAdd(&s_h[v.y >> 24], 1u);
    if (v.z != KEY_INF) atomicAdd(&s_h[v.z >> 24], 1u);
    if (v.w != KEY_INF) atomicAdd(&s_h[v.w >> 24], 1u);
  }
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&hist[k * NLEVELS + threadIdx.x], (u64c)s_h[threadIdx.x]);
}

hipError_t slice_arrivals(hipStream_t s, const uint32_t *keys, size_t plane, size_t n_slices, u64c *hist) {
  if (plane == 0 || n_slices == 0) return hipSuccess;
  const unsigned bx = (unsigned)std::min<size_t>(std::max<size_t>(plane / (4 * 256 * 16), 1), 256);      // ~16 words a thread
  k_slice_arrivals<<<dim3(bx, (unsigned)n_slices), 256, 0, s>>>(keys, plane, hist);
  return hipGetLastError();
}

// The forest's tree records (ws_merge_tree_batch_device) into the caller's slice-major layout in the slices' own colours: record c
// of the forest (1 .. n_seeds) is record c - base[k] of its slice k, at out[c + k] (every slice before it owns one record 0), its
// parent -- same slice: no pair crosses a slice border -- less the slice's base.  Thread n_seeds + k writes slice k's record 0 at
// out[base[k] + k]: the pixels of its plane that no level up to the last coloured (hist: k_slice_arrivals').
__global__ __launch_bounds__(256) void k_tree_unstack(const TreeRec *__restrict__ forest, size_t n_seeds, const uint32_t *__restrict__ base, uint32_t g,
                                                      const u64c *__restrict__ hist, uint32_t levels, uint32_t plane, TreeRec *out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_seeds) {
    const uint32_t c = (uint32_t)i + 1u, k = slice_of_colour(base, g, c);
    TreeRec r = forest[c];
    if (r.death_level != TREE_ALIVE) r.parent -= base[k];
    out[(size_t)c + k] = r;
  } else if (i < n_seeds + g) {
    const uint32_t k = (uint32_t)(i - n_seeds);
    u64c arrived = 0;
    for (uint32_t l = 0; l < levels; ++l) arrived += hist[(size_t)k * NLEVELS + l];
    out[(size_t)base[k] + k] = TreeRec{0u, TREE_ALIVE, (uint32_t)((u64c)plane - arrived), 0u};
  }
}

hipError_t tree_unstack(hipStream_t s, const TreeRec *forest, size_t n_seeds, const uint32_t *base, size_t g, const u64c *hist, uint32_t levels,
                        size_t plane, TreeRec *out) {
  if (g == 0) return hipSuccess;
  if (levels > (uint32_t)NLEVELS || plane > 0xFFFFFFFFull || g > 0xFFFFFFFFull) return hipErrorInvalidValue;
  k_tree_unstack<<<(unsigned)((n_seeds + g + 255) / 256), 256, 0, s>>>(forest, n_seeds, base, (uint32_t)g, hist, levels, (uint32_t)plane, out);
  return hipGetLastError();
}

// The stack's records (level-major, stack colours) into the caller's slice-major layout.  A workgroup takes SPLIT_CHUNK
// consecutive records; they span the levels l_lo .. l_hi (one, mostly), so its bins are (l - l_lo, slice) -- counted in LDS and
// sent on with ONE atomic per (workgroup, bin).  A chunk with more bins than LDS holds (many tiny slices) adds record by record.
// The slices' colour bases sit in LDS for the binary search of a record's slice (up to SPLIT_LDS_BASE of them).
//   SCATTER false: bins[k * levels + l] += count.   true: bins are cursors (the caller's offsets of the bins); every record is
//   written behind its bin's cursor as (colour - base[k], area).
constexpr int SPLIT_PER_THREAD = 16;
constexpr int SPLIT_CHUNK = 256 * SPLIT_PER_THREAD;
constexpr uint32_t SPLIT_LDS_BINS = 2048, SPLIT_LDS_BASE = 2048;
typedef unsigned long long u64x2_m __attribute__((ext_vector_type(2)));
template <bool SCATTER>
__global__ __launch_bounds__(256) void k_split_records(const uint64_t *__restrict__ rec, size_t n_rec, const u64c *__restrict__ off,
                                                       uint32_t levels, const uint32_t *__restrict__ base, uint32_t g, u64c *bins,
                                                       uint64_t *out) {
  __shared__ uint32_t s_cnt[SPLIT_LDS_BINS];
  __shared__ uint32_t s_base[SPLIT_LDS_BASE];
  __shared__ u64c s_pos[SCATTER ? SPLIT_LDS_BINS : 1];
  const bool lds_base = g <= SPLIT_LDS_BASE;
  if (lds_base)
    for (uint32_t k = threadIdx.x; k < g; k += 256) s_base[k] = base[k];
  const uint32_t *bs = lds_base ? s_base : base;
  const size_t r0 = (size_t)blockIdx.x * SPLIT_CHUNK;
  const size_t r1 = min(r0 + (size_t)SPLIT_CHUNK, n_rec);
  const uint32_t l_lo = level_of_record(off, 0, levels - 1, r0), l_hi = level_of_record(off, l_lo, levels - 1, r1 - 1);
  const uint32_t nb = (l_hi - l_lo + 1) * g;
  const bool lds = nb <= SPLIT_LDS_BINS;      // workgroup uniform
  __syncthreads();
  const u64x2_m *rv = reinterpret_cast<const u64x2_m *>(rec);
  uint32_t bin[SPLIT_PER_THREAD];
  u64x2_m r[SPLIT_PER_THREAD];
#pragma unroll
  for (int j = 0; j < SPLIT_PER_THREAD; ++j) {
    const size_t i = r0 + (size_t)j * 256 + threadIdx.x;
    bin[j] = 0xFFFFFFFFu;
    if (i < r1) {
      r[j] = rv[i];
      const uint32_t c = (uint32_t)r[j].x;
      const uint32_t k = slice_of_colour(bs, g, c), l = level_of_record(off, l_lo, l_hi, i);
      r[j].x = c - bs[k];
      bin[j] = lds ? (l - l_lo) * g + k : k * levels + l;
    }
  }
  if (!lds) {
#pragma unroll
    for (int j = 0; j < SPLIT_PER_THREAD; ++j) {
      if (bin[j] == 0xFFFFFFFFu) continue;
      const u64c p = atomicAdd(&bins[bin[j]], 1ull);
      if (SCATTER) { out[2 * p] = r[j].x; out[2 * p + 1] = r[j].y; }      // (the caller's records need only be 8-byte aligned)
    }
    return;
  }
  for (uint32_t b = threadIdx.x; b < nb; b += 256) s_cnt[b] = 0;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SPLIT_PER_THREAD; ++j)
    if (bin[j] != 0xFFFFFFFFu) atomicAdd(&s_cnt[bin[j]], 1u);
  __syncthreads();
  for (uint32_t b = threadIdx.x; b < nb; b += 256) {
    const uint32_t n = s_cnt[b];
    const uint32_t k = b % g, l = l_lo + b / g;
    if (!SCATTER) {
      if (n) atomicAdd(&bins[(size_t)k * levels + l], (u64c)n);
    } else {
      s_pos[b] = n ? atomicAdd(&bins[(size_t)k * levels + l], (u64c)n) : 0ull;
      s_cnt[b] = 0;
    }
  }
  if (!SCATTER) return;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < SPLIT_PER_THREAD; ++j) {
    if (bin[j] == 0xFFFFFFFFu) continue;
    const u64c p = s_pos[bin[j]] + atomicAdd(&s_cnt[bin[j]], 1u);
    out[2 * p] = r[j].x;
    out[2 * p + 1] = r[j].y;
  }
}

hipError_t split_records(hipStream_t s, bool scatter, const uint64_t *rec, size_t n_rec, const u64c *off, uint32_t levels,
                         const uint32_t *base, uint32_t g, u64c *bins, uint64_t *out) {
  if (n_rec == 0) return hipSuccess;
  const unsigned blocks = (unsigned)((n_rec + SPLIT_CHUNK - 1) / SPLIT_CHUNK);
  if (scatter) k_split_records<true><<<blocks, 256, 0, s>>>(rec, n_rec, off, levels, base, g, bins, out);
  else k_split_records<false><<<blocks, 256, 0, s>>>(rec, n_rec, off, levels, base, g, bins, nullptr);
  return hipGetLastError();
}

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
  const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 16384);
  k_union_stack<<<blocks, 256, 0, s>>>(labels, slice_h, w, n, base, parent);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const int fb = (int)std::min<size_t>((n_colours + 255) / 256, 8192);
  k_uf_flatten<<<fb > 0 ? fb : 1, 256, 0, s>>>(parent, n_colours);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  k_relabel_stack<<<blocks, 256, 0, s>>>(labels, (size_t)slice_h * w, n, base, parent);
  return hipGetLastError();
}

}  // namespace wsk
