// ws_merge.hip -- gfx950 kernels of the merging transform's level loop (see ws_merge.hpp for the maths): the level buckets,
// what a LevelStep (ws_level_plan.hpp) launches -- unions, areas, lake records, the live-lake list, the stamped unions -- the
// per-level relabel, and the two kernels that sort a stack's arrivals and records by slice.  The union-find is ws_uf.hpp's;
// the final-labels-only path is ws_merge_final.hip, everything that reads the stamped forest ws_merge_tree.hip.
#include "ws_common.hpp"
#include "ws_uf.hpp"

namespace wsk {

__global__ void k_uf_init(uint32_t *parent, uint32_t *size, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (; i < n; i += step) { parent[i] = (uint32_t)i; size[i] = 0u; }
}

hipError_t uf_init(hipStream_t s, uint32_t *parent, uint32_t *size, size_t n) {
  if (n == 0) return hipSuccess;
  k_uf_init<<<clamped_grid(n, 1024, 8192), 256, 0, s>>>(parent, size, n);
  return hipGetLastError();
}

// ---- the level buckets: edge / pixel enumeration shared by the histogram and the scatter ------

constexpr int MSEG = 1024;   // pixels per workgroup: one row segment, 4 per thread

struct PixelItems {
  // up to 4 pixels of one row segment and their right / down crossings
  uint32_t px_lvl[4], px_col[4];      // level 0xFFFFFFFF = no item
  uint32_t er_lvl[4], ed_lvl[4];
  uint2 er[4], ed[4];
};

// Loads first, unconditional and on clamped addresses (a load under a data-dependent branch is waited for before the next is
// issued: 24 dependent round trips per thread in the first form of this function), predicates afterwards.  With W % 4 == 0 and
// planes on 16-byte alignment the four pixels and the four below them are 16-byte loads.
// STACK: H rows of slices of slice_h rows each (ws_transform_to_list_batch_device): "interior" and the pixel below are taken
// within the row's slice -- no pair crosses a slice border -- and colours become colour + base[slice], one numbering for the stack
template <bool STACK>
__device__ __forceinline__ void gather_items(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                             int H, int W, int y, int x0, PixelItems &it, int slice_h,
                                             const uint32_t *__restrict__ base) {
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
  union_range(edges, n, parent, blockIdx.x, nblocks, [=](Hooked h) {
    if (hooked) hooked[atomicAdd(hooked_count, 1u)] = h.lost;
    if (death) death[h.lost] = level;
  });
}

__global__ void k_union_edges(const uint2 *__restrict__ edges, size_t n, uint32_t *parent, uint32_t *hooked,
                              uint32_t *hooked_count, const u64c *__restrict__ range) {
  union_body(edges, n, parent, hooked, hooked_count, range, nullptr, 0u, gridDim.x);
}

hipError_t union_edges(hipStream_t s, const uint2 *edges, size_t n, uint32_t *parent, uint32_t *hooked, uint32_t *hooked_count) {
  if (n == 0) return hipSuccess;
  k_union_edges<<<clamped_grid(n, 256, 4096), 256, 0, s>>>(edges, n, parent, hooked, hooked_count, nullptr);
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
// range: {first, end} of the level's arriving pixels in px_items; split: 0 when there is no hooked list (nothing to fold)
__global__ void k_fold_and_add(const uint32_t *__restrict__ hooked, const uint32_t *__restrict__ hooked_count,
                               const uint32_t *__restrict__ px_items, uint32_t *parent, uint32_t *size,
                               const u64c *__restrict__ range, int split) {
  px_items += range[0];
  const size_t n = (size_t)(range[1] - range[0]);
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

hipError_t fold_and_add_ranged(hipStream_t s, const uint32_t *hooked, const uint32_t *hooked_count, const uint32_t *px_items,
                               const u64c *range, unsigned grid, uint32_t *parent, uint32_t *size) {
  k_fold_and_add<<<hooked ? 2 * grid : grid, 256, 0, s>>>(hooked, hooked_count, px_items, parent, size, range, hooked ? 1 : 0);
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
  records_before(level_counts, level, lane, &s_base);
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
  k_sd_init<<<clamped_grid(n, 1024, 8192), 256, 0, s>>>(sd, n);
  return hipGetLastError();
}

// level L's records (and live list) from level L - 1's live list.  bid / nblocks: this job's share of the launch.
__device__ __forceinline__ void emit_alive_body(const uint2 *__restrict__ sd, size_t n_colours, const uint32_t *__restrict__ alive_in,
                                                uint32_t *alive_out, uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t L,
                                                unsigned bid, unsigned nblocks) {
  __shared__ u64c s_base, s_first;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  records_before(level_counts, L, lane, &s_base);
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
    union_range(edge_items + range[0], (size_t)(range[1] - range[0]), parent, blockIdx.x, union_blocks, [=](Hooked h) {
      hooked[atomicAdd(hooked_count, 1u)] = h.lost;
      sd[h.lost].y = level;
    });
  } else if (level > 0) {
    emit_alive_body(sd, n_colours, alive_in, alive_out, lakes, cap, level_counts, level - 1, blockIdx.x - union_blocks, gridDim.x - union_blocks);
  }
}

__global__ __launch_bounds__(256) void k_emit_alive(const uint2 *__restrict__ sd, size_t n_colours, const uint32_t *__restrict__ alive_in,
                                                    uint32_t *alive_out, uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t L) {
  emit_alive_body(sd, n_colours, alive_in, alive_out, lakes, cap, level_counts, L, blockIdx.x, gridDim.x);
}

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

// ---- the plane of one level (the hook's): out[p] = coloured by `level` ? root(labels[p]) : 0 ----------------------------------
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

template <typename OutT>
static hipError_t relabel(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *parent, OutT *out, size_t n, uint32_t level) {
  if (n == 0) return hipSuccess;
  k_relabel<OutT><<<clamped_grid(n, 1024, 8192), 256, 0, s>>>(keys, labels, parent, out, n, level);
  return hipGetLastError();
}

hipError_t relabel_u32(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *parent, uint32_t *out, size_t n, uint32_t level) {
  return relabel(s, keys, labels, parent, out, n, level);
}
hipError_t relabel_u64(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *parent, uint64_t *out, size_t n, uint32_t level) {
  return relabel(s, keys, labels, parent, out, n, level);
}

// ---- the stamped unions of transform_history (ws_transform_history_device; its readers: ws_merge_tree.hip) -------------------------
//
// The per-level unions leave a level-stamped merge forest beside the union-find: when a CAS hooks root b under a, hook[b] = a
// and death[b] = the level.  parent[] cannot serve: path halving rewrites it in later levels.  The lake of colour c at level L
// is then found by walking hook[] from c while death[x] <= L (DESIGN.md section 4.1 has the argument that the walk ends at the
// lake's smallest colour, the canonical id, whatever order the racing CASes took).

__global__ __launch_bounds__(256) void k_union_stamped(const uint2 *__restrict__ edge_items, const u64c *__restrict__ range, uint32_t *parent,
                                                       uint32_t *death, uint32_t *hook, uint32_t level) {
  union_range(edge_items + range[0], (size_t)(range[1] - range[0]), parent, blockIdx.x, gridDim.x, [=](Hooked h) {
    hook[h.lost] = h.under;
    death[h.lost] = level;
  });
}

hipError_t union_stamped_ranged(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned grid, uint32_t *parent, uint32_t *death,
                                uint32_t *hook, uint32_t level) {
  k_union_stamped<<<grid, 256, 0, s>>>(edge_items, range, parent, death, hook, level);
  return hipGetLastError();
}

// ---- a stack of slices flooded as ONE plane (ws_transform_to_list_batch_device; ws_batch.hip, run_batch) ---------------------

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
  // gridDim.y holds at most GRID_Y_MAX slices: a stack of more (thumbnails: stackable() groups up to 2^24 of them) goes in runs
  for (size_t k0 = 0; k0 < n_slices; k0 += GRID_Y_MAX) {
    const size_t run = std::min<size_t>(n_slices - k0, GRID_Y_MAX);
    k_slice_arrivals<<<dim3(bx, (unsigned)run), 256, 0, s>>>(keys + k0 * plane, plane, hist + k0 * NLEVELS);
  }
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

}  // namespace wsk
