// ws_lake_part.hpp -- the per-pixel fold of the lake statistics as the kernels of ws_merge_tree.hip and
// ws_tree_cut.hip share it: a LakePart is what one pixel, one lane, one wave or one table slot holds of a record (five u64 sums,
// the packed peak, the box and the smallest weight), lake_join is the fold, and the accumulators are planes of n entries
// (sum: w, wr, wc, r, c, peak; box: r_min, r_max, c_min, c_max, w_min) in LDS or in memory.  Device code only; a kernel file
// includes it after ws_uf.hpp.
#pragma once

#include "ws_uf.hpp"

namespace wsk {

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

static __global__ __launch_bounds__(256) void k_lake_init(u64c *sum, uint32_t *box, size_t n) {
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

}  // namespace wsk
