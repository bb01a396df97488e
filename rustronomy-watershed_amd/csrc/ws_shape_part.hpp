// ws_shape_part.hpp -- the per-pixel fold of the lakes' second moments for the k_shape_* kernels of
// ws_merge_tree.hip.  Six exact 128-bit sums a record (v row^2, v col^2, v row col, row^2, col^2, row col), each carried as TWO u64
// limbs that never exchange a carry: a pixel's term t adds t & 0xFFFFFFFF to limb A and t >> 32 to limb B.  A stays below 2^64 for
// fewer than 2^32 pixels, B because the sum stays below 2^96 (check_lake_weights: wmax * pixels * longest side < 2^64, sides <
// 2^32), so every join is twelve plain u64 adds, in a register, in LDS and in memory alike, and the sum is A + (B << 32)
// (shape_normal, once per colour).  The accumulators are twelve planes of n entries (plane 2 k: A of sum k, plane 2 k + 1: B).
// Device code only; a kernel file includes it after ws_lake_part.hpp.
#pragma once

#include "ws_lake_part.hpp"

namespace wsk {

// 100 B a slot (twelve limbs and the key): 25 KB a workgroup.  The kernel's registers allow three workgroups a CU, which 512 slots
// (50 KB) would fit as well; they measured slower, the table being cleared and walked more often than it is full (DESIGN.md
// section 4.3.2)
constexpr int SHAPE_SLOTS = 256, SHAPE_PROBES = 4, SHAPE_LIMBS = 12;

struct ShapePart {
  u64c a[SHAPE_LIMBS];
};

__device__ __forceinline__ ShapePart shape_none() { return ShapePart{{0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}}; }

// v < 2^16 and y, x < 2^32: a weighted term reaches 2^80, its B limb 2^48
__device__ __forceinline__ ShapePart shape_pixel(uint32_t v, uint32_t y, uint32_t x) {
  const u64c rr = (u64c)y * y, cc = (u64c)x * x, rc = (u64c)y * x;
  const unsigned __int128 wrr = (unsigned __int128)rr * v, wcc = (unsigned __int128)cc * v, wrc = (unsigned __int128)rc * v;
  return ShapePart{{(u64c)wrr & 0xFFFFFFFFull, (u64c)(wrr >> 32), (u64c)wcc & 0xFFFFFFFFull, (u64c)(wcc >> 32),
                    (u64c)wrc & 0xFFFFFFFFull, (u64c)(wrc >> 32), rr & 0xFFFFFFFFull, rr >> 32, cc & 0xFFFFFFFFull, cc >> 32,
                    rc & 0xFFFFFFFFull, rc >> 32}};
}

__device__ __forceinline__ void shape_join(ShapePart &a, const ShapePart &b) {
#pragma unroll
  for (int k = 0; k < SHAPE_LIMBS; ++k) a.a[k] += b.a[k];
}

// The join over the wave, in every lane.  FLAT (both sides of the plane below 65 536): the B limbs of the three plain sums are 0 in
// every lane and are not moved -- nine 64-bit exchanges a step, not twelve.
template <bool FLAT>
__device__ __forceinline__ ShapePart shape_wave_total(ShapePart a) {
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int k = 0; k < SHAPE_LIMBS; ++k)
      if (!(FLAT && k >= 6 && (k & 1))) a.a[k] += __shfl_xor(a.a[k], o, 64);
  }
  return a;
}

// entry i of accumulator planes of n entries each (LDS table or memory) takes a part: one atomic a limb, none for a limb of 0
__device__ __forceinline__ void shape_apply(u64c *acc, size_t n, size_t i, const ShapePart &a) {
#pragma unroll
  for (int k = 0; k < SHAPE_LIMBS; ++k)
    if (a.a[k]) atomicAdd(&acc[(size_t)k * n + i], a.a[k]);
}

__device__ __forceinline__ ShapePart shape_load(const u64c *acc, size_t n, size_t i) {
  ShapePart a;
#pragma unroll
  for (int k = 0; k < SHAPE_LIMBS; ++k) a.a[k] = acc[(size_t)k * n + i];
  return a;
}

__device__ __forceinline__ void shape_store(u64c *acc, size_t n, size_t i, const ShapePart &a) {
#pragma unroll
  for (int k = 0; k < SHAPE_LIMBS; ++k) acc[(size_t)k * n + i] = a.a[k];
}

// sum k of a part as (low, high) 64 bits: A + (B << 32)
__device__ __forceinline__ void shape_normal(const ShapePart &a, int k, u64c *lo, u64c *hi) {
  const u64c A = a.a[2 * k], B = a.a[2 * k + 1], l = A + (B << 32);
  *lo = l;
  *hi = (B >> 32) + (l < A ? 1ull : 0ull);
}

// a root's part into the workgroup's table; a root that finds no slot within SHAPE_PROBES updates memory itself: exact either way
__device__ __forceinline__ void shape_add(uint32_t *s_key, u64c *s_acc, uint32_t *s_used, u64c *acc, size_t n_colours, uint32_t r, const ShapePart &a) {
  const uint32_t h0 = (r * 2654435761u) >> 24;      // 8 bits
  for (int j = 0; j < SHAPE_PROBES; ++j) {
    const uint32_t slot = (h0 + (uint32_t)j) & (SHAPE_SLOTS - 1);
    const uint32_t old = atomicCAS(&s_key[slot], LAKE_EMPTY, r);
    if (old == LAKE_EMPTY) atomicAdd(s_used, 1u);
    if (old == LAKE_EMPTY || old == r) { shape_apply(s_acc, SHAPE_SLOTS, slot, a); return; }
  }
  shape_apply(acc, n_colours, r, a);
}

// the table into memory, one visit per root it holds, and empty again (SHAPE_SLOTS == the workgroup's 256 threads: a slot a thread)
__device__ __forceinline__ void shape_flush(uint32_t *s_key, u64c *s_acc, u64c *acc, size_t n_colours) {
  for (int j = threadIdx.x; j < SHAPE_SLOTS; j += 256) {
    if (s_key[j] == LAKE_EMPTY) continue;
    shape_apply(acc, n_colours, s_key[j], shape_load(s_acc, SHAPE_SLOTS, j));
    s_key[j] = LAKE_EMPTY;
    shape_store(s_acc, SHAPE_SLOTS, j, shape_none());
  }
}

}  // namespace wsk
