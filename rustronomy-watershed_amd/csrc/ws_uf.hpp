// ws_uf.hpp -- what the merging kernels' sources (ws_merge.hip, ws_merge_final.hip, ws_merge_tree.hip) share: the lock-free
// union-find over seed colours, the loop over a bucket of edges, a few lane-level helpers and the clamped grid of the wrappers.
// Union-by-min-index: a root only ever gets hooked under a SMALLER index (atomicCAS on the root's own slot) and path
// halving only ever lowers a parent (atomicMin), so every parent chain is monotone and a stale read is still an
// ancestor.  All parent updates are device-scope atomics: XCD L2s are not coherent with each other, and nothing here
// relies on a plain store being seen inside a launch.
#pragma once

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

// what a union did: the node that lost its root status and the smaller root it went under (lost == 0xFFFFFFFF: nothing, one set already)
struct Hooked { uint32_t lost, under; };

__device__ __forceinline__ Hooked uf_union(uint32_t *parent, uint32_t a, uint32_t b) {
  for (;;) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) return Hooked{0xFFFFFFFFu, 0u};
    if (a > b) { const uint32_t t = a; a = b; b = t; }
    const uint32_t old = atomicCAS(parent + b, b, a);     // b is a root only while parent[b] == b
    if (old == b) return Hooked{b, a};
    b = old;                                              // someone hooked b first: continue from there
  }
}

// The unions of n edges, strided over the nblocks workgroups of a launch that take part (bid: this one's index among them);
// on_hook(Hooked) runs once per colour: only the CAS that ends its time as a root gets there.
template <typename OnHook>
__device__ __forceinline__ void union_range(const uint2 *__restrict__ edges, size_t n, uint32_t *parent, unsigned bid, unsigned nblocks, OnHook on_hook) {
  const size_t step = (size_t)nblocks * blockDim.x;
  for (size_t i = (size_t)bid * blockDim.x + threadIdx.x; i < n; i += step) {
    const uint2 e = edges[i];
    const Hooked h = uf_union(parent, e.x, e.y);
    if (h.lost != 0xFFFFFFFFu) on_hook(h);
  }
}

// find_merge only sees pairs around a 3x3 window centre (lib.rs:411-434): one pixel of a pair must be interior
__device__ __forceinline__ bool interior(int y, int x, int H, int W) {
  return y >= 1 && y < H - 1 && x >= 1 && x < W - 1;
}

typedef uint32_t u32x4_m __attribute__((ext_vector_type(4)));      // four pixels of a row as one 16-byte load or store
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {      // total of v over the wave, in every lane
  for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
  return v;
}

// A stack of slices flooded as one plane: colour c of slice k is c + base[k] in the stack's numbering (base: g + 1 words).
// slice of a stack colour (1 .. base[g]): the k with base[k] < c <= base[k + 1] (a seedless slice has base[k] == base[k + 1])
__device__ __forceinline__ uint32_t slice_of_colour(const uint32_t *base, uint32_t g, uint32_t c) {
  uint32_t lo = 0, hi = g - 1;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1) >> 1;
    if (base[mid] < c) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Lake records of one level are contiguous: a record's position is the number of records of the earlier levels plus a
// ticket from its own level's counter.  This is the first term, *s_base = the sum of level_counts[0 .. level), which the
// first wave of every workgroup adds up (earlier launches finished those counters; lane: threadIdx.x & 63); read it behind a barrier.
__device__ __forceinline__ void records_before(const u64c *level_counts, uint32_t level, int lane, u64c *s_base) {
  if (threadIdx.x < 64) {
    u64c before = 0;
    for (uint32_t j = (uint32_t)lane; j < level; j += 64) before += level_counts[j];
    for (int o = 32; o > 0; o >>= 1) before += __shfl_xor(before, o, 64);
    if (lane == 0) *s_base = before;
  }
}

// workgroups for n items at per_block items each, at most cap of them (the kernels stride over what is left)
inline unsigned clamped_grid(size_t n, size_t per_block, size_t cap) {
  return (unsigned)std::min<size_t>((n + per_block - 1) / per_block, cap);
}

}  // namespace wsk
