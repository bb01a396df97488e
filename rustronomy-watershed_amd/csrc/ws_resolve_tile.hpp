// ws_resolve_tile.hpp -- the constants of the two-launch label resolve (ws_resolve.hip: REF_*, RL_*, CH_*, WS_REF_DENSE),
// the phase-stamp hooks of its diagnostic build, and follow_chain.
//
// The phases of k_resolve_local and k_resolve_chase are not here: they are numbered sections of the kernel bodies, because
// every cut into functions changed the compiled kernels (profiles/resolve_kernel_resources.txt lists each attempt).
#pragma once

#include "ws_common.hpp"

// per-workgroup phase stamps: only in the diagnostic builds under tools/ (they define the macros before this header)
#ifndef WS_STAMP
#define WS_STAMP(slot) do {} while (0)
#define WS_STAMP_VALUE(slot, v) do {} while (0)
#endif

namespace wsk {

constexpr uint32_t REF_BIT = 0x80000000u;
constexpr size_t REF_REGION = 64 * 16;          // work-list entries per wave of k_resolve_local: its pixels
constexpr uint32_t REF_ALL = 0xFFFFFFFFu;       // count word of a wave with REF_DENSE references or more: no list (see k_resolve_local, phase 7)
#ifndef WS_REF_DENSE
#define WS_REF_DENSE 256
#endif
constexpr uint32_t REF_DENSE = WS_REF_DENSE;

typedef uint32_t u32x4_r __attribute__((ext_vector_type(4)));

// Layout: thread t owns the 4 x 4 patch (t & 15, t >> 4) of the 64 x 64 tile, stamps / colours /
// pointers in registers; global accesses are 16 B per lane and row.  The LDS tile has pitch RL_P = 72
// and the patch grid starts at column 4, so that patch rows are 16-byte aligned (ds_*_b128); the halo
// ring sits at rows 0 / 65 and columns 3 / 68.
constexpr int RL_P = 72, RL_X0 = 4, RL_ROWS = TS + 2;
constexpr uint32_t RL_FINAL = 0x8000u;          // pointer flag: the target is a root of the in-tile forest
constexpr uint32_t RL_HALO = 0x4000u;           // pointer flag: ... namely a halo cell, where the chain leaves the tile
static_assert(RL_ROWS * RL_P <= (int)RL_HALO, "cell indices must stay below the flag bits");

// MERGE: tile_min[tile] of a tile that is one lake whose every pixel's chain leaves the tile (see k_resolve_local)
constexpr uint32_t RL_TILE_UNDECIDED = 0xFFFFFFFFu;

// k_resolve_chase: regions per wave and entries per lane in flight (see there)
constexpr int CH_R = 4, CH_U = 4;

#ifdef __HIPCC__

// Follows the chain that starts with the reference `v` (the label some pixel holds) to its colour -- or to the first
// reference that leads out of [follow_from, follow_from + span).  COMPRESS (planes whose chains cross many tiles: smooth
// maps): a chain of more than two hops that ended in a colour is walked a second time and every pixel on it is given that
// colour -- its own final label, so a plain store that no owner's store can contradict -- and whoever comes by later stops
// there.  (Path halving by compare-and-swap was measured first: the chains are shared by thousands of waves, the swaps hit
// the same addresses, and same-address atomics retire at ~25 M/s: the chase took twice as long, 0.43 -> 0.77 ms.)
template <bool COMPRESS>
__device__ __forceinline__ uint32_t follow_chain(uint32_t *labels, uint32_t v, size_t follow_from, size_t span, size_t n) {
  const uint32_t start = v;
  size_t hops = 1;
  for (; (v & REF_BIT) && (size_t)(v & ~REF_BIT) - follow_from < span && hops < n; ++hops)
    v = __hip_atomic_load(labels + (v & ~REF_BIT), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (COMPRESS && hops > 3 && !(v & REF_BIT)) {
    uint32_t w = start;
    for (size_t k = 1; k < hops && (w & REF_BIT) && (size_t)(w & ~REF_BIT) - follow_from < span; ++k) {
      const uint32_t q = w & ~REF_BIT;
      w = __hip_atomic_load(labels + q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (w & REF_BIT) __hip_atomic_store(labels + q, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  return v;
}

#endif      // __HIPCC__

}  // namespace wsk
