// ws_relax_patch.hpp -- the register patch of the relaxation kernels (ws_relax.hip) and what is done to it, once.
//
// A lane owns PH rows x RX_P columns of pixels in registers: PH = RX_P (k_relax) or RX0_PH (the 256 x 64 kernels,
// k_relax0_tall and k_relax_strips_tall).  Everything here is templated on PH and nothing else differs between the
// kernels; tools/microbench_valu.hip times these very functions.
#pragma once

#include "ws_common.hpp"
#include "ws_relax_plan.hpp"      // RX_P, RX0_PH

namespace wsk {

typedef uint32_t u32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint32_t lane_left(uint32_t old, uint32_t v) {     // lane i <- lane i-1, lane 0 keeps old
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xF, 0xF, false);
}
__device__ __forceinline__ uint32_t lane_right(uint32_t old, uint32_t v) {    // lane i <- lane i+1, lane 63 keeps old
  return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x130, 0xF, 0xF, false);
}

// one pixel: key <- min(key, max(base, 1 + min4)).  The kernels keep b <= t for every pixel (pixels
// that can never change -- seeds, the image border, halo copies -- carry b = t), and under b <= t
// min(t, max(b, x)) is the median of (b, x, t): v_min_u32, v_min3_u32, v_add_u32, v_med3_u32.
__device__ __forceinline__ uint32_t med3u(uint32_t a, uint32_t b, uint32_t c) {
  return max(min(a, b), min(max(a, b), c));
}
template <bool TRACK>
__device__ __forceinline__ void relax_px(uint32_t &t, uint32_t b, uint32_t u, uint32_t d, uint32_t l, uint32_t r, bool &changed) {
  const uint32_t n = med3u(b, min(min(u, d), min(l, r)) + 1u, t);
  if (TRACK) changed |= n != t;      // v_cmp + a scalar OR: the flag lives in an SGPR pair
  t = n;
}

typedef uint32_t patch_t[RX_P][RX_P];

// The image bytes of a patch (one dword per row) -> the pixels' bases: (level << 24) | 1, or KEY_INF for a level that never
// opens.  With the default maximum level, 254 (lib.rs:942), only byte 255 never opens, and (255 << 24) | 1 lies ABOVE every
// stamp: the `b = min(b, t)` that follows every load pins such a pixel at its stamp by itself -- no compare, no select, and
// the byte comes into place with one shift and one and-or (7 cycles per pixel instead of 16.5: these kernels are bound by
// vector issue, profiles/r3_v0_issue_counters.json).  Called AFTER the loop that loads the rows, with its one (kernel
// uniform) branch outside the row loop: a branch between two rows' loads makes every row a memory round trip of its own
// (pass 0: 168 -> 189 us, measured).
template <int PH>
__device__ __forceinline__ void patch_bases(const uint32_t (&iv)[PH], uint32_t (&B)[PH][RX_P], uint32_t max_level) {
  if (max_level == 254u) {
#pragma unroll
    for (int r = 0; r < PH; ++r) {
      B[r][0] = (iv[r] << 24) | 1u;
      B[r][1] = ((iv[r] << 16) & 0xFF000000u) | 1u;
      B[r][2] = ((iv[r] << 8) & 0xFF000000u) | 1u;
      B[r][3] = (iv[r] & 0xFF000000u) | 1u;
    }
  } else {
#pragma unroll
    for (int r = 0; r < PH; ++r)
#pragma unroll
      for (int c = 0; c < RX_P; ++c) {
        const uint32_t v = (iv[r] >> (8 * c)) & 0xFFu;
        B[r][c] = v <= max_level ? ((v << 24) | 1u) : KEY_INF;
      }
  }
}

// A sweep walks the patch rows (or columns) in its direction and, inside a row, the pixels left to right
// (top to bottom), every pixel seeing its neighbours as they are NOW -- Gauss-Seidel all the way.  (Any
// order is a valid relaxation; taking a row's "old" left/right values instead cost 40 register copies
// per round.)  up / dn: the rows above and below the patch; L / R: the columns left and right of it.
template <bool TRACK, bool DOWN, int PH>
__device__ __forceinline__ void sweep_rows(uint32_t (&T)[PH][RX_P], const uint32_t (&B)[PH][RX_P], const uint32_t (&up)[RX_P],
                                           const uint32_t (&dn)[RX_P], const uint32_t (&L)[PH], const uint32_t (&R)[PH], bool &changed) {
#pragma unroll
  for (int k = 0; k < PH; ++k) {
    const int r = DOWN ? k : PH - 1 - k;
#pragma unroll
    for (int c = 0; c < RX_P; ++c)
      relax_px<TRACK>(T[r][c], B[r][c], r == 0 ? up[c] : T[r - 1][c], r == PH - 1 ? dn[c] : T[r + 1][c],
                      c == 0 ? L[r] : T[r][c - 1], c == RX_P - 1 ? R[r] : T[r][c + 1], changed);
  }
}
template <bool TRACK, bool RIGHT, int PH>
__device__ __forceinline__ void sweep_cols(uint32_t (&T)[PH][RX_P], const uint32_t (&B)[PH][RX_P], const uint32_t (&up)[RX_P],
                                           const uint32_t (&dn)[RX_P], const uint32_t (&L)[PH], const uint32_t (&R)[PH], bool &changed) {
#pragma unroll
  for (int k = 0; k < RX_P; ++k) {
    const int c = RIGHT ? k : RX_P - 1 - k;
#pragma unroll
    for (int r = 0; r < PH; ++r)
      relax_px<TRACK>(T[r][c], B[r][c], r == 0 ? up[c] : T[r - 1][c], r == PH - 1 ? dn[c] : T[r + 1][c],
                      c == 0 ? L[r] : T[r][c - 1], c == RX_P - 1 ? R[r] : T[r][c + 1], changed);
  }
}

}  // namespace wsk
