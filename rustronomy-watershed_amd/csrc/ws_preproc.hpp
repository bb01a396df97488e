// ws_preproc.hpp -- launch wrappers of the pre-processor kernels (ws_preproc.hip: one flat span; ws_cube_input.hip: a cube
// normalised slice by slice) and the arithmetic both share.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

namespace wsk {

constexpr int PREPROC_BLOCKS = 4096;          // partial (min, max) pairs: scratch = 2 * PREPROC_BLOCKS doubles

size_t preproc_elem_size(int dtype);          // 0 for an unknown dtype
// dtype: ws_dtype of include/ws_hip.h.  The zero-seeded folds (lib.rs:1147-1156): scratch[0..1] hold (min, max) afterwards
// (n == 0: nothing runs, scratch is not written).
hipError_t preprocess_minmax(hipStream_t s, const void *data, int dtype, size_t n, double *scratch);
// The quantiser (lib.rs:1159-1172) with the (min, max) of scratch[0..1]; max - min must be finite (or no element normal).
hipError_t preprocess_quantise(hipStream_t s, const void *data, int dtype, size_t n, uint8_t maxv, const double *scratch, uint8_t *out);

#if defined(__HIPCC__)
template <typename T>
__device__ __forceinline__ double to_f64(T v) { return (double)v; }

__device__ __forceinline__ bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }   // false for NaN, +-inf

// One element of the quantiser (lib.rs:1159-1172), the only copy of this expression: mn and range = max - min as the folds left them
__device__ __forceinline__ uint8_t quantise_one(double v, double mn, double range, double maxv) {
  const double a = fabs(v);
  if (a >= 2.2250738585072014e-308 && a <= 1.7976931348623157e308) {      // f64::is_normal
    const double normal = (v - mn) / range;                               // lib.rs:1163
    return (uint8_t)(normal * maxv);                                      // lib.rs:1164: to_u8 truncates; in [0, MAX] while `range` is finite
  }
  if (v == INFINITY) return 0;                                            // lib.rs:1165-1167
  return 255;                                                             // lib.rs:1168-1170
}
#endif

// ---- a cube normalised slice by slice (ws_cube_input.hip) ------------------------------------------------------------------------
// Element (k, r, c) of the view sits at data + k * ss + r * rs + c * cs (ELEMENTS).  `scratch` holds cube_minmax_doubles(...)
// doubles: the per-(workgroup, slice) partials, then at scratch + cube_minmax_final_at(...) the 2 * n_slices finals (min, max).
struct CubeView { size_t n_slices, h, w, ss, rs, cs; };
size_t cube_minmax_blocks(const CubeView &v);          // partial pairs per slice
inline size_t cube_minmax_final_at(const CubeView &v) { return 2 * v.n_slices * cube_minmax_blocks(v); }
inline size_t cube_minmax_doubles(const CubeView &v) { return cube_minmax_final_at(v) + 2 * v.n_slices; }
// the zero-seeded folds of every slice; bad (nullable): atomicMin of the indices of the slices whose max - min is not finite
hipError_t cube_minmax(hipStream_t s, const void *data, int dtype, const CubeView &v, double *scratch, unsigned long long *bad);
// out: n_slices * h * w bytes, contiguous, slice-major; minmax: the finals of cube_minmax
hipError_t cube_quantise(hipStream_t s, const void *data, int dtype, const CubeView &v, uint8_t maxv, const double *minmax, uint8_t *out);

}  // namespace wsk
