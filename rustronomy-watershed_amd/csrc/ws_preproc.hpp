// ws_preproc.hpp -- launch wrapper of the pre-processor kernels (ws_preproc.hip).
#pragma once

#include <hip/hip_runtime.h>
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

}  // namespace wsk
