// ws_cube_input.hip -- the front end of the cube pipeline as one call each: pre_processor and find_local_minima of EVERY slice
// of a cube (tests/integration.rs:267-290, 356-380 do both to one slice after the other before any transform).
//
//   ws_pre_processor_batch(_device)       slice k of the output is pre_processor_with_max::<MAX> (lib.rs:1134-1173) of the h x w view
//                                         at data + k * slice_stride: its OWN zero-seeded (min, max), then the quantiser of
//                                         ws_preproc.hpp (quantise_one: the one copy of that expression).  The output is the contiguous
//                                         (n_slices, h, w) u8 cube the stacked batch paths take.
//   ws_find_local_minima_batch(_device)   every slice's find_local_minima (lib.rs:1178-1197) back to back, and the host offsets the
//                                         *_batch_device calls take (kernels: ws_kernels.hip, next to the single plane's).
//
// Pre-processor kernels, three forms chosen on the host (cube_form):
//   channel-last (slice_stride == 1, the layout the reference's tests slice): a wave's lanes are (pixel, slice) pairs, SL = 8, 16, 32
//     or 64 slices (the smallest that holds the cube's) by 64 / SL neighbouring pixels, SLICES FASTEST, so a wave's load covers 64
//     consecutive elements of a dense cube however few slices it has.  The fold keeps one (min, max) per lane.  The quantiser
//     takes a tile of SL slices x 8192 / SL pixels, puts its bytes into LDS as [slice][pixel] (a slice's row padded by 4 bytes to an
//     odd number of dwords: the lanes writing one pixel column hit different banks) and stores with lanes along the PIXEL axis,
//     four bytes a lane: a wave's store writes runs of at least 128 contiguous bytes, whole lines of a slice's plane.
//   row-contiguous (col_stride == 1): lanes along w, as ws_preproc.hip with a slice index.
//   general: a gather, correct for any strides.
// Every grid is one-dimensional (blocks = slices x parts): nothing has to fit gridDim.y.
#include "ws_ctx.hpp"
#include "ws_cube_plan.hpp"

namespace wsk {

constexpr int CL_P = 128;                // pixels of a channel-last tile of 64 slices (fewer slices: 64 / SL times as many): a wave's store runs are whole 128 B lines
constexpr int CL_S = 64;                 // most slices of a tile: one per lane of a wave
static_assert(CL_P % 4 == 0, "packed stores need whole dwords");

enum CubeForm { CUBE_CHANNEL_LAST = 0, CUBE_ROWS = 1, CUBE_GATHER = 2 };
static CubeForm cube_form(const CubeView &v) {
  if (v.ss == 1 && v.n_slices > 1) return CUBE_CHANNEL_LAST;
  return v.cs == 1 ? CUBE_ROWS : CUBE_GATHER;
}

// where pixel p (row-major in its slice) sits, in elements from the slice's first
struct PixMap { size_t w, rs, cs; int dense; };      // dense: rs == w * cs, no division
static PixMap pix_map(const CubeView &v) { return PixMap{v.w, v.rs, v.cs, (v.h <= 1 || v.rs == v.w * v.cs) ? 1 : 0}; }
__device__ __forceinline__ size_t pix_off(const PixMap &m, size_t p) { return m.dense ? p * m.cs : (p / m.w) * m.rs + (p % m.w) * m.cs; }

__device__ __forceinline__ void fold(double v, double &mn, double &mx) {      // lib.rs:1147-1156
  if (finite_f64(v)) { mn = v < mn ? v : mn; mx = v > mx ? v : mx; }
}

// rows / gather: workgroup (slice k, part) folds the pixels part * 256 + t, + B * 256, ... of slice k
template <typename T, bool UNIT>
__global__ __launch_bounds__(256) void k_cube_minmax(const T *__restrict__ data, size_t hw, size_t ss, PixMap m, unsigned B, double *__restrict__ partial) {
  __shared__ double s_min[4], s_max[4];
  const size_t k = blockIdx.x / B;
  const unsigned part = blockIdx.x % B;
  if (UNIT) m.cs = 1;
  const T *base = data + k * ss;
  double mn = 0.0, mx = 0.0;                                 // lib.rs:1149 / 1154: T::zero()
  for (size_t p = (size_t)part * 256 + threadIdx.x; p < hw; p += (size_t)B * 256) fold(to_f64(base[pix_off(m, p)]), mn, mx);
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { s_min[wave] = mn; s_max[wave] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int j = 1; j < 4; ++j) { mn = s_min[j] < mn ? s_min[j] : mn; mx = s_max[j] > mx ? s_max[j] : mx; }
    partial[2 * (size_t)blockIdx.x] = mn;
    partial[2 * (size_t)blockIdx.x + 1] = mx;
  }
}

// channel-last: a wave's 64 lanes are (pixel, slice) pairs, SL slices (8, 16, 32 or 64, chosen on the host: the smallest that holds
// the cube's slices, so a cube of few slices still fills its waves) by PPW = 64 / SL neighbouring pixels -- in a dense cube of SL
// slices 64 consecutive elements.  Workgroup (slice chunk sc, part) folds the pixels (part * 4 + wave) * PPW + lane_p, + B * 4 * PPW, ...
// for the slices sc * SL + lane_s.
template <typename T, int SL>
__global__ __launch_bounds__(256) void k_cube_minmax_cl(const T *__restrict__ data, size_t n_slices, size_t hw, PixMap m, unsigned B,
                                                        double *__restrict__ partial) {
  constexpr int PPW = 64 / SL;
  __shared__ double s_min[4][64], s_max[4][64];
  const size_t sc = blockIdx.x / B;
  const unsigned part = blockIdx.x % B;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lane_s = lane & (SL - 1), lane_p = lane / SL;
  const size_t k = sc * SL + lane_s;
  double mn = 0.0, mx = 0.0;
  if (k < n_slices)
    for (size_t p = ((size_t)part * 4 + wave) * PPW + lane_p; p < hw; p += (size_t)B * 4 * PPW) fold(to_f64(data[pix_off(m, p) + k]), mn, mx);
  s_min[wave][lane] = mn;
  s_max[wave][lane] = mx;
  __syncthreads();
  if (wave == 0 && lane_p == 0 && k < n_slices) {
    for (int j = 0; j < 4; ++j)
      for (int q = 0; q < PPW; ++q) {
        const double a = s_min[j][q * SL + lane_s], b = s_max[j][q * SL + lane_s];
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
      }
    partial[2 * (k * B + part)] = mn;
    partial[2 * (k * B + part) + 1] = mx;
  }
}

// a wave per slice: its B partial pairs -> minmax[2k], [2k + 1]; bad: the lowest slice whose range is not finite (lib.rs:1164 panics)
__global__ __launch_bounds__(256) void k_cube_minmax_final(const double *__restrict__ partial, size_t n_slices, unsigned B, double *__restrict__ minmax,
                                                           unsigned long long *bad) {
  const int lane = threadIdx.x & 63;
  const size_t k = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_slices) return;      // (wave uniform)
  double mn = 0.0, mx = 0.0;
  for (unsigned i = lane; i < B; i += 64) {
    const double a = partial[2 * (k * B + i)], b = partial[2 * (k * B + i) + 1];
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double a = __shfl_down(mn, off, 64), b = __shfl_down(mx, off, 64);
    mn = a < mn ? a : mn;
    mx = b > mx ? b : mx;
  }
  if (lane == 0) {
    minmax[2 * k] = mn;
    minmax[2 * k + 1] = mx;
    if (bad && !finite_f64(mx - mn)) atomicMin(bad, (unsigned long long)k);
  }
}

template <typename T, bool UNIT>
__global__ __launch_bounds__(256) void k_cube_quantise(const T *__restrict__ data, size_t hw, size_t ss, PixMap m, unsigned B,
                                                       const double *__restrict__ minmax, double maxv, uint8_t *__restrict__ out) {
  const size_t k = blockIdx.x / B;
  const unsigned part = blockIdx.x % B;
  if (UNIT) m.cs = 1;
  const T *base = data + k * ss;
  const double mn = minmax[2 * k], range = minmax[2 * k + 1] - minmax[2 * k];
  uint8_t *o = out + k * hw;
  for (size_t p = (size_t)part * 256 + threadIdx.x; p < hw; p += (size_t)B * 256) o[p] = quantise_one(to_f64(base[pix_off(m, p)]), mn, range, maxv);
}

// channel-last: workgroup = tile of SL slices x TP = CL_P * 64 / SL pixels (always 8192 elements); lanes as in the fold on the load side,
// along the pixels (4 bytes a lane) on the store side; packed: out and hw are multiples of 4
template <typename T, int SL>
__global__ __launch_bounds__(256) void k_cube_quantise_cl(const T *__restrict__ data, size_t n_slices, size_t hw, PixMap m, size_t tiles_p,
                                                          const double *__restrict__ minmax, double maxv, uint8_t *__restrict__ out, int packed) {
  constexpr int PPW = 64 / SL, TP = CL_P * PPW, PITCH = TP + 4, DW = TP / 4, ROWS = 256 / DW;
  static_assert((PITCH / 4) % 2 == 1 && DW <= 256, "an odd dword pitch; a pass of the store side covers whole rows");
  __shared__ uint32_t s_tile[SL * PITCH / 4];
  uint8_t *tile8 = reinterpret_cast<uint8_t *>(s_tile);
  const size_t sc = blockIdx.x / tiles_p, p0 = (blockIdx.x % tiles_p) * TP;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lane_s = lane & (SL - 1), lane_p = lane / SL;
  {
    const size_t k = sc * SL + lane_s;
    if (k < n_slices) {
      const double mn = minmax[2 * k], range = minmax[2 * k + 1] - minmax[2 * k];
#pragma unroll 8
      for (int i = wave * PPW + lane_p; i < TP; i += 4 * PPW) {
        const size_t p = p0 + i;
        if (p < hw) tile8[lane_s * PITCH + i] = quantise_one(to_f64(data[pix_off(m, p) + k]), mn, range, maxv);
      }
    }
  }
  __syncthreads();
  const int j = threadIdx.x % DW;                          // dword of the tile's TP pixels
  const size_t px = p0 + 4 * (size_t)j;
  if (px >= hw) return;
  for (int s = threadIdx.x / DW; s < SL; s += ROWS) {      // a wave: runs of at least 128 contiguous bytes of one slice's plane
    const size_t k = sc * SL + s;
    if (k >= n_slices) break;
    const uint32_t word = s_tile[s * (PITCH / 4) + j];
    uint8_t *o = out + k * hw + px;
    if (packed && px + 3 < hw) {
      *reinterpret_cast<uint32_t *>(o) = word;
    } else {
      for (int b = 0; b < 4 && px + b < hw; ++b) o[b] = (uint8_t)(word >> (8 * b));
    }
  }
}

// slices a wave holds in the channel-last form: the smallest of 8, 16, 32, 64 that holds them all
static int cube_wave_slices(const CubeView &v) { return v.n_slices <= 8 ? 8 : v.n_slices <= 16 ? 16 : v.n_slices <= 32 ? 32 : CL_S; }

// partial pairs per slice; n_slices * blocks <= max(65536, n_slices): the scratch is at most 1 MiB + 32 B a slice
size_t cube_minmax_blocks(const CubeView &v) {
  const size_t hw = v.h * v.w;
  if (hw == 0 || v.n_slices == 0) return 1;
  if (cube_form(v) == CUBE_CHANNEL_LAST) {
    const size_t sl = cube_wave_slices(v), held = (v.n_slices + sl - 1) / sl * sl;
    return std::min<size_t>(std::min<size_t>((hw + CL_P - 1) / CL_P, 8192), std::max<size_t>(65536 / held, 1));
  }
  return std::min<size_t>((hw + 2047) / 2048, std::max<size_t>(8192 / v.n_slices, 1));
}

#define WS_CUBE_SL(call_of)                    \
  switch (cube_wave_slices(v)) {               \
    case 8: call_of(8); break;                 \
    case 16: call_of(16); break;               \
    case 32: call_of(32); break;               \
    default: call_of(64); break;               \
  }

template <typename T>
static hipError_t run_cube_minmax(hipStream_t s, const void *data, const CubeView &v, double *scratch, unsigned long long *bad) {
  const size_t hw = v.h * v.w, B = cube_minmax_blocks(v);
  const PixMap m = pix_map(v);
  const T *d = (const T *)data;
  switch (cube_form(v)) {
    case CUBE_CHANNEL_LAST:
#define WS_FOLD_CL(SL) k_cube_minmax_cl<T, SL><<<(unsigned)((v.n_slices + SL - 1) / SL * B), 256, 0, s>>>(d, v.n_slices, hw, m, (unsigned)B, scratch)
      WS_CUBE_SL(WS_FOLD_CL)
#undef WS_FOLD_CL
      break;
    case CUBE_ROWS: k_cube_minmax<T, true><<<(unsigned)(v.n_slices * B), 256, 0, s>>>(d, hw, v.ss, m, (unsigned)B, scratch); break;
    default: k_cube_minmax<T, false><<<(unsigned)(v.n_slices * B), 256, 0, s>>>(d, hw, v.ss, m, (unsigned)B, scratch); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  k_cube_minmax_final<<<(unsigned)((v.n_slices + 3) / 4), 256, 0, s>>>(scratch, v.n_slices, (unsigned)B, scratch + cube_minmax_final_at(v), bad);
  return hipGetLastError();
}

template <typename T>
static hipError_t run_cube_quantise(hipStream_t s, const void *data, const CubeView &v, uint8_t maxv, const double *minmax, uint8_t *out) {
  const size_t hw = v.h * v.w;
  const PixMap m = pix_map(v);
  const T *d = (const T *)data;
  if (cube_form(v) == CUBE_CHANNEL_LAST) {
    const size_t sl = cube_wave_slices(v), tp = (size_t)CL_P * 64 / sl;
    const size_t tiles_p = (hw + tp - 1) / tp, chunks = (v.n_slices + sl - 1) / sl;
    if (tiles_p * chunks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const int packed = ((reinterpret_cast<uintptr_t>(out) | hw) & 3u) == 0;
#define WS_QUANT_CL(SL) k_cube_quantise_cl<T, SL><<<(unsigned)(tiles_p * chunks), 256, 0, s>>>(d, v.n_slices, hw, m, tiles_p, minmax, (double)maxv, out, packed)
    WS_CUBE_SL(WS_QUANT_CL)
#undef WS_QUANT_CL
    return hipGetLastError();
  }
  const size_t B = std::min<size_t>((hw + 1023) / 1024, std::max<size_t>(65536 / v.n_slices, 1));
  if (cube_form(v) == CUBE_ROWS) k_cube_quantise<T, true><<<(unsigned)(v.n_slices * B), 256, 0, s>>>(d, hw, v.ss, m, (unsigned)B, minmax, (double)maxv, out);
  else k_cube_quantise<T, false><<<(unsigned)(v.n_slices * B), 256, 0, s>>>(d, hw, v.ss, m, (unsigned)B, minmax, (double)maxv, out);
  return hipGetLastError();
}

#define WS_CUBE_DISPATCH(fn, ...)                          \
  switch (dtype) {                                         \
    case 0: return fn<float>(__VA_ARGS__);                 \
    case 1: return fn<double>(__VA_ARGS__);                \
    case 2: return fn<int32_t>(__VA_ARGS__);               \
    case 3: return fn<uint16_t>(__VA_ARGS__);              \
    case 4: return fn<int16_t>(__VA_ARGS__);               \
    case 5: return fn<uint8_t>(__VA_ARGS__);               \
    default: return hipErrorInvalidValue;                  \
  }

hipError_t cube_minmax(hipStream_t s, const void *data, int dtype, const CubeView &v, double *scratch, unsigned long long *bad) {
  if (v.n_slices * v.h * v.w == 0) return hipSuccess;
  WS_CUBE_DISPATCH(run_cube_minmax, s, data, v, scratch, bad)
}

hipError_t cube_quantise(hipStream_t s, const void *data, int dtype, const CubeView &v, uint8_t maxv, const double *minmax, uint8_t *out) {
  if (v.n_slices * v.h * v.w == 0) return hipSuccess;
  WS_CUBE_DISPATCH(run_cube_quantise, s, data, v, maxv, minmax, out)
}

}  // namespace wsk

using namespace wsapi;

namespace {

// n_slices * h * w and the view's span in elements (ws_cube_plan.hpp), refused when either leaves size_t; the slice count must fit a 1-D grid
int cube_extent(ws_ctx *c, size_t n_slices, size_t h, size_t w, size_t ss, size_t rs, size_t cs, size_t *total, size_t *span) {
  if (!wsplan::cube_extent(n_slices, h, w, ss, rs, cs, total, span)) return fail(c, WS_ERR_TOO_LARGE, "n_slices * h * w or the view's span overflows");
  if (*total && n_slices > 0x7FFFFFF0ull) return fail(c, WS_ERR_TOO_LARGE, "too many slices");
  return WS_OK;
}

int pre_processor_batch_body(ws_ctx *c, const void *d_data, int dtype, const CubeView &v, uint8_t max_value, uint8_t *d_out, double *d_minmax,
                             size_t *failed_slice) {
  int rc;
  const size_t doubles = cube_minmax_doubles(v);
  if ((rc = ensure(c, c->counts, (doubles + 1) * sizeof(double)))) return rc;
  double *scratch = (double *)c->counts.p, *minmax = scratch + cube_minmax_final_at(v);
  unsigned long long *bad = dtype == WS_F64 ? (unsigned long long *)(scratch + doubles) : nullptr;
  if (bad) HIP_TRY(c, hipMemsetAsync(bad, 0xFF, sizeof *bad, c->stream));
  HIP_TRY(c, cube_minmax(c->stream, d_data, dtype, v, scratch, bad));
  if (d_minmax) HIP_TRY(c, hipMemcpyAsync(d_minmax, minmax, 2 * v.n_slices * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
  if (bad) {
    // only f64 data can span more than DBL_MAX (ws_pre_processor_device): ONE word for the whole cube, read once
    unsigned long long first_bad = ~0ull;
    HIP_TRY(c, hipMemcpyAsync(&first_bad, bad, sizeof first_bad, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (first_bad != ~0ull) {
      if (failed_slice) *failed_slice = (size_t)first_bad;
      return fail(c, WS_ERR_UNSUPPORTED, "max - min of a slice is not finite: the reference panics (to_u8().unwrap() on NaN, lib.rs:1164)");
    }
  }
  HIP_TRY(c, cube_quantise(c->stream, d_data, dtype, v, max_value, minmax, d_out));
  return WS_OK;
}

int check_pre_processor(ws_ctx *c, int dtype, uint8_t max_value) {
  if (preproc_elem_size(dtype) == 0) return fail(c, WS_ERR_BAD_ARG, "unknown dtype");
  if (max_value >= WS_NEVER_FILL) return fail(c, WS_ERR_MAX_TOO_HIGH, "MAX must be < NEVER_FILL (lib.rs:1143)");
  if (max_value <= WS_ALWAYS_FILL) return fail(c, WS_ERR_MAX_TOO_LOW, "MAX must be > ALWAYS_FILL (lib.rs:1144)");
  return WS_OK;
}

}  // namespace

extern "C" {

int ws_pre_processor_batch_device(ws_ctx *c, const void *d_data, int dtype, size_t n_slices, size_t h, size_t w, size_t slice_stride,
                                  size_t row_stride, size_t col_stride, uint8_t max_value, uint8_t *d_out, double *d_minmax,
                                  size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  size_t total = 0, span = 0;
  int rc;
  if ((rc = check_pre_processor(c, dtype, max_value))) return rc;
  if ((rc = cube_extent(c, n_slices, h, w, slice_stride, row_stride, col_stride, &total, &span))) return rc;
  if (total && (!d_data || !d_out)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (total == 0) return WS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  return pre_processor_batch_body(c, d_data, dtype, CubeView{n_slices, h, w, slice_stride, row_stride, col_stride}, max_value, d_out, d_minmax,
                                  failed_slice);
}

int ws_pre_processor_batch(ws_ctx *c, const void *data, int dtype, size_t n_slices, size_t h, size_t w, size_t slice_stride, size_t row_stride,
                           size_t col_stride, uint8_t max_value, uint8_t *out, double *minmax, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  size_t total = 0, span = 0;
  int rc;
  if ((rc = check_pre_processor(c, dtype, max_value))) return rc;
  if ((rc = cube_extent(c, n_slices, h, w, slice_stride, row_stride, col_stride, &total, &span))) return rc;
  if (total && (!data || !out)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (total == 0) return WS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t es = preproc_elem_size(dtype);
  const CubeView v{n_slices, h, w, slice_stride, row_stride, col_stride};
  // the bytes between the view's first and last element cross in ONE copy; the kernels read them with the caller's strides
  if ((rc = ensure(c, c->aux, span * es))) return rc;
  if ((rc = ensure(c, c->img, total))) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->aux.p, data, span * es, hipMemcpyHostToDevice, c->stream));
  rc = pre_processor_batch_body(c, c->aux.p, dtype, v, max_value, (uint8_t *)c->img.p, nullptr, failed_slice);
  if (minmax && (rc == WS_OK || rc == WS_ERR_UNSUPPORTED)) {
    const int rc_keep = rc;
    HIP_TRY(c, hipMemcpyAsync(minmax, (const double *)c->counts.p + cube_minmax_final_at(v), 2 * n_slices * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    rc = rc_keep;
  }
  if (rc == WS_OK) HIP_TRY(c, hipMemcpyAsync(out, c->img.p, total, hipMemcpyDeviceToHost, c->stream));
  const std::string msg = c->err;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (rc != WS_OK) c->err = msg;
  return rc;
}

// One count launch, one scan of the strip counts, one write launch and ONE readback (the run's offsets) per run of slices; a run is as
// many whole slices as stay under the context's batch pixel limit, under 2^31 - 16 stacked rows and under MINIMA_RUN_NIBBLE_BYTES of
// nibble plane, at least one slice (wsplan::minima_run_slices).
int ws_find_local_minima_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                      size_t slice_stride, uint32_t *d_out_rc, size_t cap, size_t *seed_offsets, size_t *n_found) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c || !n_found || !seed_offsets || (!d_cube && n_slices * h * w) || (!d_out_rc && cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (row_stride < w) return fail(c, WS_ERR_BAD_ARG, "row_stride < w");
  if (h > 0x7FFFFFF0ull || w > 0x7FFFFFF0ull || h * w >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "plane has >= 2^32 pixels");
  *n_found = 0;
  for (size_t k = 0; k <= n_slices; ++k) seed_offsets[k] = 0;
  if (n_slices == 0 || h < 3 || w < 3) return WS_OK;                          // no 3x3 window (lib.rs:1183)
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t row_nibbles = minima_mask_bytes(1, (int)w);
  const size_t per_run = wsplan::minima_run_slices(n_slices, h, w, c->batch_max_px, row_nibbles);
  int rc;
  const size_t rows_max = per_run * h;
  if ((rc = ensure(c, c->counts, minima_stack_words(rows_max, per_run) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->aux, rows_max * row_nibbles))) return rc;
  std::vector<uint32_t> offs(per_run + 1);
  size_t total = 0;
  for (size_t k0 = 0; k0 < n_slices; k0 += per_run) {
    const size_t g = std::min(per_run, n_slices - k0);
    const size_t room = cap > total ? cap - total : 0;
    uint32_t *out = room ? d_out_rc + 2 * total : nullptr;
    uint32_t *d_offs = nullptr;
    HIP_TRY(c, minima_stack(c->stream, d_cube + k0 * slice_stride, row_stride, slice_stride, g, (int)h, (int)w, (uint32_t *)c->counts.p,
                            (uint8_t *)c->aux.p, out, room, &d_offs));
    HIP_TRY(c, hipMemcpyAsync(offs.data(), d_offs, (g + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    total = wsplan::minima_add_run(offs.data(), g, k0, total, seed_offsets);
  }
  seed_offsets[n_slices] = total;
  *n_found = total;
  if (total > cap) return fail(c, WS_ERR_CAPACITY, "seed buffer too small");
  return WS_OK;
}

int ws_find_local_minima_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                               uint64_t *out_rc, size_t cap, size_t *seed_offsets, size_t *n_found) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c || !n_found || !seed_offsets || (!cube && n_slices * h * w) || (!out_rc && cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (row_stride < w) return fail(c, WS_ERR_BAD_ARG, "row_stride < w");
  if (h > 0x7FFFFFF0ull || w > 0x7FFFFFF0ull || h * w >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "plane has >= 2^32 pixels");
  *n_found = 0;
  for (size_t k = 0; k <= n_slices; ++k) seed_offsets[k] = 0;
  if (n_slices == 0 || h < 3 || w < 3) return WS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t hw = h * w;
  size_t total_px = 0;
  if (__builtin_mul_overflow(hw, n_slices, &total_px)) return fail(c, WS_ERR_TOO_LARGE, "n_slices * h * w overflows");
  int rc;
  if ((rc = ensure(c, c->batch_cube, total_px))) return rc;
  uint8_t *d_cube = (uint8_t *)c->batch_cube.p;
  if (row_stride == w && (n_slices == 1 || slice_stride == hw)) {
    HIP_TRY(c, hipMemcpyAsync(d_cube, cube, total_px, hipMemcpyHostToDevice, c->stream));
  } else {
    for (size_t k = 0; k < n_slices; ++k)
      HIP_TRY(c, hipMemcpy2DAsync(d_cube + k * hw, w, cube + k * slice_stride, row_stride, w, h, hipMemcpyHostToDevice, c->stream));
  }
  // at most one strict maximum per 2x2 block of a slice's interior
  const size_t bound = ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1) * n_slices;
  const size_t dcap = std::min(cap, bound);
  if ((rc = ensure(c, c->batch_seeds, std::max<size_t>(dcap, 1) * 2 * sizeof(uint32_t)))) return rc;
  rc = ws_find_local_minima_batch_device(c, d_cube, n_slices, h, w, w, hw, (uint32_t *)c->batch_seeds.p, dcap, seed_offsets, n_found);
  if (rc != WS_OK && rc != WS_ERR_CAPACITY) return rc;
  const size_t got = std::min(*n_found, dcap);
  if (got)
    if (int rc_copy = labels_to_host_u64(c, (const uint32_t *)c->batch_seeds.p, out_rc, got * 2)) return rc_copy;
  return rc;
}

}  // extern "C"
