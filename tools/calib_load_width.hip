// Calibration of rocprofv3's FETCH_SIZE on gfx950 by access width: three kernels stream the same 256 MiB buffer once per launch
// with coalesced 4-, 8- and 16-byte loads per lane (k_stream4 / k_stream8 / k_stream16), three launches each.  The true bytes
// per launch are the buffer's; FETCH_SIZE (KiB) per launch against them is the factor for that width (MI355X_MICROARCH.md, HBM
// section: exactly 1/2 for 16 B per lane, other widths uncalibrated; k_seed_tables reads 8-byte entries).
//   hipcc --offload-arch=gfx950 -O3 -o calib_load_width tools/calib_load_width.hip
//   rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- ./calib_load_width          (a run of its own: no trace beside it)
// A throw-away measuring tool: nothing in the library or the tests uses it.
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

// every lane folds what it loaded into one word and stores it only if it is a value the zero-filled buffer cannot give:
// the loads cannot be dropped, and nothing is written
__global__ void k_stream4(const uint32_t *p, size_t n, uint32_t *out) {
  uint32_t acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc |= p[i];
  if (acc == 0x12345678u) out[0] = acc;
}
__global__ void k_stream8(const uint2 *p, size_t n, uint32_t *out) {
  uint32_t acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { const uint2 v = p[i]; acc |= v.x | v.y; }
  if (acc == 0x12345678u) out[0] = acc;
}
__global__ void k_stream16(const uint4 *p, size_t n, uint32_t *out) {
  uint32_t acc = 0;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) { const uint4 v = p[i]; acc |= v.x | v.y | v.z | v.w; }
  if (acc == 0x12345678u) out[0] = acc;
}

int main() {
  const size_t bytes = (size_t)256 << 20;
  void *buf = nullptr;
  uint32_t *out = nullptr;
  CHECK(hipMalloc(&buf, bytes));
  CHECK(hipMalloc(&out, 64));
  CHECK(hipMemset(buf, 0, bytes));
  CHECK(hipMemset(out, 0, 64));
  const int blocks = 256 * 8, threads = 256;
  for (int rep = 0; rep < 3; ++rep) {
    k_stream4<<<blocks, threads>>>(static_cast<const uint32_t *>(buf), bytes / 4, out);
    k_stream8<<<blocks, threads>>>(static_cast<const uint2 *>(buf), bytes / 8, out);
    k_stream16<<<blocks, threads>>>(static_cast<const uint4 *>(buf), bytes / 16, out);
    CHECK(hipGetLastError());
  }
  CHECK(hipDeviceSynchronize());
  printf("calib_load_width: %zu bytes per launch, 3 launches of k_stream4, k_stream8, k_stream16\n", bytes);
  CHECK(hipFree(buf));
  CHECK(hipFree(out));
  return 0;
}
