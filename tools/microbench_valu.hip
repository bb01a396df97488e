// microbench_valu.hip -- what is the integer vector-issue ceiling of gfx950 for the instruction mix of the relaxation?
//
// the big kernels were labelled "VALU bound" from VALUBusy (a gfx94x formula) and DESIGN computed
// with 16 lanes per clock and SIMD; MI355X_MICROARCH.md says SIMD-32 (a wave64 instruction issues over 2 cycles).  This
// measures, per instruction kind and per occupancy (1..8 waves per SIMD):
//   * independent streams of v_add_u32 / v_min_u32 / v_min3_u32 / v_med3_u32 / v_mov_b32_dpp (wave_shr:1): lane-ops/s of the
//     whole chip and cycles per wave-instruction per SIMD;
//   * the relaxation's own inner loop (ws_relax_patch.hpp: relax_px on a 4 x 4 register patch, sweeps down / right / up / left
//     with the DPP column refresh, Gauss-Seidel dependencies and all): pixel updates/s -- the ceiling a tile run's sweeps
//     can reach when nothing else (loads, LDS rows, barriers, flags) is in the way.
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -Irustronomy-watershed_amd/csrc -o tools/_build/microbench_valu tools/microbench_valu.hip
// Run (GPU box): tools/_build/microbench_valu > gpurun_out/valu.txt
#include <hip/hip_runtime.h>
#include "ws_relax_patch.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); exit(1); } } while (0)

constexpr int NCH = 16;      // independent chains per lane (the relaxation holds 16 stamps per lane)

enum { OP_ADD = 0, OP_MIN = 1, OP_MIN3 = 2, OP_MED3 = 3, OP_DPP = 4, OP_MIX4 = 5, OP_DEPCHAIN = 6 };

template <int OP>
__global__ __launch_bounds__(256) void k_stream(uint32_t *out, int iters, uint32_t x) {
  uint32_t a[NCH], b = x ^ threadIdx.x, c = x + 7u * threadIdx.x;
#pragma unroll
  for (int i = 0; i < NCH; ++i) a[i] = x * (i + 1) + threadIdx.x;
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      if (OP == OP_ADD) asm volatile("v_add_u32 %0, %1, %2" : "=v"(a[i]) : "v"(a[i]), "v"(b));
      if (OP == OP_MIN) asm volatile("v_min_u32 %0, %1, %2" : "=v"(a[i]) : "v"(a[i]), "v"(b));
      if (OP == OP_MIN3) asm volatile("v_min3_u32 %0, %1, %2, %3" : "=v"(a[i]) : "v"(a[i]), "v"(b), "v"(c));
      if (OP == OP_MED3) asm volatile("v_med3_u32 %0, %1, %2, %3" : "=v"(a[i]) : "v"(a[i]), "v"(b), "v"(c));
      if (OP == OP_DPP) asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %1 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(a[(i + 1) % NCH]));
      if (OP == OP_MIX4) {      // one pixel update's four instructions, on independent chains
        uint32_t m, n;
        asm volatile("v_min3_u32 %0, %1, %2, %3" : "=v"(m) : "v"(a[i]), "v"(b), "v"(c));
        asm volatile("v_min_u32 %0, %1, %2" : "=v"(n) : "v"(m), "v"(a[(i + 5) % NCH]));
        asm volatile("v_add_u32 %0, %1, 1" : "=v"(n) : "v"(n));
        asm volatile("v_med3_u32 %0, %1, %2, %3" : "=v"(a[i]) : "v"(b), "v"(n), "v"(a[i]));
      }
    }
    if (OP == OP_DEPCHAIN) {      // ONE chain of dependent instructions per lane: the latency a wave sees between two dependent VALU ops
#pragma unroll
      for (int i = 0; i < NCH; ++i) asm volatile("v_add_u32 %0, %1, %2" : "=v"(a[0]) : "v"(a[0]), "v"(b));
    }
  }
  uint32_t s = 0;
#pragma unroll
  for (int i = 0; i < NCH; ++i) s += a[i];
  if (s == 0x12345678u) out[threadIdx.x] = s;
}

// ---- the relaxation's inner loop: the engine's own relax_px, sweep_rows, sweep_cols and lane shifts (ws_relax_patch.hpp) ------
using namespace wsk;

// rounds of (down, right, up, checked left) on a register patch; `up` / `dn` stay what they were (in the engine they come
// from LDS once per round): 64 pixel updates per lane and round
template <int MINW>
__global__ __launch_bounds__(256, MINW) void k_sweeps(const uint32_t *in, uint32_t *out, int rounds) {
  const int tid = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t T[4][4], B[4][4], up[4], dn[4], Lh[4], Rh[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int c = 0; c < 4; ++c) { T[r][c] = in[(tid * 16 + r * 4 + c) & 0xFFFF] | 0x40000000u; B[r][c] = (T[r][c] >> 3) & 0x0FFFFFFFu; }
    up[r] = in[(tid + r) & 0xFFFF]; dn[r] = in[(tid + 4 + r) & 0xFFFF]; Lh[r] = up[r] + 3; Rh[r] = dn[r] + 5;
  }
  bool changed = false;
  for (int it = 0; it < rounds; ++it) {
    auto refresh = [&]() {
#pragma unroll
      for (int r = 0; r < 4; ++r) { Lh[r] = lane_left(Lh[r], T[r][3]); Rh[r] = lane_right(Rh[r], T[r][0]); }
    };
    bool untracked = false;
    refresh(); sweep_rows<false, true>(T, B, up, dn, Lh, Rh, untracked);
    refresh(); sweep_cols<false, true>(T, B, up, dn, Lh, Rh, untracked);
    refresh(); sweep_rows<false, false>(T, B, up, dn, Lh, Rh, untracked);
    refresh(); sweep_cols<true, false>(T, B, up, dn, Lh, Rh, changed);
    // keep the values moving: without this the patch is a fixpoint after a few rounds and the compiler knows nothing, but
    // the hardware does the same work either way (no data-dependent timing in these instructions)
  }
  uint32_t s = changed ? 1u : 0u;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) s += T[r][c];
  out[tid] = s;
}

__global__ void k_clock(unsigned long long *out) {      // shader clock against the 100 MHz real-time counter
  const unsigned long long c0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long r1 = r0;
  while (r1 - r0 < 100000ull) r1 = __builtin_amdgcn_s_memrealtime();      // 1 ms
  const unsigned long long c1 = __builtin_amdgcn_s_memtime();
  if (threadIdx.x == 0 && blockIdx.x == 0) { out[0] = c1 - c0; out[1] = r1 - r0; }
}

template <class F>
float time_ms(F f, int reps = 5) {
  hipEvent_t a, b;
  CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
  f(); f();
  CHECK(hipEventRecord(a));
  for (int i = 0; i < reps; ++i) f();
  CHECK(hipEventRecord(b));
  CHECK(hipEventSynchronize(b));
  float ms; CHECK(hipEventElapsedTime(&ms, a, b));
  CHECK(hipEventDestroy(a)); CHECK(hipEventDestroy(b));
  return ms / reps;
}

int main() {
  hipDeviceProp_t prop; CHECK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  printf("device %s, %d CUs, clock %d kHz\n", prop.name, cus, prop.clockRate);
  uint32_t *d_out, *d_in; unsigned long long *d_clk;
  CHECK(hipMalloc(&d_out, (size_t)cus * 8 * 256 * 4 + 4096)); CHECK(hipMalloc(&d_in, 65536 * 4)); CHECK(hipMalloc(&d_clk, 16));
  std::vector<uint32_t> h(65536);
  for (size_t i = 0; i < h.size(); ++i) h[i] = (uint32_t)(i * 2654435761u) >> 4;
  CHECK(hipMemcpy(d_in, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  const int iters = 4096;
  const char *names[] = {"v_add_u32", "v_min_u32", "v_min3_u32", "v_med3_u32", "v_mov_dpp wave_shr:1 (+s_nop 1)", "min3+min+add+med3 (indep)", "v_add_u32 dependent chain"};
  // a warm-up that brings the clocks up
  for (int i = 0; i < 20; ++i) k_stream<OP_ADD><<<cus * 8, 256>>>(d_out, iters, 3u);
  CHECK(hipDeviceSynchronize());
  k_clock<<<1, 64>>>(d_clk);
  unsigned long long hc[2]; CHECK(hipMemcpy(hc, d_clk, 16, hipMemcpyDeviceToHost));
  printf("idle-ish shader clock: %.0f MHz\n", (double)hc[0] / (double)hc[1] * 100.0);
  printf("\n%-36s %5s %12s %14s %16s\n", "instruction stream", "w/SIMD", "ms", "Tlane-ops/s", "cyc/wave-instr/SIMD @2.4GHz");
  for (int op = 0; op <= OP_DEPCHAIN; ++op) {
    for (int w : {1, 2, 3, 4, 6, 8}) {
      const int grid = cus * w;      // 256-thread blocks: one wave per SIMD each
      auto launch = [&]() {
        switch (op) {
          case OP_ADD: k_stream<OP_ADD><<<grid, 256>>>(d_out, iters, 3u); break;
          case OP_MIN: k_stream<OP_MIN><<<grid, 256>>>(d_out, iters, 3u); break;
          case OP_MIN3: k_stream<OP_MIN3><<<grid, 256>>>(d_out, iters, 3u); break;
          case OP_MED3: k_stream<OP_MED3><<<grid, 256>>>(d_out, iters, 3u); break;
          case OP_DPP: k_stream<OP_DPP><<<grid, 256>>>(d_out, iters, 3u); break;
          case OP_MIX4: k_stream<OP_MIX4><<<grid, 256>>>(d_out, iters, 3u); break;
          default: k_stream<OP_DEPCHAIN><<<grid, 256>>>(d_out, iters, 3u); break;
        }
      };
      const float ms = time_ms(launch);
      const double per_lane = (double)iters * NCH * (op == OP_MIX4 ? 4 : 1);
      const double instr_per_simd = per_lane * w;      // wave-instructions issued on one SIMD
      const double lane_ops = per_lane * 256.0 * grid;
      printf("%-36s %5d %12.4f %14.2f %16.2f\n", names[op], w, ms, lane_ops / (ms * 1e-3) / 1e12, ms * 1e-3 * 2.4e9 / instr_per_simd);
    }
  }
  printf("\nrelaxation inner loop (4 x 4 register patch, rounds of down/right/up/checked-left with DPP column refresh):\n");
  printf("%5s %12s %16s %22s %26s\n", "w/SIMD", "ms", "Gpx-updates/s", "cyc/px-update/SIMD-lane", "ns per round per wave");
  const int rounds = 512;
  for (int w : {1, 2, 3, 4, 6, 8}) {
    const int grid = cus * w;
    auto launch = [&]() {
      if (w <= 4) k_sweeps<4><<<grid, 256>>>(d_in, d_out, rounds);      // <= 128 VGPRs
      else k_sweeps<6><<<grid, 256>>>(d_in, d_out, rounds);             // the 80-VGPR class of k_relax
    };
    const float ms = time_ms(launch);
    const double upd = (double)rounds * 64.0 * 256.0 * grid;
    printf("%5d %12.4f %16.1f %22.3f %26.1f\n", w, ms, upd / (ms * 1e-3) / 1e9, ms * 1e-3 * 2.4e9 * 32.0 * 4.0 * cus / upd, ms * 1e6 / rounds);
  }
  k_clock<<<1, 64>>>(d_clk);
  CHECK(hipMemcpy(hc, d_clk, 16, hipMemcpyDeviceToHost));
  printf("\nshader clock after the runs: %.0f MHz\n", (double)hc[0] / (double)hc[1] * 100.0);
  return 0;
}
