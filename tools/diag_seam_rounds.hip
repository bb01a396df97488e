// diag_seam_rounds.hip -- the seam-repair flow's first passes, step by step, with what each step leaves behind (never shipped):
// rounds per tile run of pass 0 (k_relax0_tall), of the bands and of the strips as histograms, the 256 x 32 tiles that pass 0
// marks for their re-run (word 2 of entry (x + 1, y) of the shifted grid's stamps, read straight after pass 0), the tiles
// flagged for pass 2 after the strips, and the time of every step (events, median of the repetitions).
//
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -DWS_DIAG_STAMPS -Irustronomy-watershed_amd/csrc -o tools/_build/diag_seam_rounds tools/diag_seam_rounds.hip
//   diag_seam_rounds [N [PREFIX]]      N: side of the field (8192); PREFIX: PREFIX.u8 / PREFIX.seeds of tools/sim_make_field.py
//                                      (without it: the bench's noise field, seed 1, and its local minima)
#include "../rustronomy-watershed_amd/csrc/ws_relax.hip"
#include <algorithm>
#include <cstdio>
#include <vector>
using namespace wsk;
#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s line %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
static unsigned long long mix64h(unsigned long long x) { unsigned long long z = x + 0x9E3779B97F4A7C15ull; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }

int main(int argc, char **argv) {
  const int N = argc > 1 ? atoi(argv[1]) : 8192;
  if (N < 512 || N % 4) { printf("N: a multiple of 4, 512 or more\n"); return 2; }
  const int H = N, W = N; const size_t n = (size_t)H * W;
  std::vector<uint8_t> himg(n);
  std::vector<uint32_t> hbits(n / 32 + 2, 0u);
  size_t n_seeds = 0;
  if (argc > 2) {
    char path[1024];
    snprintf(path, sizeof path, "%s.u8", argv[2]);
    FILE *f = fopen(path, "rb");
    if (!f || fread(himg.data(), 1, n, f) != n) { printf("cannot read %s\n", path); return 1; }
    fclose(f);
    snprintf(path, sizeof path, "%s.seeds", argv[2]);
    f = fopen(path, "rb");
    if (!f) { printf("cannot read %s\n", path); return 1; }
    uint32_t p;
    while (fread(&p, 4, 1, f) == 1) if (p < n) { hbits[p >> 5] |= 1u << (p & 31u); ++n_seeds; }
    fclose(f);
  } else {
    for (size_t i = 0; i < n; ++i) himg[i] = (uint8_t)(mix64h((1ull << 40) + i) % 254u);
    for (int y = 1; y < H - 1; ++y)
      for (int x = 1; x < W - 1; ++x) {
        const size_t p = (size_t)y * W + x; const uint8_t v = himg[p];
        bool ok = true;
        for (int dy = -1; dy <= 1 && ok; ++dy) for (int dx = -1; dx <= 1; ++dx) if ((dy || dx) && himg[p + (ptrdiff_t)dy * W + dx] >= v) { ok = false; break; }
        if (ok) { hbits[p >> 5] |= 1u << (p & 31u); ++n_seeds; }
      }
  }
  uint8_t *img; uint32_t *keys, *stamps, *flags, *bits, *list; unsigned long long *diag;
  const size_t ntiles = relax_tiles(H, W), cap = ntiles * 4;
  const size_t flag_words = (size_t)(COUNTER_RING + 4) * FLAG_SLOT;
  CHECK(hipMalloc(&img, n)); CHECK(hipMalloc(&keys, n * 4)); CHECK(hipMalloc(&stamps, 2 * cap * 4)); CHECK(hipMalloc(&flags, flag_words * 4));
  CHECK(hipMalloc(&bits, hbits.size() * 4)); CHECK(hipMalloc(&list, relax_list_words(H, W) * 4)); CHECK(hipMalloc(&diag, ntiles * 64));
  CHECK(hipMemcpy(img, himg.data(), n, hipMemcpyHostToDevice)); CHECK(hipMemcpy(bits, hbits.data(), hbits.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_diag), &diag, sizeof(diag)));
  CHECK(hipMemset(list, 0, relax_list_words(H, W) * 4));
  PassFlags pf{flags, flags + COUNTER_RING * FLAG_SLOT, flags + (COUNTER_RING + 3) * FLAG_SLOT, flags + (COUNTER_RING + 1) * FLAG_SLOT};
  RelaxPlane plane;
  plane.img = img; plane.img_stride = W; plane.keys = keys; plane.h = H; plane.w = W; plane.max_level = 254;
  plane.stamps = stamps; plane.pf = pf; plane.seed_labels = bits; plane.seed_bits = true; plane.tile_list = list; plane.seam_min_px = 1;
  if (!relax_plan_for(plane, 0).tall0) { printf("this plane does not take the seam flow on 256 x 64 tiles\n"); return 2; }
  const int ax = (W + RX_TW - 1) / RX_TW, ay = (H + SEAM_PY - 1) / SEAM_PY, sx = ax + 1;
  printf("field %d x %d, %zu seeds, %d x %d tiles of 256 x 32\n", H, W, n_seeds, ax, ay);

  const int reps = 5;
  std::vector<float> t_step[8];
  std::vector<unsigned long long> hd(ntiles * 8);
  std::vector<uint32_t> hs(2 * cap), hf(flag_words);
  hipEvent_t a, b; CHECK(hipEventCreate(&a)); CHECK(hipEventCreate(&b));
  for (int rep = 0; rep < reps; ++rep) {
    const bool report = rep == reps - 1;
    CHECK(hipMemset(stamps, 0, 2 * cap * 4)); CHECK(hipMemset(flags, 0, flag_words * 4)); CHECK(hipMemset(keys, 0xFF, n * 4));
    int slot = 0;
    for (uint32_t pass = 0; pass < 4; ++pass) {
      const RelaxPlan plan = relax_plan_for(plane, pass);
      const RelaxLaunch l{0, plane, stamps + ((pass + 1) & 1) * cap, stamps + (pass & 1) * cap, (uint32_t)ntiles, H, 1};
      for (int i = 0; i < plan.n; ++i, ++slot) {
        const RelaxStep &st = plan.steps[i];
        CHECK(hipMemset(diag, 0, ntiles * 64));
        if (report) CHECK(hipMemset(flags + (COUNTER_RING + 1) * FLAG_SLOT, 0, 2 * FLAG_SLOT * 4));
        CHECK(hipEventRecord(a));
        CHECK(launch_step(l, st));
        CHECK(hipEventRecord(b)); CHECK(hipEventSynchronize(b));
        float ms; CHECK(hipEventElapsedTime(&ms, a, b));
        if (rep > 0 && slot < 8) t_step[slot].push_back(ms * 1e3f);
        if (!report) continue;
        CHECK(hipMemcpy(hd.data(), diag, ntiles * 64, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(hs.data(), stamps, 2 * cap * 4, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(hf.data(), flags, flag_words * 4, hipMemcpyDeviceToHost));
        unsigned long runs = 0, rounds = 0;
        for (int k = 0; k < FLAG_SLOT; ++k) { runs += hf[(COUNTER_RING + 1) * FLAG_SLOT + k]; rounds += hf[(COUNTER_RING + 2) * FLAG_SLOT + k]; }
        std::sort(t_step[slot].begin(), t_step[slot].end());
        printf("pass %u step %d (kind %d, grid %u x %u): %.1f us (median of %zu, %.1f .. %.1f); tile runs (256 x 32 units) %lu, their rounds %lu\n", pass, i, (int)st.kind, st.grid, st.block,
               t_step[slot][t_step[slot].size() / 2], t_step[slot].size(), t_step[slot].front(), t_step[slot].back(), runs, rounds);
        if (pass < 2) {      // one tile per workgroup: thread 0's round count is in the workgroup's diagnostic line
          unsigned long hist[16] = {0}, ran = 0, sweeps = 0;
          for (unsigned w = 0; w < st.grid; ++w) {
            if (hd[(size_t)w * 8] == 0) continue;
            const unsigned long long it = hd[(size_t)w * 8 + 4];
            ++ran; ++hist[it < 15 ? it : 15]; sweeps += it;
          }
          printf("  workgroups that ran %lu of %u; ending in round 1 / 2 / ...:", ran, st.grid);
          for (int k = 1; k < 16; ++k) if (hist[k]) printf(" %d:%lu", k, hist[k]);
          printf("  (mean %.2f rounds)\n", ran ? (double)sweeps / ran : 0.0);
        }
        if (pass == 0) {
          unsigned long capped = 0;
          for (int y = 0; y < ay; ++y) for (int x = 0; x < ax; ++x) capped += hs[cap + ((size_t)y * sx + x + 1) * 4 + 2] == 2u;
          printf("  256 x 32 tiles marked for their re-run by pass 0's round cap: %lu of %d (%.1f %%)\n", capped, ax * ay, 100.0 * capped / (ax * ay));
        }
        if (pass == 1) {
          unsigned long flagged = 0, by_cap = 0;
          for (int y = 0; y < ay; ++y) for (int x = 0; x < ax; ++x) {
            const bool c = hs[cap + ((size_t)y * sx + x + 1) * 4 + 2] == 2u, f = hs[cap + ((size_t)y * sx + x) * 4 + 3] == 2u;
            flagged += c || f; by_cap += c;
          }
          printf("  after this step: 256 x 32 tiles flagged for pass 2: %lu of %d (%.1f %%), %lu of them by pass 0's cap\n", flagged, ax * ay, 100.0 * flagged / (ax * ay), by_cap);
        }
      }
    }
  }
  std::vector<uint32_t> hk(n);
  CHECK(hipMemcpy(hk.data(), keys, n * 4, hipMemcpyDeviceToHost));
  unsigned long long sum = 0;
  for (size_t p = 0; p < n; ++p) sum += hk[p] * (unsigned long long)(p % 1000003 + 1);
  printf("stamp plane after pass 3: checksum %llx (sim_tile_schedule.c's formula)\n", sum);
  return 0;
}
