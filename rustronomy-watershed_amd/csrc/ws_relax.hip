// ws_relax.hip -- relaxation kernel of the fused engine (gfx950, wave64).
//
// Fixpoint: key(p) = max(base(p), 1 + min over the 4 neighbours of key(q))   (ws_common.hpp).
//
// Layout
//   * a lane owns a 4 x 4 patch of pixels IN REGISTERS (16 stamps + 16 bases);
//   * a wave is a 256-pixel-wide band (64 lanes x 4 columns); the left/right neighbour columns come
//     from the adjacent LANES with one DPP wave shift each (v_mov_b32_dpp wave_shr:1 / wave_shl:1;
//     the `old` operand supplies the tile's halo column for lane 0 / lane 63): no LDS, no conflicts;
//   * the NW waves of a workgroup are NW bands stacked vertically: tile = 256 x 4*NW pixels; only
//     band boundary rows go through LDS, one ds_write_b128 / ds_read_b128 per lane and row;
//   * global loads/stores are 16 B per lane, 1 KiB per wave instruction, row contiguous, and every
//     load is unconditional on a clamped address (a load under a data-dependent branch is waited
//     for before the next is issued -- that serialised ~50 round trips per thread in the first
//     version of this engine);
//   * one iteration = four sweeps (down, right, up, left); a sweep updates a whole patch row (or
//     column) at a time, i.e. 4 independent pixel updates, so dependency chains are 4 long;
//   * TWO tilings alternate: even passes use the grid anchored at (0, 0), odd passes the grid shifted
//     by half a tile (128, 2*NW), so the borders of one pass lie in the middle of the next pass's
//     tiles.  On the bench field 99.3 % of the stamps are final after pass 0 and every wrong one lies
//     within 8 px of a tile border (tools/exp_apron.py): the shifted pass repairs them with correct
//     surroundings, instead of the 3-4 passes it takes to walk a correction back and forth over the
//     same border.  A tile runs in pass k iff a tile of pass k-1 changed one of ITS border pixels
//     inside the quadrant the two tiles share: a pixel equation can only be left violated next to a
//     border pixel that a neighbour changed after it was read, and that border pixel sits in the
//     interior (or halo) of exactly the tile of the other grid that owns the pixel.
//
// What the measurements said (tools/diag_relax.hip, per-workgroup s_memrealtime stamps, MI355X):
// with ~5 global atomics per tile on shared words (statistics + convergence counters) a full pass
// took 440 us however the sweeps were organised: same-address atomics retire at ~12 ns each, and
// 8192 tiles x 4-5 of them IS 440 us.  Hence: no same-address atomic on the tile path.  Convergence
// words are plain stores of 1 into striped slots (idempotent), statistics are striped counters
// that exist only when profiling is on.
#include "ws_common.hpp"
#include "ws_relax_plan.hpp"      // tile geometry, round caps and the schedule (relax_plan)
#include "ws_relax_patch.hpp"     // the register patch: relax_px, the sweeps, patch_bases
#include "ws_relax_queue.hpp"     // tile_list's layout; the tile queue of the persistent pass

#include <algorithm>
#include <cstdio>
#include <cstdlib>

namespace wsk {

// Diagnostic build only (tools/diag_relax.hip defines WS_DIAG_STAMPS): per-workgroup phase stamps.
#ifdef WS_DIAG_STAMPS
__device__ unsigned long long *g_diag = nullptr;
#define WS_STAMP(slot)                                                                          \
  do {                                                                                          \
    if (threadIdx.x == 0 && g_diag) g_diag[(size_t)blockIdx.x * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); \
  } while (0)
#define WS_STAMP_VALUE(slot, v)                                                                 \
  do {                                                                                          \
    if (threadIdx.x == 0 && g_diag) g_diag[(size_t)blockIdx.x * 8 + (slot)] = (v);              \
  } while (0)
// time spent between two points, summed over a tile run (thread 0's view): WS_ACC_T0 / WS_ACC(slot) pairs
#define WS_ACC_DECL unsigned long long ws_acc_t = 0, ws_acc[3] = {0, 0, 0}
#define WS_ACC_T0 (ws_acc_t = __builtin_amdgcn_s_memrealtime())
#define WS_ACC(k) do { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); ws_acc[k] += n_ - ws_acc_t; ws_acc_t = n_; } while (0)
#define WS_ACC_STORE do { if (threadIdx.x == 0 && g_diag) { g_diag[(size_t)blockIdx.x * 8 + 5] = ws_acc[0]; g_diag[(size_t)blockIdx.x * 8 + 6] = ws_acc[1]; g_diag[(size_t)blockIdx.x * 8 + 7] = ws_acc[2]; } } while (0)
#else
#define WS_ACC_DECL do {} while (0)
#define WS_ACC_T0 do {} while (0)
#define WS_ACC(k) do {} while (0)
#define WS_ACC_STORE do {} while (0)
#define WS_STAMP(slot) do {} while (0)
#define WS_STAMP_VALUE(slot, v) do {} while (0)
#endif

// -DWS_TUNING, the queue pass (k_relax, PERSIST): ticks of thread 0 per phase of a tile run, in the kernel's q_ph / q_tp
#ifdef WS_TUNING
#define WS_QPHASE(k) do { if (PERSIST && threadIdx.x == 0) { const unsigned long long n_ = __builtin_amdgcn_s_memrealtime(); q_ph[k] += (uint32_t)(n_ - q_tp); q_tp = n_; } } while (0)
#define WS_QPHASE0 do { if (PERSIST && threadIdx.x == 0) q_tp = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define WS_QPHASE(k) do {} while (0)
#define WS_QPHASE0 do {} while (0)
#endif

// element p of a u32 plane, or bit p of a bit plane
__device__ __forceinline__ uint32_t plane_or_bit(const uint32_t *src, size_t p, int bits) {
  return bits ? (src[p >> 5] >> (p & 31u)) & 1u : src[p];
}

// Stamp words of the SAME-GRID passes (relax_todo, read_same): pass + 1 in the low bits, and
constexpr uint32_t ST_BORDER = 0x40000000u;      // a border pixel of the tile inside this quadrant changed
constexpr uint32_t ST_SELF = 0x80000000u;        // (word 0) the tile stopped at its round cap: it goes on itself
constexpr uint32_t ST_PASS = 0x3FFFFFFFu;

// Which tiles of the chunk starting at `first` have to run in this pass?  Lane k answers for tile
// first + k; the ballot is the to-do list.  tilesX x tilesY is this pass's grid, otherX x otherY the
// grid of the previous pass.
template <int TW, int TH>
__device__ __forceinline__ unsigned long long relax_todo(int first, int stride, int chunk, int H, int W, int tilesX, int tilesY, int otherX,
                                                         int otherY, int shifted, uint32_t pass,
                                                         const uint32_t *__restrict__ stamps_prev, int read_same = 0) {
  const int lane = threadIdx.x & 63;
  const int ox = shifted ? TW / 2 : 0, oy = shifted ? TH / 2 : 0;
  const int t = first + lane * stride;
  const bool mine = lane < chunk && t < tilesX * tilesY;
  const int tx = mine ? t % tilesX : 0, ty = mine ? t / tilesX : 0;
  // a shifted grid can have a last row/column outside the plane
  bool run = mine && tx * TW - ox < W && ty * TH - oy < H;
  if (read_same) {
    // Same-grid passes (the long-range regime): the previous pass ran on THIS grid.  A tile runs when it stopped at its
    // round cap itself, or when a 4-neighbour changed a border pixel on the side facing it -- the two quadrants of the
    // neighbour that hold that side (quadrant = 2 * lower half + right half).  Exact for the same reason as the
    // alternating grids: an equation can only be left violated next to a border pixel that changed after it was read.
    const size_t tt = (size_t)ty * tilesX + tx;
    const uint32_t s0 = stamps_prev[tt * 4];
    bool flagged = (s0 & ST_PASS) == pass && (s0 & ST_SELF) != 0u;
    const int nx[4] = {tx, tx, tx - 1, tx + 1}, ny[4] = {ty - 1, ty + 1, ty, ty};
    const int qa[4] = {2, 0, 1, 0}, qb[4] = {3, 1, 3, 2};      // up: its bottom quadrants; down: top; left: right; right: left
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool ok = nx[k] >= 0 && nx[k] < tilesX && ny[k] >= 0 && ny[k] < tilesY;
      const size_t ot = (size_t)(ok ? ny[k] : 0) * tilesX + (ok ? nx[k] : 0);
      const uint32_t a = stamps_prev[ot * 4 + qa[k]], b = stamps_prev[ot * 4 + qb[k]];
      flagged |= ok && (((a & ST_PASS) == pass && (a & ST_BORDER) != 0u) || ((b & ST_PASS) == pass && (b & ST_BORDER) != 0u));
    }
    run = run && flagged;
  } else if (pass != 0) {
    // Quadrant (qx, qy) of a tile is quadrant (1-qx, 1-qy) of one tile of the previous pass's grid:
    // did that tile change a border pixel there?  Four independent loads on clamped indices.
    bool flagged = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int qx = q & 1, qy = q >> 1;
      const int oi = tx + qx - (shifted ? 1 : 0), oj = ty + qy - (shifted ? 1 : 0);
      const bool ok = oi >= 0 && oi < otherX && oj >= 0 && oj < otherY;
      const size_t ot = (size_t)(ok ? oj : 0) * otherX + (ok ? oi : 0);
      const uint32_t st = stamps_prev[ot * 4 + (3 - q)];
      flagged |= ok && st == pass;
    }
    run = run && flagged;
  }
  return __builtin_amdgcn_ballot_w64(run);
}

// CHUNKED = false: one tile per workgroup -- the passes in which (nearly) every tile runs.
// CHUNKED = true: `chunk` (<= 64) consecutive tiles per workgroup, run one after the other -- the late
// passes, in which few tiles run: a pass with nothing to do costs 1/chunk of the workgroup launches.
// (One body for both, not a shared device function: at the 80-VGPR cap the out-of-line form spilled.)
// ---- long-range rows ---------------------------------------------------------------------------
//
// A column sweep moves information one patch (4 pixels) per round along a row, so a flood that has to
// cross a 256-pixel tile sideways -- the normal case on a smooth map -- took 64 rounds per tile and pass.
// The row recurrence  t_x <- min(t_x, max(b_x, t_{x-1} + 1))  is a chain of clamped increments
// f_x(v) = med3(b_x, v + 1, t_x), and those compose:  (g o f)(v) = med3(lo, v + a, hi)  with
//   a = a_f + a_g,  lo = med3(lo_g, lo_f + a_g, hi_g),  hi = med3(lo_g, hi_f + a_g, hi_g).
// So the whole row is evaluated EXACTLY -- the same values the sequential sweep would give, pixel by
// pixel, ring carries included -- by a 6-step inclusive scan over the lanes of the wave: each lane
// reduces its 4 pixels to one (lo, hi, 4) triple, the scan composes triples, and every lane then knows
// the value that enters it from its neighbour.  Used only from pass RX_SCAN_FROM_PASS on (ws_relax_plan.hpp, with the
// round caps of those passes and what was measured for them).

template <bool TRACK, bool RIGHT, int LX>
__device__ __forceinline__ void scan_row(uint32_t (&t)[RX_P], const uint32_t (&b)[RX_P], uint32_t halo_in, int xl, bool &changed) {
  // LX lanes make a tile row (64, or 32 when a wave holds two half-width bands: xl = lane & 31, and nothing crosses lane 32)
  // pixels in sweep order
  const uint32_t t0 = RIGHT ? t[0] : t[3], t1 = RIGHT ? t[1] : t[2], t2 = RIGHT ? t[2] : t[1], t3 = RIGHT ? t[3] : t[0];
  const uint32_t b0 = RIGHT ? b[0] : b[3], b1 = RIGHT ? b[1] : b[2], b2 = RIGHT ? b[2] : b[1], b3 = RIGHT ? b[3] : b[0];
  // this lane's four pixels as one function: its value for a huge and for a tiny argument
  uint32_t hi = t0;
  hi = med3u(b1, hi + 1u, t1); hi = med3u(b2, hi + 1u, t2); hi = med3u(b3, hi + 1u, t3);
  uint32_t lo = b0;
  lo = med3u(b1, lo + 1u, t1); lo = med3u(b2, lo + 1u, t2); lo = med3u(b3, lo + 1u, t3);
  // Every lane adds the same RX_P to what passes through it, so in the coordinate W = v + RX_P * (lanes still to go, this
  // one included) a lane is a PURE clamp [lo + bias, hi + bias], and clamps compose by two medians -- no running sum to
  // carry through the scan, no additions inside it (r2: a third fewer instructions per step, two shuffles instead of three)
  const uint32_t bias = RIGHT ? (uint32_t)(RX_P * (LX - 1 - xl)) : (uint32_t)(RX_P * xl);
  lo += bias;
  hi += bias;
  // Inclusive scan in sweep order, acc_i <- acc_(i -/+ o) then acc_i, WITHOUT LDS round trips (__shfl_up is a ds_bpermute:
  // ~100 cycles a step, twelve dependent steps per row and direction, in passes that run at 40 % VALU use): inside a row
  // of 16 lanes four DPP row shifts whose `old` operand is the identity for lanes with nothing before them (0 for the
  // lower bound: med3(lo, 0, hi) = lo; ~0 for the upper one), then the rows' totals across rows -- DPP row broadcasts
  // going right, v_readlane of the rows' first lanes going left (GFX9 has no broadcast in that direction).
  auto combine = [&](uint32_t plo, uint32_t phi) {
    const uint32_t nlo = med3u(lo, plo, hi), nhi = med3u(lo, phi, hi);      // the earlier clamp, then this one
    lo = nlo; hi = nhi;
  };
#define WS_DPP(old, v, ctrl, rows) (uint32_t)__builtin_amdgcn_update_dpp((int)(old), (int)(v), ctrl, rows, 0xF, false)
  if (RIGHT) {
    combine(WS_DPP(0u, lo, 0x111, 0xF), WS_DPP(~0u, hi, 0x111, 0xF));      // row_shr:1
    combine(WS_DPP(0u, lo, 0x112, 0xF), WS_DPP(~0u, hi, 0x112, 0xF));      // row_shr:2
    combine(WS_DPP(0u, lo, 0x114, 0xF), WS_DPP(~0u, hi, 0x114, 0xF));      // row_shr:4
    combine(WS_DPP(0u, lo, 0x118, 0xF), WS_DPP(~0u, hi, 0x118, 0xF));      // row_shr:8
    combine(WS_DPP(0u, lo, 0x142, 0xA), WS_DPP(~0u, hi, 0x142, 0xA));      // row_bcast:15 into rows 1 and 3
    if (LX == 64) combine(WS_DPP(0u, lo, 0x143, 0xC), WS_DPP(~0u, hi, 0x143, 0xC));      // row_bcast:31 into rows 2 and 3
  } else {
    combine(WS_DPP(0u, lo, 0x101, 0xF), WS_DPP(~0u, hi, 0x101, 0xF));      // row_shl:1
    combine(WS_DPP(0u, lo, 0x102, 0xF), WS_DPP(~0u, hi, 0x102, 0xF));      // row_shl:2
    combine(WS_DPP(0u, lo, 0x104, 0xF), WS_DPP(~0u, hi, 0x104, 0xF));      // row_shl:4
    combine(WS_DPP(0u, lo, 0x108, 0xF), WS_DPP(~0u, hi, 0x108, 0xF));      // row_shl:8
    {
      const int lane = (int)(threadIdx.x & 63u);
      const uint32_t l16 = (uint32_t)__builtin_amdgcn_readlane((int)lo, 16), h16 = (uint32_t)__builtin_amdgcn_readlane((int)hi, 16);
      const uint32_t l48 = (uint32_t)__builtin_amdgcn_readlane((int)lo, 48), h48 = (uint32_t)__builtin_amdgcn_readlane((int)hi, 48);
      const bool r0 = lane < 16, r2 = lane >= 32 && lane < 48;      // rows 0 and 2 take the total of the row after them
      combine(r0 ? l16 : (r2 ? l48 : 0u), r0 ? h16 : (r2 ? h48 : ~0u));
      if (LX == 64) {
        const uint32_t l32 = (uint32_t)__builtin_amdgcn_readlane((int)lo, 32), h32 = (uint32_t)__builtin_amdgcn_readlane((int)hi, 32);
        combine(lane < 32 ? l32 : 0u, lane < 32 ? h32 : ~0u);
      }
    }
  }
#undef WS_DPP
  // the value that leaves this lane when `halo_in` enters the row, handed to the next lane
  const uint32_t leaves = med3u(lo, halo_in + (uint32_t)(RX_P * LX), hi) - bias;
  uint32_t vin = RIGHT ? lane_left(halo_in, leaves) : lane_right(halo_in, leaves);
  if (LX != 64) vin = (RIGHT ? xl == 0 : xl == LX - 1) ? halo_in : vin;      // the first lane of the second half-row
  const uint32_t n0 = med3u(b0, vin + 1u, t0), n1 = med3u(b1, n0 + 1u, t1), n2 = med3u(b2, n1 + 1u, t2), n3 = med3u(b3, n2 + 1u, t3);
  if (TRACK) changed |= (n0 != t0) | (n1 != t1) | (n2 != t2) | (n3 != t3);
  t[RIGHT ? 0 : 3] = n0; t[RIGHT ? 1 : 2] = n1; t[RIGHT ? 2 : 1] = n2; t[RIGHT ? 3 : 0] = n3;
}

// The same idea down AND up the columns of a tile, in one phase: the rows of a column live in NB different bands (waves, or
// halves of waves), so every band publishes its four rows of each column as two clamped increments in LDS -- entered from
// above, entered from below; two waves then walk the columns once -- down and up -- through those functions from the tile's
// halo rows and leave every band the value that enters it; then every band takes its own rows downwards from what came
// from above, and upwards from what came from below.  Exact relaxation steps, like the row scan; what enters from the other
// bands is their state when the phase began.
// (r2, first form: a scan down and a scan up, each with its own barriers and with 0 .. NB - 1 dependent reads depending
// on the band -- the last band walked 15 bands while the others waited, twice per round: 4 of the 6.6 us of a tile run's
// rounds, tools/diag_relax_smooth.hip.  Second form: every band composed the NB - 1 others by itself, one barrier.
// tools/sim_tile_schedule.c, recipes "rdlu|L|" and "rlc|L|": same passes, tile runs and rounds either way.)
template <int NB, int TW, bool SPLIT>
__device__ __forceinline__ void scan_cols_both(patch_t &T, const patch_t &B, uint32_t *fn, const uint32_t *halo_top, const uint32_t *halo_bottom,
                                               int band, int xl) {      // fn: [2][NB][2][TW]: direction, band, (lo, hi)
  auto slot = [&](int dir, int k, int which) { return fn + (((size_t)dir * NB + k) * 2 + which) * TW + xl * RX_P; };
  {
    uint32_t lo[RX_P], hi[RX_P];
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {      // 0: entered from above, rows 0 .. 3; 1: from below, rows 3 .. 0
#pragma unroll
      for (int c = 0; c < RX_P; ++c) {
        uint32_t h = T[dir ? 3 : 0][c], l = B[dir ? 3 : 0][c];
#pragma unroll
        for (int k = 1; k < RX_P; ++k) {
          const int r = dir ? RX_P - 1 - k : k;
          h = med3u(B[r][c], h + 1u, T[r][c]);
          l = med3u(B[r][c], l + 1u, T[r][c]);
        }
        lo[c] = l; hi[c] = h;
      }
      *reinterpret_cast<u32x4_t *>(slot(dir, band, 0)) = u32x4_t{lo[0], lo[1], lo[2], lo[3]};
      *reinterpret_cast<u32x4_t *>(slot(dir, band, 1)) = u32x4_t{hi[0], hi[1], hi[2], hi[3]};
    }
  }
  __syncthreads();
  // What enters each band from above and from below is a chain through the bands' functions -- NB - 1 steps, but ONE chain
  // per column and direction, not one per band: wave 0 walks down, wave 1 walks up, a lane per four columns, and leaves in
  // the (lo) slot of every band the value that enters it.  (Every band composing the bands before it by itself: NB - 1 LDS
  // reads of 32 bytes in every lane -- 1 MB per round and tile at sixteen waves, 3 of a round's 9 us.)
  constexpr int LXc = TW / RX_P;      // lanes across a tile row
  {
    const int w = (int)(threadIdx.x >> 6), l = (int)(threadIdx.x & 63);
    if (w < 2 && l < LXc) {
      const int dir = w;
      const u32x4_t h4 = *reinterpret_cast<const u32x4_t *>(&(dir ? halo_bottom : halo_top)[l * RX_P]);
      uint32_t v0 = h4.x, v1 = h4.y, v2 = h4.z, v3 = h4.w;
#pragma unroll 4
      for (int i = 0; i < NB; ++i) {
        const int k = dir ? NB - 1 - i : i;
        uint32_t *lo_p = fn + (((size_t)dir * NB + k) * 2 + 0) * TW + l * RX_P, *hi_p = lo_p + TW;
        const u32x4_t l4 = *reinterpret_cast<const u32x4_t *>(lo_p);
        const u32x4_t g4 = *reinterpret_cast<const u32x4_t *>(hi_p);
        *reinterpret_cast<u32x4_t *>(lo_p) = u32x4_t{v0, v1, v2, v3};      // what enters band k
        v0 = med3u(l4.x, v0 + RX_P, g4.x); v1 = med3u(l4.y, v1 + RX_P, g4.y);
        v2 = med3u(l4.z, v2 + RX_P, g4.z); v3 = med3u(l4.w, v3 + RX_P, g4.w);
      }
    }
  }
  __syncthreads();
  const u32x4_t d4 = *reinterpret_cast<const u32x4_t *>(slot(0, band, 0));
  const u32x4_t u4 = *reinterpret_cast<const u32x4_t *>(slot(1, band, 0));
  const uint32_t vd[RX_P] = {d4.x, d4.y, d4.z, d4.w}, vu[RX_P] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
  for (int c = 0; c < RX_P; ++c) {
    uint32_t n = vd[c];
#pragma unroll
    for (int r = 0; r < RX_P; ++r) { n = med3u(B[r][c], n + 1u, T[r][c]); T[r][c] = n; }
    n = vu[c];
#pragma unroll
    for (int r = RX_P - 1; r >= 0; --r) { n = med3u(B[r][c], n + 1u, T[r][c]); T[r][c] = n; }
  }
  // (no barrier here: two lie between this phase and the next write of the functions -- the end of the round's free part
  // and the checked sweep's)
}

// ---- the pieces of a tile run that k_relax, k_relax0_tall and k_relax_strips_tall share -------------------------------------
//
// PH: rows of a lane's patch (ws_relax_patch.hpp).  A vector that a piece changes goes in by value and comes back as its
// result: as a u32x4_t & it changed what the callers compile to (the paragraph "Four blocks of a tile run are NOT here",
// after seed_stamps, has the figures of everything that could not be shared).
constexpr int SEAM_PY = RX_NW * RX_P, SEAM_PX = RX_TW;      // the grid whose seams are repaired and whose tiles are flagged: 256 x 32

// What every launch does first: the first wave of workgroup 0 clears the next pass's convergence slot, and thread 0 the length
// and the ticket of the tile list that pass + 2 counts up from (this launch reads the list of `pass` and may append to the
// list of pass + 1; k_relax_list appends only after this launch has ended).
__device__ __forceinline__ void launch_prologue(const PassFlags &pf, uint32_t *tile_list, uint32_t pass) {
  if (blockIdx.x == 0 && threadIdx.x < NSTRIPE)
    pf.edge_changed[((pass + 1) % COUNTER_RING) * FLAG_SLOT + threadIdx.x * STRIPE_STRIDE] = 0;
  if (tile_list && blockIdx.x == 0 && threadIdx.x == 0) { tile_list[(pass + 2) & 3u] = 0u; tile_list[4 + ((pass + 2) & 3u)] = 0u; }
}

// Does tile (tx, ty) of a launch with one tile per workgroup have anything to do?  (Workgroup uniform.)
template <int SEAM, int SEAM_PITCH, int TW, int TH>
__device__ __forceinline__ bool tile_has_work(int tx, int ty, int H, int W, int shifted, int otherX, int otherY, uint32_t pass,
                                              const uint32_t *stamps_prev, const uint32_t *stamps_cur, const PassFlags &pf) {
  // (a seam whose tiles on both sides have asked for a re-run already -- pass 0 stopped at its round cap there: a smooth
  // map -- is left to them: on such maps the repair would be 64 us of sweeps that the re-runs undo)
  if (SEAM == 1) {
    if (tx * TW >= W || (ty + 1) * SEAM_PITCH >= H) return false;
    // (a tile that asked for its re-run is work for pass 2: this pass must not look like a fixpoint to the host -- pass 0
    // cannot say so itself, its launch clears this pass's convergence slot)
    const int fy = (ty + 1) * (SEAM_PITCH / SEAM_PY) - 1;
    const bool fa = stamps_cur[((size_t)fy * otherX + tx + 1) * 4 + 2] == pass + 1, fb = stamps_cur[((size_t)(fy + 1) * otherX + tx + 1) * 4 + 2] == pass + 1;
    if ((fa || fb) && threadIdx.x == 0) pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT + (blockIdx.x % NSTRIPE) * STRIPE_STRIDE] = 1u;
    if (fa && fb) return false;
  } else if (SEAM == 2) {
    if (ty * TH - (shifted ? TH / 2 : 0) >= H || (tx * 32 + 1) * SEAM_PX >= W) return false;
    const int l = threadIdx.x & 63;
    const int sxl = (tx * 32 + (l >> 1) + 1) * SEAM_PX;
    const bool settled = sxl >= W || stamps_cur[((size_t)((ty * TH) / SEAM_PY) * otherX + (sxl / SEAM_PX - 1 + (l & 1)) + 1) * 4 + 2] == pass + 1;
    if (__builtin_amdgcn_ballot_w64(settled) == ~0ull) return false;
  }
  else if (tx * TW - (shifted ? TW / 2 : 0) >= W || ty * TH - (shifted ? TH / 2 : 0) >= H) return false;
  if (SEAM == 0 && pass != 0) {       // the same test as relax_todo, on scalars
    bool run = false;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int qx = q & 1, qy = q >> 1;
      const int oi = tx + qx - (shifted ? 1 : 0), oj = ty + qy - (shifted ? 1 : 0);
      const bool ok = oi >= 0 && oi < otherX && oj >= 0 && oj < otherY;
      const size_t ot = (size_t)(ok ? oj : 0) * otherX + (ok ? oi : 0);
      const uint32_t st = stamps_prev[ot * 4 + (3 - q)];
      run |= ok && st == pass;
    }
    if (!run) return false;
  }
  return true;
}

// Seed bits (or labels) as loaded -> stamps: seed = coloured pixel = stamp 0, everything else never coloured.
// col: the lane's halo column; halo_row: its four pixels of the tile's halo row (returned).
template <int PH>
__device__ __forceinline__ u32x4_t seed_stamps(uint32_t (&T)[PH][RX_P], uint32_t (&col)[PH], u32x4_t halo_row) {
#pragma unroll
  for (int r = 0; r < PH; ++r) {
#pragma unroll
    for (int c = 0; c < RX_P; ++c) T[r][c] = T[r][c] ? 0u : KEY_INF;
    col[r] = col[r] ? 0u : KEY_INF;
  }
  halo_row.x = halo_row.x ? 0u : KEY_INF; halo_row.y = halo_row.y ? 0u : KEY_INF;
  halo_row.z = halo_row.z ? 0u : KEY_INF; halo_row.w = halo_row.w ? 0u : KEY_INF;
  return halo_row;
}

// Four blocks of a tile run are NOT here and stay written out in each of the three kernels: the border and slice-wall masks,
// the band rows' way through sRow (publish and fetch), the end-of-round vote on s_flag, and the patch write-back with its
// ring-carry test.  As __forceinline__ functions over the patch by reference each of them changed the register allocation
// of the kernels that call it (product build; profiles/relax_kernel_resources.txt has the parent's table):
//   band rows + vote   plain k_relax variants 68 -> 80 VGPRs with 1 - 13 spilled, occupancy 7 -> 6; k_relax0_tall 109 -> 128
//                      VGPRs with 51 - 54 spilled; k_relax_strips_tall 96 - 113 spilled;
//   write-back         plain variants 75 - 80 VGPRs, the chunked variant 6 -> 18 spilled, k_relax0_tall 109 -> 121 VGPRs;
//   masks              of the resources only SGPRs moved (+2 .. +10, SGPR spills -22 .. +15), but every variant's instruction
//                      count did (-199 .. +143 over the forms tried); with the masks and a row form of `matters` shared,
//                      the headline median of three alternating runs lay 1.0 % under the range of the parent's three.
// Also tried for rows, vote and write-back: the rows passed by value as u32x4_t (k_relax0_tall 127 VGPRs; new spills in
// the strips, the chunked and the scan variants), the patch by non-const reference, the vector built element by element.
// In the tall kernels rows and vote ARE lambdas, as in the parent.  A macro -- the same tokens in the kernel, so the same
// code in k_relax at least -- was not tried and is the obvious next attempt.  The optimised IR shows the
// patch rows as <4 x i32> values from load to store in the failing forms (the 16-byte stores pull them together); why a
// function brings that about and the same statements written in the kernel do not is not established.  A change to one
// of the four is a change in three places until the kernels have registers to spare.

// A changed border pixel only MATTERS to the tile across the border when it can lower the pixel it touches there:
// new stamp + 1 < that pixel's stamp -- which this tile holds, as its halo.  (The halo is as old as the tile's load: the
// pixel can only have fallen since, so the test errs on the side of flagging.)  On smooth maps a third to a half of the
// late tile runs changed nothing at all (tools/sim_tile_schedule.c, SIM_CHANGED): flagged by a neighbour whose front
// had not caught up with theirs.
__device__ __forceinline__ bool matters(uint32_t before, uint32_t now, uint32_t across) { return before != now && now + 1u < across; }

// profiling only: striped counters, one per 64-byte line -- tile runs in quarter tiles of 256 x 32 (a 256 x 8 band is one;
// ws_segment.hip divides), and their rounds
__device__ __forceinline__ void count_tile_run(const PassFlags &pf, uint32_t stripe, uint32_t quarter_tiles, uint32_t rounds) {
  if (pf.stats) {
    atomicAdd(&pf.stats[stripe], quarter_tiles);
    atomicAdd(&pf.stats[FLAG_SLOT + stripe], rounds);
  }
}

// ---- k_relax: the ordinary tile run, the bands (SEAM 1), the 32-row strips (SEAM 2), and the workers of the tile queue
// (PERSIST 1: first come, PERSIST 2: in flood order; ws_relax_queue.hpp) ------------------------------------------------------
template <int NW, bool CHUNKED, bool SCAN, bool LITE, bool SPLIT = false, int SEAM = 0, int PERSIST = 0, int SEAM_PITCH = 32>
__global__ __launch_bounds__(64 * NW, SCAN ? 4 : 6) void k_relax(      // the scan variant trades occupancy (few tiles run there) for registers
const uint8_t *__restrict__ img, size_t img_stride, uint32_t *keys,
                                                      int H, int W, int tilesX, int tilesY, int otherX, int otherY,
                                                      int shifted, int chunk, uint32_t max_level, uint32_t pass,
                                                      const uint32_t *__restrict__ stamps_prev, uint32_t *stamps_cur,
                                                      PassFlags pf, uint32_t max_iters,
                                                      const uint32_t *__restrict__ seed_labels, int seed_bits, int SH, int check_carry,
                                                      int pad, uint32_t *tile_list, int use_list, int read_same,
                                                      int write_same, uint32_t list_cap, int append_next) {
  // SH: rows per slice.  A batch of independent slices is one plane of H = S * SH rows in which the first and last row
  // of every slice are image-border rows (never flooded: walls between the slices); SH == H for a single image.
  // SPLIT (the same-grid passes of a long-range flood): a wave is TWO bands of half the width -- lanes 0..31 hold four rows
  // of 128 columns, lanes 32..63 the four rows below them -- so the tile is 128 x 64 instead of 256 x 32.  On a smooth map
  // the number of passes is set by how far a pass carries a flood vertically, and a pass costs its tile runs whatever
  // their shape: tools/sim_tile_schedule.c has a quarter to a third fewer of both for the squarer tile.
  constexpr int LX = SPLIT ? 32 : 64;             // lanes across a tile row
  constexpr int NB = SPLIT ? 2 * NW : NW;         // bands of RX_P rows
  constexpr int TW = LX * RX_P, TH = NB * RX_P;
  // SEAM (relax_pass, seam repair: the pass after pass 0 of a transform that starts from its seeds).  What a pass leaves
  // wrong lies within a few pixels of its tile borders, so the pass after pass 0 only has to look along those:
  //   SEAM 1  a tile is 256 x 8 pixels (NW = 2) astride a horizontal seam of the 256 x 32 grid, rows 32 (ty + 1) - 4 ...;
  //   SEAM 2  a tile is a 32-row slice of 32 vertical seams: lanes 2j and 2j + 1 hold the 8 columns astride seam
  //           32 tile_x + j + 1 (x = 256 times that), and no stamp crosses from one lane PAIR to the next.
  // A seam tile iterates to its fixpoint and raises, in the stamp word that the next pass of the anchored grid reads, the
  // flag of every 256 x 32 tile that holds a pixel next to a changed outer row or column of it.  (otherX: that array's pitch.)
  // (SEAM_PITCH, SEAM 1: rows between two horizontal seams -- 64 after pass 0 on 256 x 64 tiles, k_relax0_tall.  The flags
  // stay those of the 256 x 32 tiles: seam row 64 (ty + 1) is the border between tile rows seam_fy and seam_fy + 1.)
  constexpr int SEAM_HALF = SEAM == 1 ? TH / 2 : 4;
  static_assert(SEAM_PITCH % SEAM_PY == 0, "a seam is a border of the 256 x 32 grid");
  // row 0: halo above the tile; rows 1+2w / 2+2w: top / bottom row of band w; last row: halo below
  __shared__ __attribute__((aligned(16))) uint32_t sRow[2 * NB + 2][TW];
  // the tile border as loaded (top row, bottom row, left column, right column): compared with the
  // final values to tell which tile edges changed; parked in LDS to keep the VGPR count at 80
  __shared__ __attribute__((aligned(16))) uint32_t sInitRow[2][TW];
  __shared__ uint32_t sInitCol[2][TH];
  __shared__ uint32_t s_edges;
  // list mode: the tiles this workgroup's runs want in the next pass's list, handed in together -- a "queued" exchange
  // and a list ticket are two dependent atomic round trips, 3 of the 4.5 us a tile run's epilogue took with seven of the
  // eight waves idle (tools/diag_relax_smooth.hip); a workgroup runs ~5 tiles in a heavy pass and now pays them once
  __shared__ uint32_t s_cand[RX_CAND];
  __shared__ uint32_t s_ncand;
  __shared__ uint32_t s_next[2];             // list mode: the entry this workgroup takes after the current one (by run parity)
  // "some lane changed in iteration k" lives in slot k % 3: written before barrier k, read after it,
  // cleared by thread 0 for iteration k + 2 -- one barrier per iteration instead of the three a
  // __syncthreads_or costs
  __shared__ uint32_t s_flag[3];
  __shared__ uint64_t s_sum[64 * NW];        // per-lane patch checksum taken at load time (parked: VGPRs are at the cap)
  // long-range columns (SCAN): every band's four rows of a column as one clamped increment (lo, hi)
  __shared__ __attribute__((aligned(16))) uint32_t sFn[2][SCAN ? NB : 1][2][SCAN ? TW : 4];

  launch_prologue(pf, tile_list, pass);
  // (XCD-aware: consecutive workgroups go to different XCDs; see xcd_span_index)
  // A chunk is `chunk` tiles one grid size apart, not neighbours: on a smooth map the tiles that still
  // run line up along a front, and four neighbours in one workgroup ran one after the other.
  const int first = (int)xcd_span_index(blockIdx.x, gridDim.x);
  const int stride = (int)gridDim.x;
  unsigned long long todo = 1;
  // list mode (late passes of a long-range flood): the tiles to run were compacted by k_relax_list; workgroup b takes
  // entries b, b + gridDim.x, ... -- no workgroup is launched for a tile that has nothing to do, none owns two busy ones
  uint32_t entry = blockIdx.x, n_entries = 0, first_entry = 0, runs_done = 0;
  // PERSIST: the queue (ws_relax_queue.hpp)
  const RelaxQueue q = relax_queue(tile_list, list_cap, (uint32_t)(tilesX * tilesY), max_level);
  __shared__ uint32_t s_qtile, s_qbucket, s_handoff;
  __shared__ uint32_t s_sidemin[4];      // PERSIST == 2: the smallest new stamp that matters across the top / bottom / left / right border
  unsigned long long q_t0 = 0;
  uint32_t q_wait = 0, q_polls = 0;
#ifdef WS_TUNING
  uint32_t q_ph[4] = {0, 0, 0, 0};
  unsigned long long q_tp = 0;      // (WS_QPHASE)
  const unsigned long long q_c0 = PERSIST ? __builtin_amdgcn_s_memtime() : 0ull;
#endif
  if (PERSIST) {
    q_t0 = __builtin_amdgcn_s_memrealtime();
    // whatever this launch does, the passes after it look at every tile again: tell the host that they have to run
    if (blockIdx.x == 0 && threadIdx.x == 0 && __hip_atomic_load(q.q_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u)
      pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT] = 1u;
  } else if (CHUNKED && use_list) {
    // (the workgroup's first entry is asked for together with the list length, not after it: one memory round trip less
    // at the head of every tile run of a thin pass, which IS such a pass's length)
    first_entry = tile_list[RL_HDR + (pass & 1u) * list_cap + min(entry, list_cap - 1u)];
    n_entries = tile_list[pass & 3u];
    if (entry >= n_entries) return;
  } else if (CHUNKED && !PERSIST) {
    todo = relax_todo<TW, TH>(first, stride, chunk, H, W, tilesX, tilesY, otherX, otherY, shifted, pass, stamps_prev, read_same);
    if (todo == 0) return;
  } else if (!PERSIST) {
    if (!tile_has_work<SEAM, SEAM_PITCH, TW, TH>(first % tilesX, first / tilesX, H, W, shifted, otherX, otherY, pass, stamps_prev, stamps_cur, pf)) return;
  }
  if (threadIdx.x == 0) { s_ncand = 0; if (PERSIST == 2) s_handoff = 0; }      // (read again only after the first tile's barriers)
  for (;;) {
  // which tile
  uint32_t q_tile = 0;
  if (PERSIST == 2) q_tile = queue_take_flood_order(q, q_t0, q_wait, q_polls, use_list, s_qtile, s_qbucket, s_handoff, s_sidemin);
  else if (PERSIST) q_tile = queue_take_first_come(q, q_t0, q_wait, q_polls, s_qtile);
  if (PERSIST) {
    if (q_tile == 0) {           // workgroup uniform: the queue has run dry (or the time budget is spent)
      if (threadIdx.x == 0) {
        atomicAdd(tile_list + RLQ_WAIT, q_wait);
        atomicAdd(tile_list + RLQ_LIFE, (uint32_t)(__builtin_amdgcn_s_memrealtime() - q_t0));
        atomicAdd(tile_list + RLQ_POLLS, q_polls);
#ifdef WS_TUNING
        for (int k = 0; k < 4; ++k) atomicAdd(tile_list + RLQ_PHASE + k, q_ph[k]);
        atomicAdd(tile_list + RLQ_PHASE + 4, (uint32_t)((__builtin_amdgcn_s_memtime() - q_c0) >> 8));      // shader cycles / 256
#endif
      }
      break;
    }
  }
  // re-derived per tile on purpose (the asm hides the value from loop-invariant hoisting): hoisted per-lane addresses
  // are more registers held across the tile loop, and the chunked variant is past the 80-VGPR cap as it is -- it spills
  // 6 VGPRs to 28 B/lane of scratch (profiles/relax_kernel_resources.txt)
  int tid = threadIdx.x;
  if (CHUNKED) asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  const int xl = SPLIT ? lane & 31 : lane;                                      // column block of the tile row
  const int band = SPLIT ? (tid >> 6) * 2 + (lane >> 5) : tid >> 6;             // four-row band of the tile
  const int tile = PERSIST ? (int)(q_tile - 1u)
                           : (CHUNKED ? (use_list ? (int)(entry == blockIdx.x ? first_entry : tile_list[RL_HDR + (pass & 1u) * list_cap + entry]) : first + (int)__builtin_ctzll(todo) * stride) : first);
  const int tile_x = tile % tilesX, tile_y = tile / tilesX;
  const int x0 = SEAM ? tile_x * TW : tile_x * TW - (shifted ? TW / 2 : 0);
  const int y0 = SEAM == 1 ? (tile_y + 1) * SEAM_PITCH - SEAM_HALF : tile_y * TH - (shifted ? TH / 2 : 0);
  const int seam_fy = (tile_y + 1) * (SEAM_PITCH / SEAM_PY) - 1;      // SEAM 1: the 256 x 32 tile row above the seam
  const int seam_x = (tile_x * 32 + (lane >> 1) + 1) * SEAM_PX;      // SEAM 2: this lane pair's seam (outside the plane: no seam)

  WS_STAMP(0);
  WS_QPHASE0;
  const int gx0 = SEAM == 2 ? (seam_x < W ? seam_x - SEAM_HALF + (lane & 1) * RX_P : W) : x0 + xl * RX_P, gyb = y0 + band * RX_P;
  if (tid == 0) { s_edges = 0; s_flag[0] = 0; s_flag[1] = 0; s_flag[2] = 0; }
  // List mode: entries are handed out by ticket, not in strides of the grid -- tile runs last 8 to 20 us, and with a fixed
  // share a pass ended with most workgroups gone and a few still on their third tile.  The ticket for the NEXT entry is
  // drawn now and read after the run: its round trip hides behind the tile.
  if (!PERSIST && CHUNKED && use_list && tid == 0) s_next[runs_done & 1u] = gridDim.x + atomicAdd(&tile_list[4 + (pass & 3u)], 1u);

  // ---- load phase ---------------------------------------------------------------------------
  uint32_t T[RX_P][RX_P], B[RX_P][RX_P], halo[RX_P];
  // fast path (workgroup uniform): the tile lies inside the image in x and image rows can be read
  // as aligned dwords -> one 16-byte stamp load and one 4-byte image load per lane and row
  // (patches outside the plane read a clamped address and are masked afterwards: with W % 4 == 0 a
  // patch is either wholly inside or wholly outside)
  // (pad: the image is the caller's unpadded one, read through padded_img_index -- byte loads)
  const bool fast = !pad && W >= RX_P && ((SEAM != 2 && x0 >= 0 && x0 + TW <= W) || (W & 3) == 0) &&
                    ((reinterpret_cast<uintptr_t>(img) | img_stride) & 3u) == 0 && img_stride <= 0xFFFFFFFFull;
  // Index arithmetic of the fast paths in 32 bits where the plane allows it: the first form of these loads spent 22 vector
  // instructions per patch row on addresses, five of them 64-bit multiplies (v_mad_i64_i32, v_mul_lo_u32: quarter rate).
  const uint32_t stride32 = (uint32_t)img_stride;
  const bool dims24 = (uint32_t)W < (1u << 24) && (uint32_t)H < (1u << 24);      // kernel uniform: row * W as v_mul_u32_u24
  const int gxc0 = min(max(gx0, 0), max(W - RX_P, 0));
  // tile halo columns: the left half of a row's lanes fetch the column left of the tile, the right half the one right
  // of it; only the first / last lane of a row ever use the value (as the DPP `old` operand)
  // (SEAM 2: every lane is the first or the last of its pair's row)
  const int xh_raw = SEAM == 2 ? ((lane & 1) ? gx0 + RX_P : gx0 - 1) : (xl < LX / 2 ? x0 - 1 : x0 + TW);
  const int xh = min(max(xh_raw, 0), W - 1);
  const bool xh_ok = SEAM == 2 ? (xh_raw >= 0 && xh_raw < W && seam_x < W) : (xl < LX / 2 ? x0 > 0 : x0 + TW < W);
  const int gy_halo_raw = band == 0 ? y0 - 1 : y0 + TH;
  const int gy_halo = min(max(gy_halo_raw, 0), H - 1);
  u32x4_t halo_row;
  // pass 0 of a whole-image transform reads the freshly painted LABEL plane instead of a stamp
  // plane (seed = coloured pixel = stamp 0, everything else never-coloured): nobody has to fill the
  // stamp plane first, this pass writes all of it
  // (seed_bits: the "plane" is one bit per pixel instead -- the side table of a strictly increasing
  // seed list, ws_kernels.hip; only offered for W % 4 == 0, so a patch row is one nibble of one word)
  const bool from_labels = seed_labels != nullptr;
  const uint32_t *ksrc = from_labels ? seed_labels : keys;
  if (fast && seed_bits) {
    uint32_t iv[RX_P];
#pragma unroll
    for (int r = 0; r < RX_P; ++r) {
      const uint32_t gyc = (uint32_t)min(max(gyb + r, 0), H - 1);
      // (a bit plane exists only for planes of fewer than 2^31 pixels: pixel indices fit 32 bits)
      const uint32_t ro = dims24 ? __umul24(gyc, (uint32_t)W) : gyc * (uint32_t)W;
      const uint32_t p = ro + (uint32_t)gxc0, ph_ = ro + (uint32_t)xh;
      const uint32_t nib = ksrc[p >> 5] >> (p & 31u);
      iv[r] = *reinterpret_cast<const uint32_t *>(img + ((unsigned long long)gyc * stride32 + (uint32_t)gxc0));
      halo[r] = (ksrc[ph_ >> 5] >> (ph_ & 31u)) & 1u;
      T[r][0] = nib & 1u; T[r][1] = nib & 2u; T[r][2] = nib & 4u; T[r][3] = nib & 8u;
    }
    patch_bases(iv, B, max_level);
    const uint32_t p = (dims24 ? __umul24((uint32_t)gy_halo, (uint32_t)W) : (uint32_t)gy_halo * (uint32_t)W) + (uint32_t)gxc0;
    const uint32_t nib = ksrc[p >> 5] >> (p & 31u);
    halo_row = u32x4_t{nib & 1u, nib & 2u, nib & 4u, nib & 8u};
  } else if (fast) {
    u32x4_t kv[RX_P];
    uint32_t iv[RX_P];
#pragma unroll
    for (int r = 0; r < RX_P; ++r) {
      const int gyc = min(max(gyb + r, 0), H - 1);
      iv[r] = *reinterpret_cast<const uint32_t *>(img + ((unsigned long long)(uint32_t)gyc * stride32 + (uint32_t)gxc0));
      if (PERSIST && !(use_list & 1)) {      // (PERSIST: use_list carries the tuning build's A/B bits -- 1: plain stamp accesses, 2: slow polls)
        coh_load4(kv[r], ksrc + (size_t)gyc * W + gxc0);
        coh_load1(halo[r], ksrc + (size_t)gyc * W + xh);
      } else {
        kv[r] = *reinterpret_cast<const u32x4_t *>(ksrc + (size_t)gyc * W + gxc0);
        halo[r] = ksrc[(size_t)gyc * W + xh];
      }
    }
    if (PERSIST && !(use_list & 1)) {
      coh_load4(halo_row, ksrc + (size_t)gy_halo * W + gxc0);
      asm volatile("s_waitcnt vmcnt(0)"
                   : "+v"(kv[0]), "+v"(kv[1]), "+v"(kv[2]), "+v"(kv[3]), "+v"(halo_row), "+v"(halo[0]), "+v"(halo[1]), "+v"(halo[2]), "+v"(halo[3])
                   :
                   : "memory");
    } else {
      halo_row = *reinterpret_cast<const u32x4_t *>(ksrc + (size_t)gy_halo * W + gxc0);
    }
#pragma unroll
    for (int r = 0; r < RX_P; ++r) {
      T[r][0] = kv[r].x; T[r][1] = kv[r].y; T[r][2] = kv[r].z; T[r][3] = kv[r].w;
    }
    patch_bases(iv, B, max_level);
  } else {
#pragma unroll
    for (int r = 0; r < RX_P; ++r) {
      const int gyc = min(max(gyb + r, 0), H - 1);
#pragma unroll
      for (int c = 0; c < RX_P; ++c) {
        const int gxc = min(max(gx0 + c, 0), W - 1);
        T[r][c] = plane_or_bit(ksrc, (size_t)gyc * W + gxc, seed_bits);
        const uint32_t v = img[pad ? padded_img_index(gyc, gxc, W, SH, img_stride) : (size_t)gyc * img_stride + gxc];
        B[r][c] = v <= max_level ? ((v << 24) | 1u) : KEY_INF;
      }
      halo[r] = plane_or_bit(ksrc, (size_t)gyc * W + xh, seed_bits);
    }
    halo_row.x = plane_or_bit(ksrc, (size_t)gy_halo * W + min(max(gx0 + 0, 0), W - 1), seed_bits);
    halo_row.y = plane_or_bit(ksrc, (size_t)gy_halo * W + min(max(gx0 + 1, 0), W - 1), seed_bits);
    halo_row.z = plane_or_bit(ksrc, (size_t)gy_halo * W + min(max(gx0 + 2, 0), W - 1), seed_bits);
    halo_row.w = plane_or_bit(ksrc, (size_t)gy_halo * W + min(max(gx0 + 3, 0), W - 1), seed_bits);
  }
  if (from_labels) halo_row = seed_stamps(T, halo, halo_row);
  // (bases: only interior pixels with img <= max level can ever be flooded (lib.rs:220-224); everything else, and every
  // seed (stamp 0 < base), is pinned at its current stamp: b = t -- patch_bases above, the border masks and the min below)
  // Workgroup uniform: the tile and its halo ring lie strictly inside the image (and the image is not a stack of
  // slices) -- every pixel is in the plane and interior, none of the masks below can bite.  These kernels are VALU-bound
  // (VALUBusy 76-84 %, profiles/), and the masks were ~8 ops per pixel of a tile run's ~60.
  const bool inner = SEAM != 2 && SH == H && x0 >= 1 && x0 + TW <= W - 1 && y0 >= 1 && y0 + TH <= H - 1;
  if (!inner) {
    // row inside its slice: the four rows of a patch are all above the plane or all from row 0 on
    const int ry0 = (SH == H || gyb < 0) ? gyb : gyb % SH;
#pragma unroll
    for (int r = 0; r < RX_P; ++r) {
      const int gy = gyb + r;
      const int ry = ry0 + r >= SH ? ry0 + r - SH : ry0 + r;
      const bool row_ok = gy >= 0 && gy < H, row_int = ry >= 1 && ry < SH - 1 && gy < H;
#pragma unroll
      for (int c = 0; c < RX_P; ++c) {
        const int gx = gx0 + c;
        if (!(row_ok && gx >= 0 && gx < W)) T[r][c] = KEY_INF;
        if (!(row_int && gx >= 1 && gx < W - 1)) B[r][c] = KEY_INF;
      }
      if (!(row_ok && xh_ok)) halo[r] = KEY_INF;
    }
    const bool ok = gy_halo_raw >= 0 && gy_halo_raw < H;
    if (!(ok && gx0 + 0 >= 0 && gx0 + 0 < W)) halo_row.x = KEY_INF;
    if (!(ok && gx0 + 1 >= 0 && gx0 + 1 < W)) halo_row.y = KEY_INF;
    if (!(ok && gx0 + 2 >= 0 && gx0 + 2 < W)) halo_row.z = KEY_INF;
    if (!(ok && gx0 + 3 >= 0 && gx0 + 3 < W)) halo_row.w = KEY_INF;
  }
#pragma unroll
  for (int r = 0; r < RX_P; ++r)
#pragma unroll
    for (int c = 0; c < RX_P; ++c) B[r][c] = min(B[r][c], T[r][c]);
  // The columns left / right of the patch, one register per patch row, PERSISTENT: a sweep refreshes them with one DPP
  // wave shift each, whose `old` operand is the register itself -- lane 0 (lane 63) has no neighbour lane and keeps what
  // it holds, the tile's halo column, for the whole tile run.  (Passing the halo as `old` every time cost a v_mov per
  // shift to set the destination up: 16 of the ~80 vector instructions of a sweep.)
  // (SPLIT: lane 32 is the first lane of the lower band and lane 31 the last of the upper one: the shift hands them a
  // value from the other band, which a select replaces with their halo column again)
  uint32_t Lh[RX_P], Rh[RX_P];
#pragma unroll
  for (int r = 0; r < RX_P; ++r) { Lh[r] = halo[r]; Rh[r] = halo[r]; }
  // the tile's halo column as every lane of the row sees it: the register of the row's first / last lane
  auto row_first = [&](uint32_t v) -> uint32_t {
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 0);
    if (!SPLIT) return a;
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)v, 32);
    return lane < 32 ? a : b;
  };
  auto row_last = [&](uint32_t v) -> uint32_t {
    const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
    if (!SPLIT) return b;
    const uint32_t a = (uint32_t)__builtin_amdgcn_readlane((int)v, 31);
    return lane < 32 ? a : b;
  };
  auto refresh_columns = [&]() {
#pragma unroll
    for (int r = 0; r < RX_P; ++r) {
      Lh[r] = lane_left(Lh[r], T[r][3]);
      Rh[r] = lane_right(Rh[r], T[r][0]);
      if (SPLIT) { Lh[r] = lane == 32 ? halo[r] : Lh[r]; Rh[r] = lane == 31 ? halo[r] : Rh[r]; }
      if (SEAM == 2) { Lh[r] = (lane & 1) ? Lh[r] : halo[r]; Rh[r] = (lane & 1) ? halo[r] : Rh[r]; }
    }
  };
  {
    if (band == 0) *reinterpret_cast<u32x4_t *>(&sRow[0][xl * RX_P]) = halo_row;
    if (band == NB - 1) *reinterpret_cast<u32x4_t *>(&sRow[2 * NB + 1][xl * RX_P]) = halo_row;
    *reinterpret_cast<u32x4_t *>(&sRow[1 + 2 * band][xl * RX_P]) = u32x4_t{T[0][0], T[0][1], T[0][2], T[0][3]};
    *reinterpret_cast<u32x4_t *>(&sRow[2 + 2 * band][xl * RX_P]) = u32x4_t{T[3][0], T[3][1], T[3][2], T[3][3]};
  }
  if (band == 0) *reinterpret_cast<u32x4_t *>(&sInitRow[0][xl * RX_P]) = u32x4_t{T[0][0], T[0][1], T[0][2], T[0][3]};
  if (band == NB - 1) *reinterpret_cast<u32x4_t *>(&sInitRow[1][xl * RX_P]) = u32x4_t{T[3][0], T[3][1], T[3][2], T[3][3]};
  uint32_t init_col[RX_P];          // SEAM 2: this lane's outer column as loaded (every lane has one)
  if (SEAM == 2) {
#pragma unroll
    for (int r = 0; r < RX_P; ++r) init_col[r] = T[r][(lane & 1) ? 3 : 0];
  } else if (xl == 0 || xl == LX - 1) {
#pragma unroll
    for (int r = 0; r < RX_P; ++r) sInitCol[xl == 0 ? 0 : 1][band * RX_P + r] = T[r][xl == 0 ? 0 : 3];
  }
  __syncthreads();
  WS_STAMP(1);
  WS_QPHASE(0);

  // ---- relaxation ---------------------------------------------------------------------------
  // One round = three free-running sweeps (down, right, up), a barrier that publishes the band
  // boundary rows, then ONE checked sweep (left) on fresh neighbours.  The fixpoint is reached
  // exactly when that checked sweep changes nothing in the whole tile: every pixel has then been
  // evaluated against final neighbour values.  Only the checked sweep pays for change tracking, and
  // a tile that was already converged leaves after 4 sweeps instead of 8.
  if (!from_labels) {                // (kernel uniform: the pass that creates the stamp plane writes every patch anyway)
    uint64_t sum_before = 0;         // stamps only ever decrease: a 64-bit patch sum tells "changed" exactly
#pragma unroll
    for (int r = 0; r < RX_P; ++r)
#pragma unroll
      for (int c = 0; c < RX_P; ++c) sum_before += T[r][c];
    s_sum[tid] = sum_before;
  }
  uint32_t iters = 0;
  WS_ACC_DECL;
  bool unfinished = max_iters == 0;      // left before the checked sweep came back clean (round cap)
  // the three free sweeps of a round, then the band boundary rows are published
  auto free_sweeps = [&](uint32_t round) {
    bool untracked = false;
    uint32_t up[RX_P], dn[RX_P];
    {
      const u32x4_t up4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band][xl * RX_P]);
      const u32x4_t dn4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band + 3][xl * RX_P]);
      up[0] = up4.x; up[1] = up4.y; up[2] = up4.z; up[3] = up4.w;
      dn[0] = dn4.x; dn[1] = dn4.y; dn[2] = dn4.z; dn[3] = dn4.w;
    }
    if (!SCAN) {
      // (SEAM 1, the bands: from the second round on the free part of a round is the sweep up alone -- k_relax0_tall has the
      // recipe, the replay and why the fixpoint is the same)
      if (!(SEAM == 1 && round > 1)) {
        refresh_columns();
        sweep_rows<false, true>(T, B, up, dn, Lh, Rh, untracked);       // down
        refresh_columns();
        sweep_cols<false, true>(T, B, up, dn, Lh, Rh, untracked);       // right
      }
      refresh_columns();
      sweep_rows<false, false>(T, B, up, dn, Lh, Rh, untracked);      // up
    } else {
      // The long-range variant: exact scans right, left, then down and up in one phase, instead of the three sweeps (which move a stamp by one
      // patch; with them as well a round cost a quarter more and the passes were no fewer: gpurun_out/r2w/skipfree.log).
      // The checked sweep that follows still sees every pixel's four neighbours: the exit test is the same.
      WS_ACC_T0;
#pragma unroll
      for (int r = 0; r < RX_P; ++r) scan_row<false, true, LX>(T[r], B[r], row_first(Lh[r]), xl, untracked);
#pragma unroll
      for (int r = 0; r < RX_P; ++r) scan_row<false, false, LX>(T[r], B[r], row_last(Rh[r]), xl, untracked);
      WS_ACC(0);
      scan_cols_both<NB, TW, SPLIT>(T, B, &sFn[0][0][0][0], sRow[0], sRow[2 * NB + 1], band, xl);
      WS_ACC(1);
    }
    *reinterpret_cast<u32x4_t *>(&sRow[1 + 2 * band][xl * RX_P]) = u32x4_t{T[0][0], T[0][1], T[0][2], T[0][3]};
    *reinterpret_cast<u32x4_t *>(&sRow[2 + 2 * band][xl * RX_P]) = u32x4_t{T[3][0], T[3][1], T[3][2], T[3][3]};
    __syncthreads();
  };
  // LITE (passes >= 2: few pixels are still wrong, many flagged tiles need no change at all): the checked sweep comes
  // FIRST and the free sweeps after it -- a tile that is already a fixpoint leaves after one sweep instead of four.
  // Same sequence of sweeps as the other order minus the first three; the exit test is the same.
  for (; max_iters != 0;) {
    ++iters;
    // (chunk == 3, pass 0 of a seam-repair transform: after two full rounds a tile of the bench field has two or three stamps
    // left to settle -- from the third round on a round is its checked sweep alone, one sweep to settle them and one to see
    // that nothing moves, instead of a round of four that finds nothing to do)
    if (!LITE && !(chunk == 3 && iters > 2)) free_sweeps(iters);
    bool changed = false;
    uint32_t up[RX_P], dn[RX_P];
    {
      const u32x4_t up4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band][xl * RX_P]);
      const u32x4_t dn4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band + 3][xl * RX_P]);
      up[0] = up4.x; up[1] = up4.y; up[2] = up4.z; up[3] = up4.w;
      dn[0] = dn4.x; dn[1] = dn4.y; dn[2] = dn4.z; dn[3] = dn4.w;
    }
    WS_ACC_T0;
    refresh_columns();
    sweep_cols<true, false>(T, B, up, dn, Lh, Rh, changed);         // left, checked
    WS_ACC(2);
    const uint32_t slot = (iters - 1) % 3;
    if (__builtin_amdgcn_ballot_w64(changed) != 0) {
      // a neighbour band reads these rows only if another round follows, i.e. only if someone changed
      *reinterpret_cast<u32x4_t *>(&sRow[1 + 2 * band][xl * RX_P]) = u32x4_t{T[0][0], T[0][1], T[0][2], T[0][3]};
      *reinterpret_cast<u32x4_t *>(&sRow[2 + 2 * band][xl * RX_P]) = u32x4_t{T[3][0], T[3][1], T[3][2], T[3][3]};
      if (lane == 0) s_flag[slot] = 1;
    }
    __syncthreads();
    const bool again = s_flag[slot] != 0;
    if (tid == 0) s_flag[(slot + 2) % 3] = 0;
    if (!again) break;
    if (iters >= max_iters) { unfinished = true; break; }
    if (LITE) free_sweeps(iters);
  }
  bool any_lower = true;             // a pass that creates the stamp plane writes every patch
  if (!from_labels) {
    uint64_t sum_after = 0;
#pragma unroll
    for (int r = 0; r < RX_P; ++r)
#pragma unroll
      for (int c = 0; c < RX_P; ++c) sum_after += T[r][c];
    any_lower = sum_after != s_sum[tid];
  }
  WS_STAMP(2);
  WS_QPHASE(1);
  WS_ACC_STORE;
#ifdef WS_DIAG_STAMPS
  if (threadIdx.x == 0 && g_diag) g_diag[(size_t)blockIdx.x * 8 + 4] = iters;
#endif

  // ---- write back the patches that changed (16 B per lane and row), ring-carry check, edge flags
  uint32_t e = 0, ovf = 0;
  if (any_lower) {
    const bool full_x = gx0 >= 0 && gx0 + RX_P <= W;
#pragma unroll
    for (int r = 0; r < RX_P; ++r) {
      const int gy = gyb + r;
      if (gy >= 0 && gy < H) {
        if (full_x) {
          if (PERSIST && !(use_list & 1)) coh_store4(keys + (size_t)gy * W + gx0, u32x4_t{T[r][0], T[r][1], T[r][2], T[r][3]});
          else *reinterpret_cast<u32x4_t *>(keys + (size_t)gy * W + gx0) = u32x4_t{T[r][0], T[r][1], T[r][2], T[r][3]};
        } else {
#pragma unroll
          for (int c = 0; c < RX_P; ++c) if (gx0 + c >= 0 && gx0 + c < W) keys[(size_t)gy * W + gx0 + c] = T[r][c];
        }
      }
      if (check_carry) {               // kernel uniform
#pragma unroll
        for (int c = 0; c < RX_P; ++c)   // a finite non-seed stamp with ring 0 (a carry) or 2^24 - 1 (the last before one: out of level 254 the carry is KEY_INF)
          ovf |= (T[r][c] != 0u && T[r][c] < KEY_INF && ((T[r][c] + 1u) & RING_MASK) <= 1u);
      }
    }
    e |= 16u;
    // A tile that stopped at the round cap is not a fixpoint of its own pixels: the four tiles of the
    // other grid that cover it re-examine all of it in the next pass.
    // (before a same-grid pass the tile marks ITSELF instead: word 0 of its stamps, below)
    if (unfinished && !write_same) e |= 15u;
    // bit q: a BORDER pixel of the tile inside quadrant q = 2*(lower half) + (right half) changed
    const uint32_t qbit = 1u << ((band >= NB / 2 ? 2 : 0) + (xl >= LX / 2 ? 1 : 0));
    // (bits 6 .. 9: the same changes by SIDE -- top row, bottom row, left column, right column -- for the passes that
    // stay on one grid, where a side matters to exactly one neighbour)
    // (SEAM 1: what a band changes in its first and last four columns, where a vertical seam runs, is the business of the
    // strip that follows -- it looks at those columns again, in every row -- and raises no flag here: with them a band's
    // first / last row "changed" in a quarter of the bands, whatever their height, for the two seam pixels at its corners;
    // tools/sim_tile_schedule.c, SIM_REPAIR: 55 % of the tiles flagged with them, 41 % without, 9 % with bands of 16 rows)
    const bool row_counts = SEAM != 1 || !((lane == 0 && x0 > 0) || (lane == 63 && x0 + TW < W));
    // A changed border pixel only MATTERS to the tile across the border when it can lower the pixel it touches there:
    // new stamp + 1 < that pixel's stamp -- which this tile holds, as its halo.  (The halo is as old as the tile's load: the
    // pixel can only have fallen since, so the test errs on the side of flagging.)  On smooth maps a third to a half of the
    // late tile runs changed nothing at all (tools/sim_tile_schedule.c, SIM_CHANGED): flagged by a neighbour whose front
    // had not caught up with theirs.
    auto least = [](uint32_t before, uint32_t now, uint32_t across) { return matters(before, now, across) ? now : 0xFFFFFFFFu; };      // (PERSIST == 2: the queue's order)
    if (band == 0) {
      const u32x4_t o = *reinterpret_cast<const u32x4_t *>(&sInitRow[0][xl * RX_P]);
      const u32x4_t a = *reinterpret_cast<const u32x4_t *>(&sRow[0][xl * RX_P]);      // the halo row above, as loaded
      if (matters(o.x, T[0][0], a.x) || matters(o.y, T[0][1], a.y) || matters(o.z, T[0][2], a.z) || matters(o.w, T[0][3], a.w)) e |= qbit | (row_counts ? 64u : 0u);
      if (PERSIST == 2 && (e & 64u)) atomicMin(&s_sidemin[0], min(min(least(o.x, T[0][0], a.x), least(o.y, T[0][1], a.y)), min(least(o.z, T[0][2], a.z), least(o.w, T[0][3], a.w))));
    }
    if (band == NB - 1) {
      const u32x4_t o = *reinterpret_cast<const u32x4_t *>(&sInitRow[1][xl * RX_P]);
      const u32x4_t a = *reinterpret_cast<const u32x4_t *>(&sRow[2 * NB + 1][xl * RX_P]);      // the halo row below
      if (matters(o.x, T[3][0], a.x) || matters(o.y, T[3][1], a.y) || matters(o.z, T[3][2], a.z) || matters(o.w, T[3][3], a.w)) e |= qbit | (row_counts ? 128u : 0u);
      if (PERSIST == 2 && (e & 128u)) atomicMin(&s_sidemin[1], min(min(least(o.x, T[3][0], a.x), least(o.y, T[3][1], a.y)), min(least(o.z, T[3][2], a.z), least(o.w, T[3][3], a.w))));
    }
    if (SEAM == 2) {
      // a lane pair raises its own flags: the anchored tile that holds this lane's columns (left of the seam for the even
      // lane, right of it for the odd one), and that tile's neighbour above / below when the slice's first / last row changed
      bool col = false;
#pragma unroll
      for (int r = 0; r < RX_P; ++r) col |= matters(init_col[r], T[r][(lane & 1) ? 3 : 0], (lane & 1) ? Rh[r] : Lh[r]);      // (Lh / Rh of these lanes: the halo column)
      col |= unfinished;      // stopped at the round cap: the tiles on both sides of every seam of this slice look again
      const int fx = seam_x / SEAM_PX - 1 + (lane & 1);
      const uint32_t mark = pass + 1;
      if (seam_x < W) {      // (anchored tile rows are SEAM_PY pixel rows; a slice lies in one of them)
        if (col && gyb >= 0 && gyb < H) { stamps_cur[((size_t)(gyb / SEAM_PY) * otherX + fx) * 4 + 3] = mark; e |= 1u; }
        if ((e & 64u) && y0 > 0) { stamps_cur[((size_t)((y0 - 1) / SEAM_PY) * otherX + fx) * 4 + 3] = mark; e |= 1u; }
        if ((e & 128u) && y0 + TH < H) { stamps_cur[((size_t)((y0 + TH) / SEAM_PY) * otherX + fx) * 4 + 3] = mark; e |= 1u; }
      }
      e &= 1u | 16u;
    } else if (xl == 0 || xl == LX - 1) {
#pragma unroll
      for (int r = 0; r < RX_P; ++r)
        if (matters(sInitCol[xl == 0 ? 0 : 1][band * RX_P + r], T[r][xl == 0 ? 0 : 3], xl == 0 ? Lh[r] : Rh[r])) e |= qbit | (xl == 0 ? 256u : 512u);      // (Lh of a row's first lane, Rh of its last: the halo column)
      if (PERSIST == 2 && (e & (256u | 512u))) {
        uint32_t m = 0xFFFFFFFFu;
#pragma unroll
        for (int r = 0; r < RX_P; ++r) m = min(m, least(sInitCol[xl == 0 ? 0 : 1][band * RX_P + r], T[r][xl == 0 ? 0 : 3], xl == 0 ? Lh[r] : Rh[r]));
        atomicMin(&s_sidemin[xl == 0 ? 2 : 3], m);
      }
    }
  }
  // (SEAM 2, a slice that stopped at its round cap: also the lanes that changed nothing ask for their tile's re-run)
  if (SEAM == 2 && unfinished && !any_lower && seam_x < W && gyb >= 0 && gyb < H) {
    stamps_cur[((size_t)(gyb / SEAM_PY) * otherX + (seam_x / SEAM_PX - 1 + (lane & 1))) * 4 + 3] = pass + 1;
    e |= 1u;
  }
  // PERSIST: every wave's stamps have left for memory before the workgroup's barrier, and so before wave 0 flags a neighbour
  if (PERSIST) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (ovf) atomicExch(pf.overflow, 1u);      // never taken on sane inputs (tests/test_gpu_planted_stamps.py plants the others)
  if (unfinished && (write_same || SEAM == 1 || chunk == 3)) e |= 32u;      // (chunk == 3: pass 0 of a seam-repair transform)
  if (e) atomicOr(&s_edges, e);
  __syncthreads();
  if (tid == 0) {
    const uint32_t ed = s_edges;
    const uint32_t stripe = (blockIdx.x % NSTRIPE) * STRIPE_STRIDE;
    if (SEAM) {
      // SEAM 1: the tile above the seam holds the pixels over this tile's first row, the tile below those under its last;
      // what its first / last COLUMN changed lies inside a vertical strip, which runs after the bands.  (SEAM 2: the lanes
      // have stored their flags themselves.)
      bool any = SEAM == 2 && (ed & 1u) != 0u;
      if (SEAM == 1) {      // (bit 5: the band stopped at its round cap)
        if (ed & (64u | 32u)) { stamps_cur[((size_t)seam_fy * otherX + tile_x) * 4 + 3] = pass + 1; any = true; }
        if (ed & (128u | 32u)) { stamps_cur[((size_t)(seam_fy + 1) * otherX + tile_x) * 4 + 3] = pass + 1; any = true; }
      }
      if (any) pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT + stripe] = 1u;
      if (ed) pf.any_change[stripe] = 1u;
    } else if (ed) {
      const size_t t = (size_t)tile_y * tilesX + tile_x;
      // pass 0 of a seam-repair transform (chunk == 3) that stopped at its round cap: nobody reads this pass's own stamps
      // (the bands and strips look at every seam anyway), so the tile asks for its re-run where pass 2 will look -- the
      // word of the OTHER stamp array that the bands and strips use for the same purpose
      // (pass 2 runs anchored tile (x, y) for word 3 of entry (x, y) or word 2 of entry (x + 1, y): the first is the bands'
      // and strips', the second this one's, so that they can tell a tile pass 0 gave up on from one a band has flagged)
      if (!CHUNKED && chunk == 3 && (ed & 32u)) const_cast<uint32_t *>(stamps_prev)[((size_t)tile_y * otherX + tile_x + 1) * 4 + 2] = pass + 2;
      if (write_same) {      // the next pass runs on this grid (relax_todo, read_same)
        if (ed & 33u) stamps_cur[t * 4 + 0] = (pass + 1) | (ed & 1u ? ST_BORDER : 0u) | (ed & 32u ? ST_SELF : 0u);
        if (ed & 2u) stamps_cur[t * 4 + 1] = (pass + 1) | ST_BORDER;
        if (ed & 4u) stamps_cur[t * 4 + 2] = (pass + 1) | ST_BORDER;
        if (ed & 8u) stamps_cur[t * 4 + 3] = (pass + 1) | ST_BORDER;
      } else {
        if (ed & 1u) stamps_cur[t * 4 + 0] = pass + 1;
        if (ed & 2u) stamps_cur[t * 4 + 1] = pass + 1;
        if (ed & 4u) stamps_cur[t * 4 + 2] = pass + 1;
        if (ed & 8u) stamps_cur[t * 4 + 3] = pass + 1;
      }
      // plain, idempotent stores into striped words: no same-address atomics on the tile path
      if (ed & 47u) pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT + stripe] = 1u;
      if (append_next) {
        // The next pass's tile list is written by the tiles that cause its entries (no k_relax_list launch between two
        // passes: 5 us of every ~45).  A tighter rule than relax_todo's same-grid test (which only has the quadrant
        // stamps): a changed top-row pixel matters to the tile above and to nobody else, and so on round the tile -- a tenth
        // fewer tile runs on smooth maps than "every neighbour that touches the quadrant"; I go on myself if I stopped at
        // the round cap.  The candidates only go to LDS here: the workgroup hands them in together (append_flush).
        const bool want[5] = {(ed & 32u) != 0u, (ed & 64u) != 0u && tile_y > 0, (ed & 128u) != 0u && tile_y + 1 < tilesY,
                              (ed & 256u) != 0u && tile_x > 0, (ed & 512u) != 0u && tile_x + 1 < tilesX};
        const uint32_t who[5] = {(uint32_t)t, (uint32_t)(t - tilesX), (uint32_t)(t + tilesX), (uint32_t)(t - 1), (uint32_t)(t + 1)};
        uint32_t n = s_ncand;
        if (PERSIST == 2) {
          // the bucket of what I announce: the level of the smallest stamp that matters across that side; for myself (I
          // stopped at the round cap) the lowest of them and of the bucket I ran from
          uint32_t bk[5];
          bk[0] = s_qbucket;
#pragma unroll
          for (int k = 1; k < 5; ++k) {
            bk[k] = min(s_sidemin[k - 1] >> q.pq_shift, (uint32_t)(PQ_B - 1));
            if (want[k]) bk[0] = min(bk[0], bk[k]);
          }
#pragma unroll
          for (int k = 0; k < 5; ++k)
            if (want[k]) s_cand[n++] = who[k] | (bk[k] << 24);
        } else {
#pragma unroll
          for (int k = 0; k < 5; ++k)
            if (want[k]) s_cand[n++] = who[k];
        }
        s_ncand = n;
      }
      pf.any_change[stripe] = 1u;
    }
    count_tile_run(pf, stripe, (uint32_t)(TW * TH / 2048), iters);
  }
  WS_STAMP(3);
  WS_QPHASE(2);
  // hand in (the queue), or the next tile
  if (PERSIST == 2) {
    queue_hand_in_flood_order(q, (uint32_t)tile, tid, lane, use_list, s_cand, s_ncand, s_qtile, s_qbucket, s_handoff);
    WS_QPHASE(3);
    continue;
  }
  if (PERSIST) {
    queue_hand_in_first_come(q, (uint32_t)tile, tid, lane, s_cand, s_ncand);
    WS_QPHASE(3);
    continue;
  }
  // next tile of the chunk: every wave is past its last read of the shared arrays (barrier above)
  if (!CHUNKED) break;
  if (use_list) {
    entry = s_next[runs_done & 1u];      // (written before this run's first barrier)
    ++runs_done;
    const bool last = entry >= n_entries;
    // wave 0 hands the candidates in: when this was the workgroup's last tile, or when another tile's five might not fit
    if (append_next && tid < 64 && (last || s_ncand > RX_CAND - 5u)) append_flush(tile_list, list_cap, pass, s_cand, s_ncand);
    if (last) break;
  } else {
    todo &= todo - 1;
    if (todo == 0) break;
  }
  }
}

// The tiles that have to run in `pass`, compacted: tile_list[pass & 3] = how many, entries from tile_list[RL_HDR + (pass & 1) *
// list_cap] on (any order).  It also clears the tiles' "queued for pass" words, which the passes that append their
// successors' lists themselves (k_relax, append_next) exchange: every transform that reaches those passes comes through here.
// Same test as relax_todo; one atomicAdd per wave that found any.  Worth its own launch only when few tiles run: on a
// smooth map a pass moves the flood fronts by one tile, a few hundred tiles out of thousands, and the chunked launch
// (a workgroup per four tiles, most of them idle, some with two busy ones to run back to back) took twice as long as
// the tiles themselves.
template <int TW, int TH>
__global__ __launch_bounds__(256) void k_relax_list(int H, int W, int tilesX, int tilesY, int otherX, int otherY, int shifted,
                                                    uint32_t pass, const uint32_t *__restrict__ stamps_prev, uint32_t *tile_list,
                                                    int read_same, uint32_t list_cap) {
  const int lane = threadIdx.x & 63;
  const int first = (int)((blockIdx.x * blockDim.x + threadIdx.x) & ~63u);      // this wave's 64 consecutive tiles
  if ((uint32_t)(first + lane) <= list_cap) tile_list[RL_HDR + 2 * (size_t)list_cap + first + lane] = 0u;      // queued marks (and the dummy slot)
  const unsigned long long todo = relax_todo<TW, TH>(first, 1, 64, H, W, tilesX, tilesY, otherX, otherY, shifted, pass, stamps_prev, read_same);
  if (todo == 0) return;
  uint32_t base = 0;
  if (lane == 0) base = atomicAdd(&tile_list[pass & 3u], (uint32_t)__popcll(todo));
  base = __shfl(base, 0, 64);
  if ((todo >> lane) & 1ull)
    tile_list[RL_HDR + (pass & 1u) * (size_t)list_cap + base + __popcll(todo & ((1ull << lane) - 1ull))] = (uint32_t)(first + lane);
}

// The first pass on the 128 x 64 grid (RX_SAME_GRID_FROM): its tile list from the edge stamps that the pass before it left
// on the 256 x 32 grid.  An equation can only be left violated inside a tile that stopped at its round cap, or next to a
// border pixel that a tile changed: every new tile that touches an old tile with ANY stamp word of that pass (the old
// tile's rectangle grown by one pixel) runs -- a superset of the tiles relax_todo would pick, and running a tile that has
// nothing to do changes nothing.
template <int TW, int TH, int OTW, int OTH>
__global__ __launch_bounds__(256) void k_relax_list_regrid(int H, int W, int tilesX, int tilesY, int oldX, int oldY, uint32_t pass,
                                                           const uint32_t *__restrict__ stamps_prev, uint32_t *tile_list, uint32_t list_cap,
                                                           int persist) {
  // persist: the list is the first filling of the persistent pass's queue (k_relax, PERSIST) -- (sequence number, tile) pairs
  // in the ring, the tiles' state words "queued", the tiles counted in [RLQ_PENDING]; the host has zeroed ring and counters
  const int lane = threadIdx.x & 63;
  const int first = (int)((blockIdx.x * blockDim.x + threadIdx.x) & ~63u);
  const int t = first + lane;
  bool run = false;
  if (t < tilesX * tilesY) {
    const int tx = t % tilesX, ty = t / tilesX;
    const int x_lo = max(tx * TW - 1, 0) / OTW, x_hi = min((tx * TW + TW) / OTW, oldX - 1);
    const int y_lo = max(ty * TH - 1, 0) / OTH, y_hi = min((ty * TH + TH) / OTH, oldY - 1);
    for (int oy = y_lo; oy <= y_hi; ++oy)
      for (int ox = x_lo; ox <= x_hi; ++ox) {
        const uint4 st = *reinterpret_cast<const uint4 *>(stamps_prev + ((size_t)oy * oldX + ox) * 4);
        run |= (st.x & ST_PASS) == pass || (st.y & ST_PASS) == pass || (st.z & ST_PASS) == pass || (st.w & ST_PASS) == pass;
      }
    run = run && tx * TW < W && ty * TH < H;
  }
  if ((uint32_t)t <= list_cap) tile_list[RL_HDR + 2 * (size_t)list_cap + t] = persist && run ? 1u : 0u;      // queued marks (and the dummy slot)
  const unsigned long long todo = __builtin_amdgcn_ballot_w64(run);
  if (todo == 0) return;
  uint32_t base = 0;
  if (lane == 0) {
    base = atomicAdd(&tile_list[persist ? RLQ_TAIL : (pass & 3u)], (uint32_t)__popcll(todo));      // (persist == 2: a count for the diagnostics)
    if (persist) atomicAdd(&tile_list[RLQ_PENDING], (uint32_t)__popcll(todo));
  }
  base = __shfl(base, 0, 64);
  const uint32_t idx = base + (uint32_t)__popcll(todo & ((1ull << lane) - 1ull));
  if (persist == 2) {      // the queue in flood order: everything starts in bucket 0 (these 64 tiles are two words of its bitmap, this wave's alone)
    uint32_t *avail = tile_list + pq_base(list_cap);
    if (lane == 0) atomicAdd(avail, (uint32_t)__popcll(todo));
    if ((lane & 31) == 0) (avail + PQ_HDR)[(first >> 5) + (lane >> 5)] = (uint32_t)(todo >> (lane & 32));
  } else if (run && persist) reinterpret_cast<unsigned long long *>(tile_list + RL_HDR)[idx] = ((unsigned long long)(idx + 1u) << 32) | (uint32_t)t;
  else if (run) tile_list[RL_HDR + (pass & 1u) * (size_t)list_cap + idx] = (uint32_t)t;
}

// Every tile of the plane, as the list of `pass`: the pass after the persistent one looks at each of them once (a tile that
// is at its fixpoint leaves after one checked sweep), whatever the queue did.
template <int TW, int TH>
__global__ __launch_bounds__(256) void k_relax_list_all(int H, int W, int tilesX, int tilesY, uint32_t pass, uint32_t *tile_list, uint32_t list_cap) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) { tile_list[pass & 3u] = (uint32_t)(tilesX * tilesY); tile_list[4 + (pass & 3u)] = 0u; }
  if ((uint32_t)t <= list_cap) tile_list[RL_HDR + 2 * (size_t)list_cap + t] = 0u;      // queued marks: the append protocol of the later passes starts clean
  if (t < tilesX * tilesY) tile_list[RL_HDR + (pass & 1u) * (size_t)list_cap + t] = (uint32_t)t;      // (every tile of this grid starts inside the plane)
}

// words of scratch relax_pass wants for its tile lists
// header, two entry arrays, queued marks (+ dummies); the persistent pass's buckets: counts (a line each), bitmaps
size_t relax_list_words(int h, int w) {
  const uint32_t tiles = (uint32_t)relax_tiles(h, w);
  return pq_base(tiles) + PQ_HDR + (size_t)PQ_B * pq_words_per_bucket(tiles);
}

size_t relax_tiles(int h, int w) { return relax_plan_tiles(h, w); }

// Row block of a tiled field: the caller has rewritten the plane's halo rows (row 0 and / or row h - 1).  Only tiles that
// hold those rows have anything new to look at: raise, in the stamp array that the EVEN pass `pass` reads (the shifted
// grid's), every quadrant flag of its first / last tile row, so that exactly the first / last tile row of the anchored
// grid runs in that pass; what they change spreads by the usual flags.  The stamp arrays must be zeroed first.
__global__ void k_flag_tile_rows(uint32_t *prev, int sx, int bottom_row, uint32_t pass, int halo_flags) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sx * 4) return;
  if (halo_flags & 1) prev[i] = pass;
  if (halo_flags & 2) prev[(size_t)bottom_row * sx * 4 + i] = pass;
}

hipError_t block_flag_border_tiles(hipStream_t s, uint32_t *stamps, int h, int w, uint32_t pass, int halo_flags) {
  if ((pass & 1u) != 0 || h == 0 || w == 0) return hipErrorInvalidValue;
  const int th = RX_NW * RX_P;
  const int sx = (w + RX_TW - 1) / RX_TW + 1;
  const size_t cap = relax_tiles(h, w) * 4;
  // An anchored tile row t runs when row t or t + 1 of the shifted grid is flagged.  What has to run is every tile that
  // holds a pixel NEXT to a halo row, i.e. plane rows 1 (tile row 0: shifted row 0) and h - 2 -- which need not share a
  // tile with the halo row h - 1 itself (a block of 32 k + 1 rows: the halo row has a tile row of its own, and running
  // only that one, whose pixels are all pinned, repairs nothing).  Shifted row (h - 2) / th + 1 starts tile row
  // (h - 2) / th and, when it exists, the one below.
  const int bottom_row = (h - 2) / th + 1;
  k_flag_tile_rows<<<(sx * 4 + 255) / 256, 256, 0, s>>>(stamps + cap, sx, bottom_row, pass, halo_flags);      // array 1: written by odd passes
  return hipGetLastError();
}

// ---- pass 0 of the seam-repair flow on 256 x 64 tiles --------------------------------------------------------------------
//
// Pass 0 of a transform that starts from its seeds and repairs its seams with bands and strips (relax_pass, seam_flow) has
// its own kernel: the same sweeps and the same pieces as k_relax, but a lane owns 4 columns x 8 rows -- two stacked 4 x 4 patches -- so the
// tile is 256 x 64 with the same eight waves.  What a tile run pays outside its sweeps (image bytes to bases, seed bits to
// stamps, addresses, the band rows' way through LDS) is paid once per 32 pixels of a lane instead of once per 16, rows 3
// and 4 of a patch are neighbours in registers, and the plane has half as many horizontal seams for the bands to repair.
// None of this fits k_relax's 80 registers, and none of that template's other nine variants needs it.
//   * only the fast path: W % 4 == 0, image rows readable as aligned dwords, seeds as a bit plane (relax_pass asks);
//   * the stamp plane is created here (every patch is written), so there is no "did my patch change" sum;
//   * nobody reads pass 0's quadrant flags in this flow -- bands and strips look at every seam whatever they say -- so the
//     tile border as loaded is not kept.  "A border pixel changed and matters across the border" (the pass's convergence
//     word) needs no copy either: a border pixel starts as a seed (0, for ever) or at KEY_INF, so it changed iff it is
//     neither now, and what lies across the border is still in the halo row of LDS / the halo column registers;
//   * a tile that stops at its round cap marks BOTH 256 x 32 tiles it covers, in the words the bands, the strips and pass 2
//     read, and all their quadrant flags, as k_relax does for its one.

// (flagAX / flagSX: tile columns of the anchored / shifted 256 x 32 grid, the pitches of stamps_own / stamps_rerun)
__global__ __launch_bounds__(64 * RX_NW, 4) void k_relax0_tall(const uint8_t *__restrict__ img, uint32_t stride32, uint32_t *keys, int H, int W,
                                                               int tilesX, int flagAX, int flagSX, uint32_t max_level, uint32_t *stamps_own,
                                                               uint32_t *stamps_rerun, PassFlags pf, uint32_t max_iters,
                                                               const uint32_t *__restrict__ seed_mask, int SH, int check_carry, uint32_t *tile_list) {
  constexpr int NB = RX_NW, TW = RX_TW, TH = RX0_TH;
  constexpr uint32_t pass = 0;
  // row 0: halo above the tile; rows 1+2w / 2+2w: top / bottom row of band w; last row: halo below
  __shared__ __attribute__((aligned(16))) uint32_t sRow[2 * NB + 2][TW];
  __shared__ uint32_t s_flag[3];      // "some lane changed in round k" in slot k % 3 (k_relax)

  launch_prologue(pf, tile_list, pass);
  const int tile = (int)xcd_span_index(blockIdx.x, gridDim.x);      // (XCD-aware: consecutive workgroups go to different XCDs)
  const int tile_x = tile % tilesX, tile_y = tile / tilesX;
  const int x0 = tile_x * TW, y0 = tile_y * TH;
  if (x0 >= W || y0 >= H) return;
  const int tid = threadIdx.x, lane = tid & 63, band = tid >> 6;
  const int gx0 = x0 + lane * RX_P, gyb = y0 + band * RX0_PH;
  if (tid == 0) { s_flag[0] = 0; s_flag[1] = 0; s_flag[2] = 0; }

  // ---- load phase: unconditional loads on clamped addresses; a patch (W % 4 == 0) is wholly inside the plane or wholly outside
  uint32_t T[RX0_PH][RX_P], B[RX0_PH][RX_P];
  uint32_t Lh[RX0_PH], Rh[RX0_PH];
  const bool dims24 = (uint32_t)W < (1u << 24) && (uint32_t)H < (1u << 24);      // kernel uniform: row * W as v_mul_u32_u24
  const uint32_t gxc0 = (uint32_t)min(gx0, W - RX_P);
  // tile halo columns: the left half of the lanes fetch the column left of the tile, the right half the one right of it;
  // only lane 0 / lane 63 ever use the value (as the DPP `old` operand)
  const int xh_raw = lane < 32 ? x0 - 1 : x0 + TW;
  const uint32_t xh = (uint32_t)min(max(xh_raw, 0), W - 1);
  const bool xh_ok = lane < 32 ? x0 > 0 : x0 + TW < W;
  const int gy_halo_raw = band == 0 ? y0 - 1 : y0 + TH;
  const uint32_t gy_halo = (uint32_t)min(max(gy_halo_raw, 0), H - 1);
  u32x4_t halo_row;
  {
    uint32_t iv[RX0_PH];
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      const uint32_t gyc = (uint32_t)min(gyb + r, H - 1);
      // (a bit plane exists only for planes of fewer than 2^31 pixels: pixel indices fit 32 bits)
      const uint32_t ro = dims24 ? __umul24(gyc, (uint32_t)W) : gyc * (uint32_t)W;
      const uint32_t p = ro + gxc0, ph_ = ro + xh;
      const uint32_t nib = seed_mask[p >> 5] >> (p & 31u);
      iv[r] = *reinterpret_cast<const uint32_t *>(img + ((unsigned long long)gyc * stride32 + gxc0));
      Lh[r] = (seed_mask[ph_ >> 5] >> (ph_ & 31u)) & 1u;
      T[r][0] = nib & 1u; T[r][1] = nib & 2u; T[r][2] = nib & 4u; T[r][3] = nib & 8u;
    }
    const uint32_t p = (dims24 ? __umul24(gy_halo, (uint32_t)W) : gy_halo * (uint32_t)W) + gxc0;
    const uint32_t nib = seed_mask[p >> 5] >> (p & 31u);
    halo_row = u32x4_t{nib & 1u, nib & 2u, nib & 4u, nib & 8u};
    patch_bases(iv, B, max_level);
  }
  halo_row = seed_stamps(T, Lh, halo_row);
  // Workgroup uniform: the tile and its halo ring lie strictly inside the image (and the image is not a stack of slices) --
  // none of the masks below can bite (k_relax)
  const bool inner = SH == H && x0 >= 1 && x0 + TW <= W - 1 && y0 >= 1 && y0 + TH <= H - 1;
  if (!inner) {
    int ry = SH == H ? gyb : gyb % SH;      // row inside its slice (a patch of eight rows may hold the walls of several slices)
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      const int gy = gyb + r;
      const bool row_ok = gy < H, row_int = ry >= 1 && ry < SH - 1 && gy < H;
#pragma unroll
      for (int c = 0; c < RX_P; ++c) {
        const int gx = gx0 + c;
        if (!(row_ok && gx < W)) T[r][c] = KEY_INF;
        if (!(row_int && gx >= 1 && gx < W - 1)) B[r][c] = KEY_INF;
      }
      if (!(row_ok && xh_ok)) Lh[r] = KEY_INF;
      if (++ry == SH) ry = 0;
    }
    const bool ok = gy_halo_raw >= 0 && gy_halo_raw < H;
    if (!(ok && gx0 + 0 < W)) halo_row.x = KEY_INF;
    if (!(ok && gx0 + 1 < W)) halo_row.y = KEY_INF;
    if (!(ok && gx0 + 2 < W)) halo_row.z = KEY_INF;
    if (!(ok && gx0 + 3 < W)) halo_row.w = KEY_INF;
  }
#pragma unroll
  for (int r = 0; r < RX0_PH; ++r) {
#pragma unroll
    for (int c = 0; c < RX_P; ++c) B[r][c] = min(B[r][c], T[r][c]);      // b <= t: seeds and everything that can never change are pinned
    Rh[r] = Lh[r];
  }
  // the columns left / right of the patch, persistent: lane 0 / lane 63 keep the tile's halo column (k_relax, refresh_columns)
  auto refresh_columns = [&]() {
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      Lh[r] = lane_left(Lh[r], T[r][3]);
      Rh[r] = lane_right(Rh[r], T[r][0]);
    }
  };
  auto publish_rows = [&]() {
    *reinterpret_cast<u32x4_t *>(&sRow[1 + 2 * band][lane * RX_P]) = u32x4_t{T[0][0], T[0][1], T[0][2], T[0][3]};
    *reinterpret_cast<u32x4_t *>(&sRow[2 + 2 * band][lane * RX_P]) = u32x4_t{T[RX0_PH - 1][0], T[RX0_PH - 1][1], T[RX0_PH - 1][2], T[RX0_PH - 1][3]};
  };
  if (band == 0) *reinterpret_cast<u32x4_t *>(&sRow[0][lane * RX_P]) = halo_row;
  if (band == NB - 1) *reinterpret_cast<u32x4_t *>(&sRow[2 * NB + 1][lane * RX_P]) = halo_row;
  publish_rows();
  __syncthreads();

  // ---- relaxation: round 1 is k_relax's round (three free sweeps down, right, up; the band rows published; one checked sweep
  // left); every later round is ONE free sweep, up, the band rows published, and the checked sweep left -- "DRU|L, then U|L".
  // What a tile has left to settle after its first round has to travel in every direction, and a checked left sweep alone
  // as a later round (the rule tuned on 256 x 32 tiles) left tiles moving at the round cap; a free sweep in another direction
  // in front of the checked one lets them end.  The replay (tools/sim_tile_schedule.c, SIM_P0_RECIPE2 / SIM_P0_RECIPE_LATER)
  // and the counts and times measured on the GPU: DESIGN section 10.
  // Exactness needs no new argument: every sweep is a sequence of relaxation steps on stamps that start from an upper bound,
  // any order of such steps reaches the same fixpoint, and a run still ends only when a CHECKED sweep over all its pixels, on
  // published rows, has changed nothing -- or at the round cap, where it marks its tiles as before.
  uint32_t iters = 0;
  bool unfinished = max_iters == 0;
  uint32_t up[RX_P], dn[RX_P];
  auto fetch_rows = [&]() {
    const u32x4_t up4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band][lane * RX_P]);
    const u32x4_t dn4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band + 3][lane * RX_P]);
    up[0] = up4.x; up[1] = up4.y; up[2] = up4.z; up[3] = up4.w;
    dn[0] = dn4.x; dn[1] = dn4.y; dn[2] = dn4.z; dn[3] = dn4.w;
  };
  for (; max_iters != 0;) {
    ++iters;
    {
      bool untracked = false;
      fetch_rows();
      if (iters == 1) {
        refresh_columns();
        sweep_rows<false, true>(T, B, up, dn, Lh, Rh, untracked);       // down
        refresh_columns();
        sweep_cols<false, true>(T, B, up, dn, Lh, Rh, untracked);       // right
      }
      refresh_columns();
      sweep_rows<false, false>(T, B, up, dn, Lh, Rh, untracked);      // up
      publish_rows();
      __syncthreads();
    }
    bool changed = false;
    fetch_rows();
    refresh_columns();
    sweep_cols<true, false>(T, B, up, dn, Lh, Rh, changed);           // left, checked
    const uint32_t slot = (iters - 1) % 3;
    if (__builtin_amdgcn_ballot_w64(changed) != 0) {
      publish_rows();      // a neighbour band reads these rows only if another round follows, i.e. only if someone changed
      if (lane == 0) s_flag[slot] = 1;
    }
    __syncthreads();
    const bool again = s_flag[slot] != 0;
    if (tid == 0) s_flag[(slot + 2) % 3] = 0;
    if (!again) break;
    if (iters >= max_iters) { unfinished = true; break; }
  }
  WS_STAMP(0);
  WS_STAMP_VALUE(4, iters);      // (tools/diag_seam_rounds.hip: the rounds of this tile run)

  // ---- write every patch back (16 B per lane and row), ring-carry check, flags
  uint32_t ovf = 0;
  if (gx0 < W) {
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      const int gy = gyb + r;
      if (gy < H) *reinterpret_cast<u32x4_t *>(keys + (size_t)gy * W + gx0) = u32x4_t{T[r][0], T[r][1], T[r][2], T[r][3]};
      if (check_carry) {               // kernel uniform
#pragma unroll
        for (int c = 0; c < RX_P; ++c)   // a finite non-seed stamp with ring 0 (a carry) or 2^24 - 1 (the last before one: out of level 254 the carry is KEY_INF)
          ovf |= (T[r][c] != 0u && T[r][c] < KEY_INF && ((T[r][c] + 1u) & RING_MASK) <= 1u);
      }
    }
  }
  if (ovf) atomicExch(pf.overflow, 1u);      // never taken on sane inputs (and by no test: this kernel starts from seeds only)
  const uint32_t stripe = (blockIdx.x % NSTRIPE) * STRIPE_STRIDE;
  // A changed border pixel matters to the tile across the border when it can lower the pixel it touches there, which this
  // tile holds as its halo (`matters`).  No copy of the border as loaded is kept: a border pixel starts as a seed (0, for ever) or at
  // KEY_INF, so "before" is 0 -- changed: neither a seed nor still KEY_INF, which `now + 1 < across` implies.
  bool edge = false;
  if (band == 0) {
    const u32x4_t a = *reinterpret_cast<const u32x4_t *>(&sRow[0][lane * RX_P]);      // the halo row above, as loaded
    edge |= matters(0u, T[0][0], a.x) || matters(0u, T[0][1], a.y) || matters(0u, T[0][2], a.z) || matters(0u, T[0][3], a.w);
  }
  if (band == NB - 1) {
    const u32x4_t a = *reinterpret_cast<const u32x4_t *>(&sRow[2 * NB + 1][lane * RX_P]);      // the halo row below
    constexpr int l = RX0_PH - 1;
    edge |= matters(0u, T[l][0], a.x) || matters(0u, T[l][1], a.y) || matters(0u, T[l][2], a.z) || matters(0u, T[l][3], a.w);
  }
  if (lane == 0 || lane == 63) {
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) edge |= matters(0u, T[r][lane == 0 ? 0 : 3], lane == 0 ? Lh[r] : Rh[r]);      // (Lh of lane 0, Rh of lane 63: the halo column)
  }
  // plain, idempotent stores into striped words: no same-address atomics on the tile path
  if (edge) pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT + stripe] = 1u;
  if (tid == 0) {
    if (unfinished) {
      // Stopped at the round cap: not a fixpoint of its own pixels.  Both 256 x 32 tiles ask for their re-run where pass 2
      // will look -- word 2 of entry (x + 1, y) of the stamp array the bands and strips write (k_relax, chunk == 3) -- and
      // raise all their quadrant flags.
#pragma unroll
      for (int k = 0; k < RX0_TH / (RX_NW * RX_P); ++k) {
        const int fy = tile_y * (RX0_TH / (RX_NW * RX_P)) + k;
        if (fy * (RX_NW * RX_P) >= H) break;
        stamps_rerun[((size_t)fy * flagSX + tile_x + 1) * 4 + 2] = pass + 2;
        uint32_t *own = stamps_own + ((size_t)fy * flagAX + tile_x) * 4;
        own[0] = pass + 1; own[1] = pass + 1; own[2] = pass + 1; own[3] = pass + 1;
      }
      pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT + stripe] = 1u;
    }
    pf.any_change[stripe] = 1u;
    count_tile_run(pf, stripe, (uint32_t)(TW * TH / 2048), 2u * iters);      // a 256 x 64 run counts as two tile runs of `iters` rounds each
  }
}

// ---- the strips of that flow on 64-row slices ----------------------------------------------------------------------------
//
// After pass 0 on 256 x 64 tiles the horizontal seams, and the bands that repair them, lie at rows 64 k.  A strip slice of 32
// rows (k_relax, SEAM 2) then has every other end on a row 64 k + 32 that no band has touched: the vertical seam is as wrong
// there as anywhere, the two slices that meet run side by side on each other's stale rows, both change their outer rows and
// both flag -- tools/sim_tile_schedule.c (SIM_REPAIR_GEOM): 31 % of the 256 x 32 tiles flagged for pass 2, 26 % of them by a
// slice's first / last row, against 9 % / 4 % when pass 0 ran on 256 x 32 tiles.  Slices of 64 rows end on rows 64 k only,
// where the bands have run: 7 % / 2 %.
// The layout is k_relax0_tall's: eight waves, a lane holds 4 columns x 8 rows; and SEAM 2's across: lanes 2 j and 2 j + 1 hold
// the 8 columns astride seam 32 tile_x + j + 1 (x = 256 times that), and a select after each DPP shift keeps stamps from
// crossing from one lane PAIR to the next.  Sweep order and round cap are those of the 32-row strips.
//   * only the fast path (W % 4 == 0, image rows readable as aligned dwords: k_relax0_tall's conditions, relax_pass asks);
//   * of the slice as loaded only what the flag rule reads is kept: every lane's outer column, the first and the last row;
//   * the flags are those of SEAM 2, in the same words, by the same "changed and matters" rule: a lane flags the 256 x 32 tile
//     that holds its eight rows (a slice spans two tile rows), on its own side of the seam, when its outer column changed;
//     the tile above / below the slice when the slice's first / last row (rows 64 k and 64 k + 63) changed; a slice that stops
//     at its round cap marks both tile rows on both sides of each of its seams.
__global__ __launch_bounds__(64 * RX_NW, 4) void k_relax_strips_tall(const uint8_t *__restrict__ img, uint32_t stride32, uint32_t *keys, int H, int W,
                                                                     int stripsX, int flagSX, uint32_t max_level, uint32_t pass, uint32_t *stamps_cur,
                                                                     PassFlags pf, uint32_t max_iters, int SH, int check_carry, uint32_t *tile_list) {
  constexpr int NB = RX_NW, TW = RX_TW, TH = RX0_TH;
  // row 0: halo above the slice; rows 1+2w / 2+2w: top / bottom row of band w; last row: halo below
  __shared__ __attribute__((aligned(16))) uint32_t sRow[2 * NB + 2][TW];
  __shared__ __attribute__((aligned(16))) uint32_t sInitRow[2][TW];      // the slice's first and last row as loaded
  __shared__ uint32_t s_flag[3];      // "some lane changed in round k" in slot k % 3 (k_relax)
  __shared__ uint32_t s_edges;
  __shared__ uint64_t s_sum[64 * NB];      // per-lane patch checksum taken at load time (k_relax)
  __shared__ uint32_t sInitCol[RX0_PH][64 * NB];      // every lane's outer column as loaded (parked: the sweeps need the registers)

  launch_prologue(pf, tile_list, pass);
  const int tile = (int)xcd_span_index(blockIdx.x, gridDim.x);
  const int tile_x = tile % stripsX, tile_y = tile / stripsX;
  const int y0 = tile_y * TH;
  if (y0 >= H || (tile_x * 32 + 1) * SEAM_PX >= W) return;
  const int tid = threadIdx.x, lane = tid & 63, band = tid >> 6;
  const int seam_x = (tile_x * 32 + (lane >> 1) + 1) * SEAM_PX;      // this lane pair's seam (outside the plane: no seam)
  const bool has_seam = seam_x < W;
  const int fx = seam_x / SEAM_PX - 1 + (lane & 1);      // the tile column this lane's columns lie in
  {
    // A 256 x 32 tile that pass 0 gave up on (word 2 of entry (x + 1, y): k_relax0_tall) is left to its re-run: when that is
    // every tile this slice touches -- a smooth map -- the slice does not run.  Per 32-row half, as the marks are.
    bool settled = true;
#pragma unroll
    for (int k = 0; k < TH / SEAM_PY; ++k) {
      const int fy = tile_y * (TH / SEAM_PY) + k;
      const bool there = has_seam && fy * SEAM_PY < H;
      const uint32_t word = stamps_cur[there ? ((size_t)fy * flagSX + fx + 1) * 4 + 2 : 2];
      settled &= !there || word == pass + 1;
    }
    if (__builtin_amdgcn_ballot_w64(settled) == ~0ull) return;      // (workgroup uniform: every wave asks the same 64 questions)
  }
  const int gx0 = has_seam ? seam_x - RX_P + (lane & 1) * RX_P : W, gyb = y0 + band * RX0_PH;
  if (tid == 0) { s_edges = 0; s_flag[0] = 0; s_flag[1] = 0; s_flag[2] = 0; }

  // ---- load phase: unconditional loads on clamped addresses; a patch (W % 4 == 0) is wholly inside the plane or wholly outside
  uint32_t T[RX0_PH][RX_P], B[RX0_PH][RX_P];
  uint32_t halo[RX0_PH];      // the column outside this lane's side of the strip: left of the even lane, right of the odd one
  const uint32_t gxc0 = (uint32_t)min(gx0, W - RX_P);
  const int xh_raw = (lane & 1) ? gx0 + RX_P : gx0 - 1;
  const uint32_t xh = (uint32_t)min(max(xh_raw, 0), W - 1);
  const bool xh_ok = has_seam && xh_raw < W;
  const int gy_halo_raw = band == 0 ? y0 - 1 : y0 + TH;
  const uint32_t gy_halo = (uint32_t)min(max(gy_halo_raw, 0), H - 1);
  u32x4_t halo_row;
  {
    u32x4_t kv[RX0_PH];
    uint32_t iv[RX0_PH];
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      const uint32_t gyc = (uint32_t)min(gyb + r, H - 1);
      iv[r] = *reinterpret_cast<const uint32_t *>(img + ((unsigned long long)gyc * stride32 + gxc0));
      kv[r] = *reinterpret_cast<const u32x4_t *>(keys + (size_t)gyc * W + gxc0);
      halo[r] = keys[(size_t)gyc * W + xh];
    }
    halo_row = *reinterpret_cast<const u32x4_t *>(keys + (size_t)gy_halo * W + gxc0);
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) { T[r][0] = kv[r].x; T[r][1] = kv[r].y; T[r][2] = kv[r].z; T[r][3] = kv[r].w; }
    patch_bases(iv, B, max_level);
  }
  {
    // pixels outside the plane never hold a stamp, pixels of the image border and of a slice wall never change (k_relax)
    int ry = SH == H ? gyb : gyb % SH;      // row inside its slice of a stack (a patch of eight rows may hold the walls of several)
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      const int gy = gyb + r;
      const bool row_ok = gy < H, row_int = ry >= 1 && ry < SH - 1 && gy < H;
#pragma unroll
      for (int c = 0; c < RX_P; ++c) {
        const int gx = gx0 + c;
        if (!(row_ok && gx < W)) T[r][c] = KEY_INF;
        if (!(row_int && gx >= 1 && gx < W - 1)) B[r][c] = KEY_INF;
      }
      if (!(row_ok && xh_ok)) halo[r] = KEY_INF;
      if (++ry == SH) ry = 0;
    }
    const bool ok = gy_halo_raw >= 0 && gy_halo_raw < H;
    if (!(ok && gx0 + 0 < W)) halo_row.x = KEY_INF;
    if (!(ok && gx0 + 1 < W)) halo_row.y = KEY_INF;
    if (!(ok && gx0 + 2 < W)) halo_row.z = KEY_INF;
    if (!(ok && gx0 + 3 < W)) halo_row.w = KEY_INF;
  }
  uint32_t Lh[RX0_PH], Rh[RX0_PH];
  {
    uint64_t sum_before = 0;      // stamps only ever decrease: a 64-bit patch sum tells "changed" exactly
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
#pragma unroll
      for (int c = 0; c < RX_P; ++c) {
        B[r][c] = min(B[r][c], T[r][c]);      // b <= t: seeds and everything that can never change are pinned
        sum_before += T[r][c];
      }
      Lh[r] = halo[r];
      Rh[r] = halo[r];
      sInitCol[r][tid] = (lane & 1) ? T[r][RX_P - 1] : T[r][0];
    }
    s_sum[tid] = sum_before;
  }
  // The columns left / right of the patch, persistent (k_relax): the even lane's right column is the odd lane's first, the
  // odd lane's left column the even lane's last, and the select puts the strip's halo column back where the shift has
  // brought in a stamp of the next lane pair.
  auto refresh_columns = [&]() {
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      Lh[r] = lane_left(Lh[r], T[r][RX_P - 1]);
      Rh[r] = lane_right(Rh[r], T[r][0]);
      Lh[r] = (lane & 1) ? Lh[r] : halo[r];
      Rh[r] = (lane & 1) ? halo[r] : Rh[r];
    }
  };
  auto publish_rows = [&]() {
    *reinterpret_cast<u32x4_t *>(&sRow[1 + 2 * band][lane * RX_P]) = u32x4_t{T[0][0], T[0][1], T[0][2], T[0][3]};
    *reinterpret_cast<u32x4_t *>(&sRow[2 + 2 * band][lane * RX_P]) = u32x4_t{T[RX0_PH - 1][0], T[RX0_PH - 1][1], T[RX0_PH - 1][2], T[RX0_PH - 1][3]};
  };
  if (band == 0) {
    *reinterpret_cast<u32x4_t *>(&sRow[0][lane * RX_P]) = halo_row;
    *reinterpret_cast<u32x4_t *>(&sInitRow[0][lane * RX_P]) = u32x4_t{T[0][0], T[0][1], T[0][2], T[0][3]};
  }
  if (band == NB - 1) {
    *reinterpret_cast<u32x4_t *>(&sRow[2 * NB + 1][lane * RX_P]) = halo_row;
    *reinterpret_cast<u32x4_t *>(&sInitRow[1][lane * RX_P]) = u32x4_t{T[RX0_PH - 1][0], T[RX0_PH - 1][1], T[RX0_PH - 1][2], T[RX0_PH - 1][3]};
  }
  publish_rows();
  __syncthreads();

  // ---- relaxation: the strips' rounds -- three free sweeps, the band rows published, one checked sweep -- to the slice's
  // fixpoint or the round cap.  (Full rounds in EVERY round, unlike k_relax0_tall and the bands: with the sweep up alone from
  // the second round on a slice needs fewer sweeps but more rounds, and this launch is a chain of loads, barriers and stores,
  // not of sweeps: measured slower)
  uint32_t iters = 0;
  bool unfinished = max_iters == 0;
  uint32_t up[RX_P], dn[RX_P];
  auto fetch_rows = [&]() {
    const u32x4_t up4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band][lane * RX_P]);
    const u32x4_t dn4 = *reinterpret_cast<const u32x4_t *>(&sRow[2 * band + 3][lane * RX_P]);
    up[0] = up4.x; up[1] = up4.y; up[2] = up4.z; up[3] = up4.w;
    dn[0] = dn4.x; dn[1] = dn4.y; dn[2] = dn4.z; dn[3] = dn4.w;
  };
  for (; max_iters != 0;) {
    ++iters;
    {
      bool untracked = false;
      fetch_rows();
      refresh_columns();
      sweep_rows<false, true>(T, B, up, dn, Lh, Rh, untracked);       // down
      refresh_columns();
      sweep_cols<false, true>(T, B, up, dn, Lh, Rh, untracked);       // right
      refresh_columns();
      sweep_rows<false, false>(T, B, up, dn, Lh, Rh, untracked);      // up
      publish_rows();
      __syncthreads();
    }
    bool changed = false;
    fetch_rows();
    refresh_columns();
    sweep_cols<true, false>(T, B, up, dn, Lh, Rh, changed);           // left, checked
    const uint32_t slot = (iters - 1) % 3;
    if (__builtin_amdgcn_ballot_w64(changed) != 0) {
      publish_rows();      // a neighbour band reads these rows only if another round follows, i.e. only if someone changed
      if (lane == 0) s_flag[slot] = 1;
    }
    __syncthreads();
    const bool again = s_flag[slot] != 0;
    if (tid == 0) s_flag[(slot + 2) % 3] = 0;
    if (!again) break;
    if (iters >= max_iters) { unfinished = true; break; }
  }
  WS_STAMP(0);
  WS_STAMP_VALUE(4, iters);      // (tools/diag_seam_rounds.hip)

  // ---- write back the patches that changed (16 B per lane and row), ring-carry check, flags
  uint64_t sum_after = 0;
#pragma unroll
  for (int r = 0; r < RX0_PH; ++r)
#pragma unroll
    for (int c = 0; c < RX_P; ++c) sum_after += T[r][c];
  uint32_t e = 0, ovf = 0;
  if (has_seam && sum_after != s_sum[tid]) {      // (a seam inside the plane: gx0 + RX_P <= W)
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) {
      const int gy = gyb + r;
      if (gy < H) *reinterpret_cast<u32x4_t *>(keys + (size_t)gy * W + gx0) = u32x4_t{T[r][0], T[r][1], T[r][2], T[r][3]};
      if (check_carry) {               // kernel uniform
#pragma unroll
        for (int c = 0; c < RX_P; ++c)   // a finite non-seed stamp with ring 0 (a carry) or 2^24 - 1 (the last before one: out of level 254 the carry is KEY_INF)
          ovf |= (T[r][c] != 0u && T[r][c] < KEY_INF && ((T[r][c] + 1u) & RING_MASK) <= 1u);
      }
    }
    e |= 16u;
  }
  if (ovf) atomicExch(pf.overflow, 1u);      // never taken on sane inputs (and by no test: this kernel follows a pass 0 from seeds only)
  // Flags: the word that pass 2 reads for anchored tile (x, y), word 3 of entry (x, y) of the shifted grid's stamps.
  // Why they are a superset of the pixels whose equation can be violated, on slices of 64 rows: when the strips start, an
  // equation can only be violated next to a vertical seam (pass 0's tiles and the bands are fixpoints of their own pixels, and
  // what a band changed in its outer rows it has flagged, save in the columns that lie inside a strip).  A slice that did
  // not stop at its cap is a fixpoint of its 8 x 64 pixels per seam against the halo it loaded, so what it leaves violated
  // lies (a) across one of its outer columns, next to a pixel it lowered: in the 256 x 32 tile that holds that row, on that
  // lane's side of the seam -- flagged by the lane; (b) across its first or last row, in the slice above or below, which
  // lies in the tile above or below on the same side -- flagged by the lane of band 0 / band 7 that holds the pixel; (c) at
  // its own first or last row, when the slice above or below lowered the halo row after this one had loaded it -- which is
  // that slice's case (b).  The halo columns belong to no strip and do not change during the launch.  In each case the
  // lowered pixel can only pull its neighbour down when it is at least two below what the neighbour held when the slice
  // loaded it (`matters`; the neighbour can only have fallen since, so the test errs on the side of flagging).  A slice at
  // its cap is no fixpoint: both tile rows on both sides of every seam of it run again and examine all its pixels.  Slice
  // ends lie on rows 64 k and 64 k + 63 only -- the rows 64 k + 32 are interior rows now, as they are in pass 0's tiles.
  if (has_seam) {
    const uint32_t mark = pass + 1;
    bool col = unfinished;
#pragma unroll
    for (int r = 0; r < RX0_PH; ++r) col |= matters(sInitCol[r][tid], (lane & 1) ? T[r][RX_P - 1] : T[r][0], halo[r]);
    bool top = false, bottom = false;
    if (band == 0) {
      const u32x4_t o = *reinterpret_cast<const u32x4_t *>(&sInitRow[0][lane * RX_P]);
      const u32x4_t a = *reinterpret_cast<const u32x4_t *>(&sRow[0][lane * RX_P]);      // the halo row above, as loaded
      top = matters(o.x, T[0][0], a.x) || matters(o.y, T[0][1], a.y) || matters(o.z, T[0][2], a.z) || matters(o.w, T[0][3], a.w);
    }
    if (band == NB - 1) {
      const u32x4_t o = *reinterpret_cast<const u32x4_t *>(&sInitRow[1][lane * RX_P]);
      const u32x4_t a = *reinterpret_cast<const u32x4_t *>(&sRow[2 * NB + 1][lane * RX_P]);      // the halo row below
      constexpr int l = RX0_PH - 1;
      bottom = matters(o.x, T[l][0], a.x) || matters(o.y, T[l][1], a.y) || matters(o.z, T[l][2], a.z) || matters(o.w, T[l][3], a.w);
    }
    // (a lane's eight rows lie in one tile row of the 256 x 32 grid)
    if (col && gyb < H) { stamps_cur[((size_t)(gyb / SEAM_PY) * flagSX + fx) * 4 + 3] = mark; e |= 1u; }
    if (top && y0 > 0) { stamps_cur[((size_t)((y0 - 1) / SEAM_PY) * flagSX + fx) * 4 + 3] = mark; e |= 1u; }
    if (bottom && y0 + TH < H) { stamps_cur[((size_t)((y0 + TH) / SEAM_PY) * flagSX + fx) * 4 + 3] = mark; e |= 1u; }
  }
  if (e) atomicOr(&s_edges, e);
  __syncthreads();
  if (tid == 0) {
    const uint32_t ed = s_edges;
    const uint32_t stripe = (blockIdx.x % NSTRIPE) * STRIPE_STRIDE;
    // plain, idempotent stores into striped words: no same-address atomics on the tile path
    if (ed & 1u) pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT + stripe] = 1u;
    if (ed) pf.any_change[stripe] = 1u;
    count_tile_run(pf, stripe, (uint32_t)(TW * TH / 2048), 2u * iters);      // a 64-row slice counts as two of 32 rows of `iters` rounds each
  }
}

// The tuning knobs (tools/README.md): a -DWS_TUNING build reads them here, once per process; the product's tuning_env
// knows no environment and this returns the product's constants.
static RelaxKnobs relax_knobs() {
  RelaxKnobs k;
  if (const char *e = tuning_env("WS_RELAX_SAME_GRID_FROM")) k.same_grid_from = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_QUEUE_FROM")) k.queue_from = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_PERSIST")) k.persist = atoi(e);
  if (const char *e = tuning_env("WS_RELAX_P0_ROUNDS")) k.p0_rounds = (uint32_t)atoi(e);
  k.no_seam = tuning_env("WS_RELAX_NO_SEAM") != nullptr;
  if (const char *e = tuning_env("WS_RELAX_LATE_CAP")) k.late_cap = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_SCAN_FROM")) k.scan_from = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_WIDE_CAP")) {
    if (sscanf(e, "%d,%d", &k.wide_cap_n, &k.wide_cap_c) != 2) k.wide_cap_n = k.wide_cap_c = 0;
  }
  if (const char *e = tuning_env("WS_RELAX_EARLY_CAP")) k.early_cap = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_LITE_FROM")) k.lite_from = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_CHUNK_FROM")) k.chunk_from = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_SEAM_BAND")) k.seam_band = atoi(e);
  k.no_tall = tuning_env("WS_RELAX_NO_TALL") != nullptr;
  k.no_tall_strips = tuning_env("WS_RELAX_NO_TALL_STRIPS") != nullptr;
  if (const char *e = tuning_env("WS_RELAX_LIST_FROM")) k.list_from = (uint32_t)atoi(e);
  k.no_append = tuning_env("WS_RELAX_NO_APPEND") != nullptr;
  k.no_split = tuning_env("WS_RELAX_NO_SPLIT") != nullptr;
  if (const char *e = tuning_env("WS_RELAX_PERSIST_WORKERS")) k.persist_workers = (unsigned)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_PERSIST_CAP")) k.persist_cap = (uint32_t)atoi(e);
  if (const char *e = tuning_env("WS_RELAX_PERSIST_MODE")) k.persist_queue_mode = atoi(e);
  k.persist_diag = tuning_env("WS_RELAX_PERSIST_DIAG") != nullptr;
  return k;
}

static const RelaxKnobs &relax_knobs_once() {
  static const RelaxKnobs knobs = relax_knobs();
  return knobs;
}

RelaxPlan relax_plan_for(const RelaxPlane &p, uint32_t pass) {
  RelaxGeom g;
  g.h = p.h; g.w = p.w; g.slice_h = p.slice_h; g.padded = p.padded;
  g.has_seeds = p.seed_labels != nullptr; g.seed_bits = p.seed_bits;
  g.aligned4 = ((reinterpret_cast<uintptr_t>(p.img) | p.img_stride) & 3u) == 0;
  g.stride32 = p.img_stride <= 0xFFFFFFFFull;
  g.has_list = p.tile_list != nullptr;
  g.seam_min_px = p.seam_min_px; g.persist_mode = p.persistent_pass; g.max_iters = p.max_iters;
  return relax_plan(g, pass, relax_knobs_once());
}

namespace {

// what every step of a pass is launched with
struct RelaxLaunch {
  hipStream_t s;
  const RelaxPlane &p;
  const uint32_t *prev;      // the edge stamps the pass before wrote
  uint32_t *cur;             // ... and the ones this pass writes
  uint32_t list_cap;         // entries per tile list
  int sh;                    // rows per slice
  // A carry out of the 24-bit ring field leaves a finite stamp with ring 0 in the plane (and nothing ever lowers it: the
  // true stamp does not exist).  A transform that hands the finished plane to k_resolve_local lets that kernel look for
  // it, once, instead of every write-back of every pass here (5 VALU ops per pixel in kernels that are VALU-bound).
  int check_carry;
};

// k_relax's argument list
template <int NW, bool CHUNKED, bool SCAN, bool LITE, bool SPLIT = false, int SEAM = 0, int PERSIST = 0, int SEAM_PITCH = 32>
void launch_relax(const RelaxLaunch &l, const RelaxStep &st) {
  const RelaxPlane &p = l.p;
  const uint32_t *seeds = st.seeds ? p.seed_labels : nullptr;
  k_relax<NW, CHUNKED, SCAN, LITE, SPLIT, SEAM, PERSIST, SEAM_PITCH><<<st.grid, st.block, 0, l.s>>>(
      p.img, p.img_stride, p.keys, p.h, p.w, st.tilesX, st.tilesY, st.otherX, st.otherY, st.shifted, st.chunk, p.max_level, st.pass, l.prev, l.cur, p.pf,
      st.max_iters, seeds, seeds && p.seed_bits ? 1 : 0, l.sh, l.check_carry, p.padded ? 1 : 0, p.tile_list, st.use_list, st.read_same, st.write_same,
      l.list_cap, st.append_next);
}

// tools/ only (WS_RELAX_PERSIST_DIAG): what the workers of the queue pass did
void print_queue_diagnostics(const RelaxLaunch &l, uint32_t pass) {
  uint32_t hd[RL_HDR];
  (void)hipStreamSynchronize(l.s);
  (void)hipMemcpy(hd, l.p.tile_list, sizeof hd, hipMemcpyDeviceToHost);
  fprintf(stderr, "[ws] persistent pass %u: pushed %u popped %u pending %u done %u runs %u | workers wait %.1f us, life %.1f us (sums / 512), polls %u\n", pass,
          hd[RLQ_TAIL], hd[RLQ_HEAD], hd[RLQ_PENDING], hd[RLQ_DONE], hd[RLQ_RUNS], hd[RLQ_WAIT] / 100.0 / 512.0, hd[RLQ_LIFE] / 100.0 / 512.0, hd[RLQ_POLLS]);
  const double runs = hd[RLQ_RUNS] ? hd[RLQ_RUNS] : 1;
  fprintf(stderr, "[ws]   per tile run (us): load %.2f rounds %.2f epilogue %.2f hand-in %.2f; shader clock %.0f MHz\n", hd[RLQ_PHASE] / 100.0 / runs, hd[RLQ_PHASE + 1] / 100.0 / runs,
          hd[RLQ_PHASE + 2] / 100.0 / runs, hd[RLQ_PHASE + 3] / 100.0 / runs, hd[RLQ_LIFE] ? 256.0 * hd[RLQ_PHASE + 4] / hd[RLQ_LIFE] * 100.0 : 0.0);
}

hipError_t launch_step(const RelaxLaunch &l, const RelaxStep &st) {
  const RelaxPlane &p = l.p;
  uint32_t *const list = p.tile_list;
  switch (st.kind) {
    case RelaxStep::TALL_PASS0:      // (the anchored grid's tile columns are this kernel's own)
      k_relax0_tall<<<st.grid, st.block, 0, l.s>>>(p.img, (uint32_t)p.img_stride, p.keys, p.h, p.w, st.tilesX, st.tilesX, st.otherX, p.max_level, l.cur,
                                                   const_cast<uint32_t *>(l.prev), p.pf, st.max_iters, p.seed_labels, l.sh, l.check_carry, list);
      break;
    case RelaxStep::BANDS:
      if (st.seam_pitch == RX0_TH) launch_relax<3, false, false, false, false, 1, 0, RX0_TH>(l, st);
      else if (st.nw == 2) launch_relax<2, false, false, false, false, 1>(l, st);
      else if (st.nw == 3) launch_relax<3, false, false, false, false, 1>(l, st);
      else launch_relax<4, false, false, false, false, 1>(l, st);
      break;
    case RelaxStep::STRIPS: launch_relax<RX_NW, false, false, false, false, 2>(l, st); break;
    case RelaxStep::STRIPS_TALL:
      k_relax_strips_tall<<<st.grid, st.block, 0, l.s>>>(p.img, (uint32_t)p.img_stride, p.keys, p.h, p.w, st.tilesX, st.otherX, p.max_level, st.pass, l.cur, p.pf,
                                                         st.max_iters, l.sh, l.check_carry, list);
      break;
    case RelaxStep::FULL: launch_relax<RX_NW, false, false, false>(l, st); break;
    case RelaxStep::FULL_LITE: launch_relax<RX_NW, false, false, true>(l, st); break;
    case RelaxStep::CHUNKED: launch_relax<RX_NW, true, false, true>(l, st); break;
    case RelaxStep::CHUNKED_SCAN:
    case RelaxStep::LISTED: launch_relax<RX_NW, true, true, true>(l, st); break;
    case RelaxStep::LISTED_SPLIT: launch_relax<RX_SNW, true, true, true, true>(l, st); break;
    case RelaxStep::QUEUE_FIRST_COME: launch_relax<RX_SNW, true, true, true, true, 0, 1>(l, st); break;
    case RelaxStep::QUEUE_FLOOD_ORDER: launch_relax<RX_QNW, true, true, true, true, 0, 2>(l, st); break;
    case RelaxStep::LIST_BUILD:
      k_relax_list<RX_TW, RX_NW * RX_P><<<st.grid, st.block, 0, l.s>>>(p.h, p.w, st.tilesX, st.tilesY, st.otherX, st.otherY, st.shifted, st.pass, l.prev, list, st.read_same, l.list_cap);
      break;
    case RelaxStep::LIST_BUILD_SPLIT:
      k_relax_list<RX_STW, RX_STH><<<st.grid, st.block, 0, l.s>>>(p.h, p.w, st.tilesX, st.tilesY, st.otherX, st.otherY, st.shifted, st.pass, l.prev, list, st.read_same, l.list_cap);
      break;
    case RelaxStep::LIST_REGRID:
      if (st.regrid == 2)
        k_relax_list_regrid<RX_STW, RX_QTH, RX_TW, RX_NW * RX_P><<<st.grid, st.block, 0, l.s>>>(p.h, p.w, st.tilesX, st.tilesY, st.otherX, st.otherY, st.pass, l.prev, list, l.list_cap, st.regrid);
      else
        k_relax_list_regrid<RX_STW, RX_STH, RX_TW, RX_NW * RX_P><<<st.grid, st.block, 0, l.s>>>(p.h, p.w, st.tilesX, st.tilesY, st.otherX, st.otherY, st.pass, l.prev, list, l.list_cap, st.regrid);
      break;
    case RelaxStep::LIST_ALL:
      k_relax_list_all<RX_STW, RX_STH><<<st.grid, st.block, 0, l.s>>>(p.h, p.w, st.tilesX, st.tilesY, st.pass, list, l.list_cap);
      break;
    case RelaxStep::CLEAR_RING: return hipMemsetAsync(list + RL_HDR, 0, 2 * (size_t)l.list_cap * sizeof(uint32_t), l.s);
    case RelaxStep::CLEAR_COUNTERS: return hipMemsetAsync(list + 8, 0, (RL_HDR - 8) * sizeof(uint32_t), l.s);
    case RelaxStep::CLEAR_BUCKETS:
      return hipMemsetAsync(list + pq_base(l.list_cap), 0, (PQ_HDR + (size_t)PQ_B * pq_words_per_bucket(l.list_cap)) * sizeof(uint32_t), l.s);
  }
  return hipGetLastError();
}

}  // namespace

// One relaxation pass: what relax_plan (ws_relax_plan.hpp) decides, launched step by step.
hipError_t relax_pass(hipStream_t s, const RelaxPlane &p, uint32_t pass) {
  const RelaxPlan plan = relax_plan_for(p, pass);
  const size_t cap = relax_tiles(p.h, p.w) * 4;
  const RelaxLaunch l{s, p, p.stamps + ((pass + 1) & 1) * cap, p.stamps + (pass & 1) * cap, (uint32_t)relax_tiles(p.h, p.w),
                      p.slice_h > 0 ? p.slice_h : p.h, p.carry_checked_later ? 0 : 1};
  for (int i = 0; i < plan.n; ++i) {
    const RelaxStep &st = plan.steps[i];
    const hipError_t e = launch_step(l, st);
    if (e != hipSuccess) return e;
    const bool queue = st.kind == RelaxStep::QUEUE_FIRST_COME || st.kind == RelaxStep::QUEUE_FLOOD_ORDER;
    if (queue && relax_knobs_once().persist_diag) {
      hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
      (void)hipStreamIsCapturing(s, &capturing);
      if (capturing == hipStreamCaptureStatusNone) print_queue_diagnostics(l, pass);
    }
  }
  return hipSuccess;
}

}  // namespace wsk
