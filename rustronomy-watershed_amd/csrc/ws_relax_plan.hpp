// ws_relax_plan.hpp -- the relaxation's schedule: what relax_pass (ws_relax.hip) launches for one pass of one plane.
//
// Plain C++17, no HIP: relax_plan() is a pure function of the plane's geometry, the pass number and the tuning knobs, and
// the one place where the schedule is decided.  relax_pass asks it and launches the steps it returns, one after the other;
// run_fused_form asks it whether pass 1 is two launches; tests/cpp/test_relax_plan.cpp runs it on a CPU against a table
// recorded from the function it was split out of (tests/relax_plan_cases.txt) and checks what consecutive passes must agree on.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace wsk {

constexpr int RX_TW = 256;   // tile width: 64 lanes x 4 columns
constexpr int RX_P = 4;      // patch side
constexpr int RX_NW = 8;     // 512 threads: tile 256 x 32
constexpr int RX0_PH = 2 * RX_P;              // pass 0 on 256 x 64 tiles (k_relax0_tall): rows of a lane's patch
constexpr int RX0_TH = RX_NW * RX0_PH;        // ... and its tile height: 64

// Long-range rows (k_relax, SCAN) are used only from pass RX_SCAN_FROM_PASS on (the bench field has converged by then; the
// scan costs registers, so the early passes run a variant without it).
// (r2: scans from the first round on and a cap on the rounds per tile run in those passes -- 8192^2 smooth maps, correlation
// length 16 / 64 / 256 px: 16.4 -> 13.1, 29.2 -> 22.2, 12.5 -> 10.7 ms with a cap of two (gpurun_out/r2e); three since the
// rounds of those passes are scans only and the scans DPP shifts: 8.4 -> 7.2, 8.6 -> 8.3, 4.1 -> 4.0 ms, gpurun_out/r2w/dpp.log)
constexpr uint32_t RX_SCAN_FROM_PASS = 4;
constexpr uint32_t RX_EARLY_ROUND_CAP = 4;     // rounds per tile run in passes 1 .. RX_SCAN_FROM_PASS - 1 (0: no cap): smooth 8192^2, correlation 16 px: 12.4 -> 10.4 ms
constexpr uint32_t RX_LATE_ROUND_CAP = 3;      // rounds per tile run from pass RX_SCAN_FROM_PASS on (0: no cap); see relax_plan
// Rounds per tile run of the persistent pass.  The ordinary late passes stop a tile after three (a pass ends when its slowest
// tile ends); without a pass barrier that reason is gone and a run's fixed costs (loads, stores, queue: ~10 us) are spread over
// more rounds: 8192^2 smooth maps, correlation 16 px: 6.74 ms with three, 6.36 with six, 6.28 with twelve.
constexpr uint32_t RLQ_ROUND_CAP = 6;
// first pass that runs on the grid of the pass before it (odd; see relax_plan).  8192^2 smooth maps, correlation length
// 64 / 256 px: 436 -> 260 and 516 -> 292 passes, 16.8 -> 12.6 and 11.0 -> 7.0 ms (gpurun_out/r2k, bit-exact)
constexpr uint32_t RX_SAME_GRID_FROM = 7;
constexpr uint32_t RX_LIST_FROM_PASS = 6;      // the bench field has converged by then (its passes 4 and 5 find nothing to do)
constexpr unsigned RX_LIST_GRID = 512;       // two workgroups of the scan variant per CU: all resident, the tickets share the list out
constexpr uint32_t SEAM_P0_ROUNDS = 6;      // k_relax, chunk == 3: two rounds of four sweeps, then up to four of one; k_relax0_tall: one of four, then up to five of two
// Round caps of the seam-repair flow: three rounds bring a tile of the bench field to its own fixpoint (the third finds
// nothing to do); a tile, band or strip slice of a smooth map that is still moving then asks for a re-run in pass 2 instead
// of carrying a flood across its 256 columns sweep by sweep.
constexpr uint32_t SEAM_REPAIR_ROUNDS = 4;

// the 128 x 64 grid of the same-grid passes
#ifndef WS_SPLIT_NW
#define WS_SPLIT_NW RX_NW
#endif
constexpr int RX_SNW = WS_SPLIT_NW;
constexpr int RX_STW = RX_TW / 2, RX_STH = 2 * RX_SNW * RX_P;      // tile of the SPLIT kernel: 128 x 64
// The queue in flood order runs on tiles of twice the height, 128 x 128 (sixteen waves): the launch is bound by the chain of
// tile runs along the floods, and a flood crosses half as many of these vertically.  The ordinary same-grid passes are
// slower on them (a pass lasts as long as its slowest tile); 8192^2 smooth maps, correlation 4 / 16 / 64 / 256 px, passes:
// 3.06 / 6.04 / 6.94 / 3.73 ms on 128 x 64, 3.58 / 7.23 / 7.39 / 3.48 on 128 x 128; queue: 3.78 / 7.2 / 5.12 / 4.09 against
// 3.69 / 6.75 / 4.69 / 3.65 (gpurun_out/r3am).
#ifndef WS_QUEUE_NW
#define WS_QUEUE_NW 16
#endif
constexpr int RX_QNW = WS_QUEUE_NW;
constexpr int RX_QTH = 2 * RX_QNW * RX_P;

// capacity of ONE of the two edge-stamp arrays: the shifted grid has one more row and column; the 128 x 64 grid of the
// same-grid passes has its own count
inline size_t relax_plan_tiles(int h, int w) {
  const int th = RX_NW * RX_P;
  const size_t a = (size_t)((w + RX_TW - 1) / RX_TW + 1) * ((h + th - 1) / th + 1);
  const size_t b = (size_t)((w + RX_STW - 1) / RX_STW + 1) * ((h + RX_STH - 1) / RX_STH + 1);
  return std::max(a, b);
}

// What the schedule of a transform depends on, and nothing else.
struct RelaxGeom {
  int h = 0, w = 0;
  int slice_h = 0;
  bool padded = false;
  bool has_seeds = false;      // a seed plane is given ...
  bool seed_bits = false;      // ... as one bit per pixel
  bool aligned4 = false;       // (img | img_stride) & 3 == 0: image rows can be read as aligned dwords
  bool stride32 = false;       // img_stride fits 32 bits
  bool has_list = false;       // a tile list exists
  size_t seam_min_px = (size_t)1 << 24;
  int persist_mode = 0;
  uint32_t max_iters = 0xFFFFFFFFu;      // the caller's round cap
};

// The tuning knobs (WS_RELAX_*, tools/README.md), at the product's values.  Only a -DWS_TUNING build ever sets another
// (relax_knobs, ws_relax.hip).
struct RelaxKnobs {
  uint32_t same_grid_from = RX_SAME_GRID_FROM;
  uint32_t queue_from = 3;
  int persist = -1;                  // >= 0: instead of the caller's persist_mode
  uint32_t p0_rounds = 2;
  bool no_seam = false;
  uint32_t late_cap = RX_LATE_ROUND_CAP;
  uint32_t scan_from = RX_SCAN_FROM_PASS;
  int wide_cap_n = 0, wide_cap_c = 0;      // "n,c": the first n scan passes with c rounds instead
  uint32_t early_cap = RX_EARLY_ROUND_CAP;
  uint32_t lite_from = 2;
  uint32_t chunk_from = 3;
  int seam_band = 6;
  bool no_tall = false;
  bool no_tall_strips = false;
  uint32_t list_from = RX_LIST_FROM_PASS;
  bool no_append = false;
  bool no_split = false;
  unsigned persist_workers = 0;      // 0: one per CU in flood order, all that are resident first come
  uint32_t persist_cap = RLQ_ROUND_CAP;
  int persist_queue_mode = 0;        // WS_RELAX_PERSIST_MODE: handed to the queue kernel as it is
  bool persist_diag = false;         // the launcher prints what the workers did
};

// One launch or memset of a pass.
struct RelaxStep {
  enum Kind {
    TALL_PASS0,                        // k_relax0_tall
    BANDS, STRIPS, STRIPS_TALL,        // the seam repair: k_relax SEAM 1 / SEAM 2, k_relax_strips_tall
    FULL, FULL_LITE,                   // one tile per workgroup
    CHUNKED, CHUNKED_SCAN,             // `chunk` tiles per workgroup
    LIST_BUILD, LIST_BUILD_SPLIT, LIST_REGRID, LIST_ALL,      // k_relax_list on either grid, k_relax_list_regrid, k_relax_list_all
    LISTED, LISTED_SPLIT,              // tiles from the list, 256 x 32 / 128 x 64
    QUEUE_FIRST_COME, QUEUE_FLOOD_ORDER,
    CLEAR_RING, CLEAR_COUNTERS, CLEAR_BUCKETS      // the queue's memsets
  } kind = FULL;
  int nw = RX_NW, seam_pitch = 32;      // bands: waves (rows each side of a seam: 2 nw) and the pitch of the seams they repair
  unsigned grid = 1, block = 64 * RX_NW;
  int tilesX = 0, tilesY = 0, otherX = 0, otherY = 0;
  int shifted = 0, chunk = 1;
  uint32_t max_iters = 0;
  bool seeds = false;                   // the kernel derives the stamps from the seed plane
  int use_list = 0, read_same = 0, write_same = 0, append_next = 0;
  int regrid = 0;                       // k_relax_list_regrid's mode: 0 a list, 1 / 2 the first filling of the queue
  uint32_t pass = 0;                    // the kernel's `pass` argument
};

// Today's longest pass is the queue pass: three clears, regrid, queue kernel, list-all.
constexpr int RELAX_MAX_STEPS = 6;
static_assert(RELAX_MAX_STEPS >= 3 + 1 + 1 + 1, "the queue pass must fit");

struct RelaxPlan {
  RelaxStep steps[RELAX_MAX_STEPS];
  int n = 0;
  bool seam_flow = false;      // the transform repairs pass 0's seams with bands and strips: its pass 1 is two launches
  bool tall0 = false;          // ... and its pass 0 runs on 256 x 64 tiles
  RelaxStep &add(RelaxStep::Kind kind, unsigned grid, unsigned block) {
    RelaxStep &st = steps[n++];
    st.kind = kind; st.grid = grid; st.block = block;
    return st;
  }
};

// Does a transform of this plane, started from its seeds, repair pass 0's seams with bands and strips?
// Seam repair (k_relax, SEAM): a transform that starts from its seeds runs pass 0 to every tile's own fixpoint and then,
// as "pass 1", 8-row bands astride the horizontal seams of the 256 x 32 grid and 8-column strips astride the vertical
// ones -- a third of the pixels of the shifted grid's pass, which it replaces -- and those raise the flags that pass 2
// reads.  Planes it is not offered for (odd widths, stacks of slices, the virtual halo, planes of a tile or two) keep
// the alternating grids from pass 1 on.
// (8192^2 bench field: pass 0 141 -> 168 us, pass 1 117 us -> bands 34 + strips 30 us, the later passes as before: 0.622 ->
// 0.595 ms per transform; 2048^2: 0.131 -> 0.137 ms, one more launch in a transform that is all launch gaps -- hence the
// size threshold.  Wider bands, smaller strip slices and a second, shifted strip launch were measured too: no better,
// profiles/r2_v6_seam_ab.log.)
inline bool relax_seam_flow(const RelaxGeom &g, const RelaxKnobs &k) {
  const int ax = (g.w + RX_TW - 1) / RX_TW, ay = (g.h + RX_NW * RX_P - 1) / (RX_NW * RX_P);
  // (a stack of slices takes it too: slice walls are rows of pinned pixels, wherever they fall in a band or a strip slice)
  return !k.no_seam && g.has_seeds && g.seed_bits && !g.padded && (g.w & 3) == 0 && ax >= 2 && ay >= 2 &&
         (size_t)g.h * (size_t)g.w >= g.seam_min_px;
}

// Pass 0 of that flow on 256 x 64 tiles (k_relax0_tall) wherever its one load path applies -- image rows that can be read
// as aligned dwords -- and the plane has a seam at a multiple of 64 rows for the bands to repair.  Pass 1 asks the same
// question of the same arguments, so the bands know which seams pass 0 left.
// Why the flags are still a superset of the pixels whose equation can be violated: a pass-0 tile that did not stop at its
// round cap is a fixpoint of its own pixels against the halo it loaded, so an equation can only be violated next to a
// border of a 256 x 64 tile -- the horizontal seams at rows 64 k, the vertical ones at columns 256 k.  The bands lie
// astride every row 64 k, the strips astride every column 256 k in ALL rows (in slices of 64 rows whose ends lie on the
// bands' rows: k_relax_strips_tall, where the argument is spelt out for them), each iterates to its
// own fixpoint on fresh stamps and flags the 256 x 32 tile that holds a pixel next to a changed outer row or column of
// it, exactly as before.  The rows 64 k + 32, seams of the old geometry, are interior rows of a pass-0 tile now: nothing
// is left violated there unless the tile stopped at its cap -- and then it has marked both 256 x 32 tiles it covers for
// pass 2, all of whose pixels that pass examines again.  Stamps start from an upper bound and only fall, as ever.
inline bool relax_tall0(const RelaxGeom &g, const RelaxKnobs &k) {
  return relax_seam_flow(g, k) && !k.no_tall && k.seam_band == 6 && g.h > RX0_TH && g.w >= RX_P && g.aligned4 && g.stride32;
}

inline RelaxPlan relax_plan(const RelaxGeom &g, uint32_t pass, const RelaxKnobs &k) {
  RelaxPlan plan;
  const int h = g.h, w = g.w;
  const int th = RX_NW * RX_P;
  const int ax = (w + RX_TW - 1) / RX_TW, ay = (h + th - 1) / th;     // grid anchored at (0, 0): even passes
  const int sx = ax + 1, sy = ay + 1;                                 // grid shifted by half a tile: odd passes
  const auto odd_from_3 = [](uint32_t v) { return v < 3u ? 3u : (v | 1u); };
  // Passes from RX_SAME_GRID_FROM on all run on the anchored grid (relax_todo, read_same): in the long-range regime a tile
  // that stops at its round cap goes on itself, instead of handing its area to the FOUR tiles of the other grid that
  // cover it (each of which loads 8192 pixels to work on a quarter of them).
  const uint32_t same_from_passes = odd_from_3(k.same_grid_from);      // odd: the pass before it runs on the anchored grid
  // The queue in flood order (persist_mode == 2: the caller has seen sparse seeds, or was told to) starts as early as the
  // schedule allows -- pass 3, right behind the seam repair and one pass with scans: a flood that crosses hundreds of tiles
  // gains six of them from passes 3 .. 6 and pays six launches and their host round trip for it (8192^2, 35 seeds: 0.3 of
  // 4.2 ms).  Pass 4 is then the pass that looks at every tile again; when it finds nothing to change the transform ends
  // inside the replayed graph (run_fused_form: passes 0 .. 4 and the gated resolve).
  const uint32_t queue_from = odd_from_3(k.queue_from);
  const int persist_mode = k.persist >= 0 ? k.persist : g.persist_mode;
  const size_t tiles = relax_plan_tiles(h, w);
  const uint32_t list_cap = (uint32_t)tiles;      // entries per tile list
  const bool queue_plane = persist_mode == 2 && g.has_list && !g.padded && (w & 3) == 0 && w >= RX_P && g.aligned4 && tiles < (1u << 24);
  // ... and so do the passes themselves on maps of middling seed density (persist_mode 4: the caller has seen between one
  // seed per two tiles and ~30 per tile): same grid from pass 3, scans from pass 2, lists from pass 3.  8192^2 smooth maps,
  // correlation 6 / 8 / 10 / 12 / 16 px: 3.45 / 3.79 / 4.37 / 4.68 / 5.76 -> 3.37 / 3.59 / 4.13 / 4.38 / 5.26 ms; at 4 px
  // (80 seeds per tile) the late schedule wins, 2.96 against 3.12, and a random field never gets that far (gpurun_out/r3ax, r3ay).
  const bool early_queue = (queue_plane || (persist_mode == 4 && g.has_list)) && queue_from < same_from_passes;
  const uint32_t same_from = early_queue ? queue_from : same_from_passes;
  const int read_same = pass >= same_from ? 1 : 0, write_same = pass + 1 >= same_from ? 1 : 0;
  const int shifted = read_same ? 0 : (int)(pass & 1u);
  const int tx = shifted ? sx : ax, ty = shifted ? sy : ay;
  const int ox_ = read_same ? ax : (shifted ? ax : sx), oy_ = read_same ? ay : (shifted ? ay : sy);        // the previous pass's grid
  plan.seam_flow = relax_seam_flow(g, k);
  plan.tall0 = relax_tall0(g, k);
  const bool seam_flow = plan.seam_flow, tall0 = plan.tall0;
  // Pass 0 only has to produce a good first guess: pass 1 re-examines every pixel on the shifted grid
  // anyway (a capped tile raises all four of its quadrant flags), so its last round -- the one that
  // finds nothing left to do, a third of its time on the bench field -- is not worth running.
  uint32_t max_iters = g.max_iters;
  const uint32_t p0_cap = seam_flow ? SEAM_P0_ROUNDS : k.p0_rounds;
  if (pass == 0 && p0_cap < max_iters) max_iters = p0_cap;
  // Late passes (the long-range regime of smooth maps: a few hundred tiles along the flood fronts per pass) end when their
  // SLOWEST tile ends, and a tile that the front is crossing diagonally can take a dozen rounds.  Capping the rounds lets a
  // pass end after the typical tile's work: a capped tile raises all four quadrant flags (like a capped pass-0 tile), so
  // the tiles of the other grid that cover it carry on in the next pass -- next to the front, which has moved on meanwhile.
  const uint32_t scan_from = early_queue ? same_from - 1u : std::max(k.scan_from, 1u);
  if (pass >= scan_from && k.late_cap != 0 && k.late_cap < max_iters) max_iters = k.late_cap;
  if (pass >= scan_from && pass < scan_from + (uint32_t)k.wide_cap_n) max_iters = (uint32_t)k.wide_cap_c;
  // Passes 1 .. 3 have no scans: on a smooth map a tile that iterates to its own fixpoint by sweeps alone takes up to 64
  // rounds to carry a flood across its 256 columns, all 8192 tiles of them, in a pass that the scan passes then redo.
  if (pass >= 1 && pass < scan_from && k.early_cap != 0 && k.early_cap < max_iters) max_iters = k.early_cap;

  // every k_relax step: the grid it runs on and the grid whose flags it reads
  const auto tiled = [](RelaxStep &st, int tilesX, int tilesY, int otherX, int otherY, int shifted_, int chunk, uint32_t pass_, uint32_t rounds) -> RelaxStep & {
    st.tilesX = tilesX; st.tilesY = tilesY; st.otherX = otherX; st.otherY = otherY;
    st.shifted = shifted_; st.chunk = chunk; st.pass = pass_; st.max_iters = rounds;
    return st;
  };
  const int ay_tall = (h + RX0_TH - 1) / RX0_TH;
  if (tall0 && pass == 0) {
    // (otherX: the shifted grid's tile columns, the pitch of the flags that pass 2 reads)
    tiled(plan.add(RelaxStep::TALL_PASS0, (unsigned)(ax * ay_tall), 64 * RX_NW), ax, ay_tall, sx, sy, 0, 1, pass, max_iters).seeds = true;
    return plan;
  }
  if (seam_flow && pass == 1) {
    // Rows each side of a seam (seam_band: tuning knob, tools/ only).  What pass 0 leaves wrong thins out fourfold per pixel of distance from
    // the seam, and a band raises a flag when its first or last row changes: with 4 rows a side 41 % of the tiles are flagged
    // (pass 2: 52 us), with 6 a tile in eight (25 us), with 8 one in eleven (23 us) -- and the bands cost 35 / 50 / 59 us.
    // After a tall pass 0, bands only where it has seams: rows 64 k (half the workgroups, the same twelve rows each); the strips as ever
    const int nw = tall0 ? 3 : k.seam_band == 4 ? 2 : k.seam_band == 6 ? 3 : 4;
    const int by = tall0 ? ay_tall - 1 : ay - 1;
    RelaxStep &bands = tiled(plan.add(RelaxStep::BANDS, (unsigned)(ax * by), 64u * nw), ax, by, sx, sy, 0, 1, pass, SEAM_REPAIR_ROUNDS);
    bands.nw = nw;
    bands.seam_pitch = tall0 ? RX0_TH : 32;
    const int strips_x = (ax - 1 + 31) / 32;
    // After pass 0 on 256 x 64 tiles the strips run on slices of 64 rows, whose ends lie where the bands have run
    // (k_relax_strips_tall); every other flow keeps its 32-row slices.
    if (tall0 && !k.no_tall_strips)
      tiled(plan.add(RelaxStep::STRIPS_TALL, (unsigned)(strips_x * ay_tall), 64 * RX_NW), strips_x, ay_tall, sx, sy, 0, 1, pass, SEAM_REPAIR_ROUNDS);
    else
      tiled(plan.add(RelaxStep::STRIPS, (unsigned)(strips_x * ay), 64 * RX_NW), strips_x, ay, sx, sy, 0, 1, pass, SEAM_REPAIR_ROUNDS);
    return plan;
  }
  const auto same_or_other = [&](RelaxStep &st, int use_list, int append_next) {
    st.use_list = use_list; st.read_same = read_same; st.write_same = write_same; st.append_next = append_next;
  };
  // passes 0 and 1 run every tile and pass 2 about half of them (bench field): one tile per workgroup
  // (pass 2 after a seam repair runs a tile in ten: a workgroup per four tiles, as in the later passes)
  const uint32_t chunk_from_now = seam_flow ? std::min(k.chunk_from, 2u) : k.chunk_from;
  if (pass < chunk_from_now) {
    const bool lite = pass >= k.lite_from;
    RelaxStep &st = tiled(plan.add(lite ? RelaxStep::FULL_LITE : RelaxStep::FULL, (unsigned)(tx * ty), 64 * RX_NW), tx, ty, ox_, oy_, shifted,
                          !lite && seam_flow && pass == 0 ? 3 : 1, pass, max_iters);
    st.seeds = pass == 0;
    same_or_other(st, 0, 0);
    return plan;
  }
  const int chunk = 4;
  const unsigned grid = (unsigned)((tx * ty + chunk - 1) / chunk);
  const uint32_t list_from = early_queue ? same_from : k.list_from;
  if (pass < scan_from) {
    same_or_other(tiled(plan.add(RelaxStep::CHUNKED, grid, 64 * RX_NW), tx, ty, ox_, oy_, shifted, chunk, pass, max_iters), 0, 0);
    return plan;
  }
  if (!(g.has_list && pass >= list_from && pass >= scan_from + 1)) {
    same_or_other(tiled(plan.add(RelaxStep::CHUNKED_SCAN, grid, 64 * RX_NW), tx, ty, ox_, oy_, shifted, chunk, pass, max_iters), 0, 0);
    return plan;
  }
  // (two passes earlier a launch has cleared this pass's counter: every kernel variant does, given a list)
  // From the second same-grid pass on the list is there already: the tiles of the pass before appended it.
  const uint32_t first_list_pass = std::max(list_from, scan_from + 1);
  const int append_next = !k.no_append && pass >= same_from && pass >= first_list_pass ? 1 : 0;
  const bool appended = !k.no_append && pass >= 1 && pass - 1 >= same_from && pass - 1 >= first_list_pass;
  // The same-grid passes run on 128 x 64 tiles (k_relax, SPLIT); the first of them builds its list from the stamps the
  // 256 x 32 grid left behind.
  const bool split = !k.no_split && pass >= same_from && same_from >= first_list_pass;
  const int gx = split ? (w + RX_STW - 1) / RX_STW : tx, gy = split ? (h + RX_STH - 1) / RX_STH : ty;
  if (!appended) {
    // (one thread per tile and a few more: the queued marks, dummy slot included, are cleared here)
    const unsigned blocks = (unsigned)((std::max<size_t>((size_t)gx * gy, list_cap + 1) + 255) / 256);
    // The first same-grid pass as ONE persistent launch (k_relax, PERSIST): workgroups pull tiles from a queue and a tile
    // that changes something its neighbour must see queues that neighbour at once.  The pass after it runs every tile
    // from an all-tiles list, so the fixpoint is certified by the ordinary machinery whatever the queue did.
    // 8192^2 smooth maps, correlation length 4 / 16 / 64 / 256 px (profiles/r3_v1_persistent_ab.txt): 3.0 / 5.8 / 6.7 / 3.5 ms
    // with the passes; first come (mode 1) 3.0 / 6.4 / 6.4 / 4.1 -- a tile run costs 13-17 us either way (4 us of loads past
    // L2, 4-8 of scan rounds, 3 of write-through stores, 2 of queue atomics), the queue saves the launch gaps and the
    // tails of the passes and pays for them with a sixth more tile runs (a tile runs on the first flag instead of on all
    // flags of a pass); in flood order (mode 2, from pass 3, on 128 x 128 tiles) 4.2 / 5.8 / 3.9 / 3.0: a third of the
    // tile runs, and a win where floods are long.  The context picks mode 2 by itself when seeds are sparse
    // (run_fused_form); ws_ctx_set_persistent_pass forces or forbids.
    const bool persist = (persist_mode == 1 || persist_mode == 2) && split && pass == same_from && !g.padded && (w & 3) == 0 && w >= RX_P &&
                         g.aligned4 && (size_t)gx * gy <= list_cap && list_cap < (1u << 24);
    if (persist) {
      const bool in_order = persist_mode == 2;      // buckets in flood order (PERSIST == 2) instead of the first-come ring
      plan.add(RelaxStep::CLEAR_RING, 1, 1);          // the ring: no entry yet
      plan.add(RelaxStep::CLEAR_COUNTERS, 1, 1);      // counters (and diagnostics)
      if (in_order) plan.add(RelaxStep::CLEAR_BUCKETS, 1, 1);
      const int qy = in_order ? (h + RX_QTH - 1) / RX_QTH : gy;      // (flood order: the queue's own grid, 128 x 128)
      RelaxStep &regrid = tiled(plan.add(RelaxStep::LIST_REGRID, blocks, 256), gx, qy, ax, ay, 0, 1, pass, 0);
      regrid.regrid = in_order ? 2 : 1;
      // In flood order: one worker per CU.  Two (all that are resident) run twice as long each, the rounds too -- a
      // workgroup is one wave per SIMD, and two share their vector issue -- so nothing is gained where all are busy, and
      // where most are idle their looks at the counts are in the way: 8192^2 smooth maps, correlation 4 / 16 / 64 / 256 px,
      // 3.89 / 7.75 / 5.73 / 4.14 ms with 512 workers, 3.82 / 7.22 / 4.98 / 3.98 with 256 (gpurun_out/r3z).
      const unsigned workers = k.persist_workers ? k.persist_workers
                                                 : std::min<unsigned>(in_order ? RX_LIST_GRID / 2 : RX_LIST_GRID * RX_NW / RX_SNW, (unsigned)(gx * qy));
      RelaxStep &queue = tiled(plan.add(in_order ? RelaxStep::QUEUE_FLOOD_ORDER : RelaxStep::QUEUE_FIRST_COME, workers, 64u * (in_order ? RX_QNW : RX_SNW)),
                               gx, qy, gx, qy, 0, chunk, pass, k.persist_cap);
      queue.use_list = k.persist_queue_mode; queue.read_same = 1; queue.write_same = 1; queue.append_next = 1;
      tiled(plan.add(RelaxStep::LIST_ALL, blocks, 256), gx, gy, gx, gy, 0, 1, pass + 1, 0);
      return plan;
    }
    if (split && pass == same_from) {
      tiled(plan.add(RelaxStep::LIST_REGRID, blocks, 256), gx, gy, ax, ay, 0, 1, pass, 0);
    } else if (split) {
      tiled(plan.add(RelaxStep::LIST_BUILD_SPLIT, blocks, 256), gx, gy, gx, gy, 0, 1, pass, 0).read_same = 1;
    } else {
      tiled(plan.add(RelaxStep::LIST_BUILD, blocks, 256), tx, ty, ox_, oy_, shifted, 1, pass, 0).read_same = read_same;
    }
  }
  if (split) {
    RelaxStep &st = tiled(plan.add(RelaxStep::LISTED_SPLIT, std::min<unsigned>(RX_LIST_GRID * RX_NW / RX_SNW, (unsigned)(gx * gy)), 64 * RX_SNW),
                          gx, gy, gx, gy, 0, chunk, pass, max_iters);
    st.use_list = 1; st.read_same = 1; st.write_same = 1; st.append_next = append_next;
  } else {
    same_or_other(tiled(plan.add(RelaxStep::LISTED, std::min<unsigned>(RX_LIST_GRID, (unsigned)(tx * ty)), 64 * RX_NW), tx, ty, ox_, oy_, shifted, chunk, pass, max_iters),
                  1, append_next);
  }
  return plan;
}

}  // namespace wsk
