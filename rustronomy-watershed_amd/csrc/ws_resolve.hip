// ws_resolve.hip -- label resolve of the fused engine (gfx950, wave64): with the stamps final, every pixel takes the
// colour of the seed at the root of its parent chain.
//
//   k_resolve                           iterative form, one launch per pass (resolve_pass): planes of 2^31 pixels or
//                                       more, and the row blocks of ws_block_init / _relax / _resolve
//   k_resolve_local + k_resolve_chase   two-launch form (resolve_two_launch, a ResolveJob): every fused transform.
//                                       Their constants and follow_chain are in ws_resolve_tile.hpp; the phases of
//                                       both kernels are numbered sections of the kernel bodies (see k_resolve_local).
#include "ws_common.hpp"
#include "ws_resolve_tile.hpp"

#include <algorithm>

namespace wsk {

// ------------------------------------------------------- tile scheduling helper ----
//
// A tile re-runs in pass p only if a neighbour changed the edge it shares with it in pass p-1
// (edge stamps, double buffered by pass parity; layout per tile: 0 top, 1 bottom, 2 left, 3 right;
// value = pass + 1 of the writer).

__device__ __forceinline__ bool tile_must_run(const uint32_t *stamps_prev, int tx, int ty, int tilesX,
                                              int tilesY, uint32_t pass) {
  if (pass == 0) return true;
  // stamp layout per tile: 0 top, 1 bottom, 2 left, 3 right; value = pass+1 of the writer
  const int t = ty * tilesX + tx;
  bool run = false;
  if (ty > 0) run |= stamps_prev[(size_t)(t - tilesX) * 4 + 1] == pass;
  if (ty + 1 < tilesY) run |= stamps_prev[(size_t)(t + tilesX) * 4 + 0] == pass;
  if (tx > 0) run |= stamps_prev[(size_t)(t - 1) * 4 + 3] == pass;
  if (tx + 1 < tilesX) run |= stamps_prev[(size_t)(t + 1) * 4 + 2] == pass;
  return run;
}

size_t resolve_tiles(int h, int w) { return (size_t)tiles_of(w) * tiles_of(h); }

// ---------------------------------------------------- fused engine: label resolve ----
//
// With the stamps final, the colour of a pixel is the colour of its parent: the first
// neighbour in down,right,left,up order (lib.rs:190) that was coloured strictly earlier
// (lib.rs:237-248, col0).  Parents form a forest rooted at the seeds.  A tile computes the
// parent direction of its 16 pixels per thread once, then pulls labels along the forest
// until nothing changes; labels only ever go 0 -> final, so a coloured pixel is done.

__global__ __launch_bounds__(NTHREADS) void k_resolve(const uint32_t *__restrict__ keys, uint32_t *labels,
                                                      int H, int W, int tilesX, int tilesY, uint32_t pass,
                                                      uint32_t *stamps, PassFlags pf) {
  __shared__ uint32_t sB[LP][LP];
  __shared__ uint32_t s_edges;

  const int tile_x = blockIdx.x % tilesX, tile_y = blockIdx.x / tilesX;
  const size_t ntiles = (size_t)tilesX * tilesY;
  const uint32_t *stamps_prev = stamps + ((pass + 1) & 1) * ntiles * 4;
  uint32_t *stamps_cur = stamps + (pass & 1) * ntiles * 4;
  if (blockIdx.x == 0 && threadIdx.x < NSTRIPE)
    pf.edge_changed[((pass + 1) % COUNTER_RING) * FLAG_SLOT + threadIdx.x * STRIPE_STRIDE] = 0;
  if (!tile_must_run(stamps_prev, tile_x, tile_y, tilesX, tilesY, pass)) return;

  const int tid = threadIdx.x;
  const int lane = tid & 63, strip = tid >> 6;
  const int x0 = tile_x * TS, y0 = tile_y * TS;
  const int lx = lane + 1, ly0 = strip * STRIP + 1;
  const int gx = x0 + lane, gy0 = y0 + strip * STRIP;
  if (tid == 0) s_edges = 0;

  // phase 1: stamps -> LDS, parent directions -> registers
  for (int idx = tid; idx < LP * LP; idx += NTHREADS) {
    const int ly = idx / LP, lxx = idx - ly * LP;
    const int gy = y0 - 1 + ly, gxx = x0 - 1 + lxx;
    uint32_t v = KEY_INF;
    if (gy >= 0 && gy < H && gxx >= 0 && gxx < W) v = keys[(size_t)gy * W + gxx];
    sB[ly][lxx] = v;
  }
  __syncthreads();
  uint32_t dirs = 0;      // 2 bits per pixel: 0 down, 1 right, 2 left, 3 up
  uint32_t has_parent = 0;
#pragma unroll
  for (int i = 0; i < STRIP; ++i) {
    const uint32_t k = sB[ly0 + i][lx];
    const int gy = gy0 + i;
    // flooded pixels are interior pixels (lib.rs:220-222).  On a row block of a larger field the
    // first/last local rows are halo copies whose down/up neighbour is not here, so their parent
    // cannot be decided locally: they are left to the owning rank.
    if (k != 0u && k != KEY_INF && gy >= 1 && gy < H - 1 && gx >= 1 && gx < W - 1) {
      const uint32_t d = sB[ly0 + i + 1][lx], r = sB[ly0 + i][lx + 1];
      const uint32_t l = sB[ly0 + i][lx - 1];
      const uint32_t dir = d < k ? 0u : (r < k ? 1u : (l < k ? 2u : 3u));   // at a fixpoint one of the four is < k
      dirs |= dir << (2 * i);
      has_parent |= 1u << i;
    }
  }
  __syncthreads();

  // phase 2: labels -> the same LDS tile
  for (int idx = tid; idx < LP * LP; idx += NTHREADS) {
    const int ly = idx / LP, lxx = idx - ly * LP;
    const int gy = y0 - 1 + ly, gxx = x0 - 1 + lxx;
    uint32_t v = 0;
    if (gy >= 0 && gy < H && gxx >= 0 && gxx < W) v = labels[(size_t)gy * W + gxx];
    sB[ly][lxx] = v;
  }
  __syncthreads();
  uint32_t own[STRIP];
#pragma unroll
  for (int i = 0; i < STRIP; ++i) own[i] = sB[ly0 + i][lx];

  uint32_t todo = 0;      // pixels with a parent and no colour yet
#pragma unroll
  for (int i = 0; i < STRIP; ++i) todo |= (((has_parent >> i) & 1u) && own[i] == 0u) ? (1u << i) : 0u;
  uint32_t changed_mask = 0;

  for (;;) {
    int changed = 0;
    if (todo) {
#pragma unroll
      for (int i = 0; i < STRIP; ++i) {
        if ((todo >> i) & 1u) {
          const uint32_t dir = (dirs >> (2 * i)) & 3u;
          const uint32_t vd = (i == STRIP - 1) ? sB[ly0 + STRIP][lx] : own[i + 1];
          const uint32_t vu = (i == 0) ? sB[ly0 - 1][lx] : own[i - 1];
          const uint32_t vr = sB[ly0 + i][lx + 1], vl = sB[ly0 + i][lx - 1];
          const uint32_t src = dir == 0u ? vd : (dir == 1u ? vr : (dir == 2u ? vl : vu));
          if (src) { own[i] = src; sB[ly0 + i][lx] = src; todo &= ~(1u << i); changed = 1; changed_mask |= 1u << i; }
        }
      }
#pragma unroll
      for (int i = STRIP - 1; i >= 0; --i) {
        if ((todo >> i) & 1u) {
          const uint32_t dir = (dirs >> (2 * i)) & 3u;
          const uint32_t vd = (i == STRIP - 1) ? sB[ly0 + STRIP][lx] : own[i + 1];
          const uint32_t vu = (i == 0) ? sB[ly0 - 1][lx] : own[i - 1];
          const uint32_t vr = sB[ly0 + i][lx + 1], vl = sB[ly0 + i][lx - 1];
          const uint32_t src = dir == 0u ? vd : (dir == 1u ? vr : (dir == 2u ? vl : vu));
          if (src) { own[i] = src; sB[ly0 + i][lx] = src; todo &= ~(1u << i); changed = 1; changed_mask |= 1u << i; }
        }
      }
    }
    if (!__syncthreads_or(changed)) break;
  }

  if (gx < W) {
#pragma unroll
    for (int i = 0; i < STRIP; ++i) {
      const int gy = gy0 + i;
      if (((changed_mask >> i) & 1u) && gy < H) labels[(size_t)gy * W + gx] = own[i];
    }
  }
  uint32_t e = 0;
  if (strip == 0 && (changed_mask & 1u)) e |= 1u;
  if (strip == (NTHREADS / 64) - 1 && (changed_mask >> (STRIP - 1))) e |= 2u;
  if (lane == 0 && changed_mask) e |= 4u;
  if (lane == 63 && changed_mask) e |= 8u;
  if (changed_mask) e |= 16u;                                             // anything at all
  if (e) atomicOr(&s_edges, e);
  __syncthreads();
  if (tid == 0) {
    const uint32_t ed = s_edges;
    if (ed) {
      const size_t t = (size_t)tile_y * tilesX + tile_x;
      if (ed & 1u) stamps_cur[t * 4 + 0] = pass + 1;
      if (ed & 2u) stamps_cur[t * 4 + 1] = pass + 1;
      if (ed & 4u) stamps_cur[t * 4 + 2] = pass + 1;
      if (ed & 8u) stamps_cur[t * 4 + 3] = pass + 1;
      // plain, idempotent stores into striped words (no same-address atomics on the tile path)
      const uint32_t stripe = (blockIdx.x % NSTRIPE) * STRIPE_STRIDE;
      if (ed & 15u) pf.edge_changed[(pass % COUNTER_RING) * FLAG_SLOT + stripe] = 1u;
      pf.any_change[stripe] = 1u;
    }
  }
}

hipError_t resolve_pass(hipStream_t s, const uint32_t *keys, uint32_t *labels, int h, int w,
                        uint32_t pass, uint32_t *stamps, PassFlags pf) {
  const int tx = tiles_of(w), ty = tiles_of(h);
  k_resolve<<<tx * ty, NTHREADS, 0, s>>>(keys, labels, h, w, tx, ty, pass, stamps, pf);
  return hipGetLastError();
}

// ------------------------------------ fused engine: label resolve, two-launch form ----
//
// Same forest as k_resolve, but resolved without iterating over launches:
//   k_resolve_local  every tile builds the parent pointers of its pixels in LDS and collapses the
//                    in-tile part of the forest by pointer jumping (log2(depth) rounds; a pixel whose
//                    parent is a seed -- about half of them on a random field -- takes no part).  A pixel
//                    whose root is a seed of the tile gets that seed's colour; a pixel whose chain
//                    leaves the tile gets a REFERENCE to the halo pixel where it leaves
//                    (REF_BIT | global pixel index) instead of a colour.
//   k_resolve_chase  follows references until a colour is found.  A reference always points to a
//                    pixel with a strictly smaller stamp, so chains end at a seed; concurrent
//                    updates only ever replace a reference by what it resolves to.
// Needs pixel indices < 2^31 (planes up to 46340^2); larger planes use the k_resolve loop.

// TABLES: the seeds were never painted; their colours come from the side tables of a strictly
// increasing seed list (k_seed_tables) and every pixel of the plane is written here.
// MERGE: the merging transform's final-labels path wants to know, per 64 x 64 tile, whether the tile is one lake
// (every image-interior pixel coloured) and a colour to stand for it -- both are lying around here: tile_min[tile] =
// a colour of the tile that is not a reference (0: not one lake; RL_TILE_UNDECIDED: one lake, but every pixel's
// chain leaves the tile, k_tile_scan looks at the finished labels).  Saves a 268 MB pass over the label plane.
// With halo seeds' colours (below) tile_min may be the colour of a seed in the NEIGHBOURING tile.  It is still a colour that
// some pixel of this tile holds in the finished plane, and nothing in ws_merge_final.hip asks for more: k_tile_scan, the same
// word's other source, takes the smallest colour of the finished labels, foreign ones included; k_tile_links and k_tile_roots
// join and replace colours; k_union_seeds joins every seed of the tile with it (one lake: all of the tile is one set, whichever
// member names it); k_tile_edges joins the edge pixels' colours with it.  A corner pixel is never flooded, so it never holds a
// halo's colour and stays out as before.
// BLOCK: the plane's first / last row (a row block of a larger field, ws_block_*: halo_flags bit 0 / 1) or its whole border
// ring (a tile of a field cut both ways) holds other ranks' pixels: finite stamps that are not flooded here (phase 2 keeps
// the border masks).  With TABLES a halo pixel that some flood reached (finite, non-zero stamp) has a colour only its owner
// knows: it stands for itself as a REFERENCE (phase 4), so every chain that ends on it is left as a reference to it
// (k_resolve_chase stops at halo pixels) until ws_block_import_boundary has written the halo rows' true colours.
// SH: always H.  No caller has a slice height for this kernel any more (ResolveJob has none: a stack of slices resolves like
// one plane, and BLOCK, the only reader, never had one); the argument and phase 2's arithmetic on it stay because every form
// of the row mask without them changed the registers of a BLOCK instantiation (profiles/resolve_kernel_resources.txt).
//
// The phases, in order; a barrier separates each from the next use of the LDS tile:
//   1  load           stamps of the patch and the halo ring -> registers and LDS; labels or table words -> registers
//   2  parents        the branch-free parent pointer of every pixel, the carry test; the tile becomes pointers
//   3  jump           barrier-free pointer jumping
//   4  colours        seed colours from the tables (TABLES), halo rows' references (BLOCK && TABLES); TABLES && !BLOCK: ahead of
//                     phase 3's closing barrier (it touches no LDS but the halo colours it publishes)
//   5  store          colours and halo references -- or, TABLES && !BLOCK, halo seeds' colours -- through LDS, refmask, the stores
//   6  classify       tile_min (MERGE)
//   7  references     per-wave count word and list
// They are sections of this body, not functions: a function is simplified by the compiler on its own before it is inlined,
// and every cut tried changed the instructions, and most the registers, spills or occupancy, of some instantiation
// (profiles/resolve_kernel_resources.txt has the figures of each).  The kernel is the code it was in ws_kernels.hip.
template <bool TABLES, bool MERGE, bool BLOCK>
__global__ __launch_bounds__(NTHREADS, 5) void k_resolve_local(const uint32_t *__restrict__ keys, uint32_t *labels,
                                                            int H, int W, int tilesX, uint32_t *ref_count,
                                                            uint32_t *ref_list, uint32_t max_rounds,
                                                            const uint32_t *__restrict__ seed_mask,
                                                            const uint32_t *__restrict__ word_base, uint32_t *tile_min,
                                                            const uint32_t *__restrict__ gate, int SH, uint32_t *carry_flag,
                                                            const uint32_t *__restrict__ seed_err, int halo_flags) {
  // One LDS tile, used three times: stamps (+ halo ring) -> parent pointers -> painted colours.
  // (HALO_SEEDS, below: one word per halo cell behind the tile)
  __shared__ __attribute__((aligned(16))) uint32_t sB[RL_ROWS * RL_P + (TABLES && !BLOCK ? NTHREADS : 0)];
  // Side tables built from a seed list that turned out not to be strictly increasing, or to leave the plane, describe
  // some other list: nothing may be computed from them (the host repeats the transform once it has read the same words).
  // k_seed_tables has finished before this kernel starts, so the words are final: [0] out of bounds, [2] not strict.
  if (TABLES && seed_err && (seed_err[0] | seed_err[2]) != 0u) return;
  // Speculative launch (ws_segment.hip): queued behind a relaxation pass before the host knows whether that pass still
  // changed anything.  `gate` is the pass's striped convergence slot: any word set -> not a fixpoint yet, leave.
  if (gate && __builtin_amdgcn_ballot_w64(gate[(threadIdx.x & 63) * STRIPE_STRIDE] != 0u) != 0ull) return;
  const uint32_t tile = xcd_span_index(blockIdx.x, gridDim.x);
  const int tile_x = tile % tilesX, tile_y = tile / tilesX;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int pc = tid & 15, pr = tid >> 4;
  const int x0 = tile_x * TS, y0 = tile_y * TS;
  const int gx0 = x0 + pc * 4, gy0 = y0 + pr * 4;
  const int lx0 = RL_X0 + pc * 4, ly0 = 1 + pr * 4;
  WS_STAMP(0);

  // ---- phase 1, load.  Unconditional loads on clamped addresses (see ws_relax.hip)
  uint32_t K[4][4], Lb[4][4];
  // A halo cell that is a SEED of the plane holds the seed's colour instead of a reference (phases 4 and 5): with the tables,
  // on the 16-byte path, outside a row block.
  constexpr bool HALO_SEEDS = TABLES && !BLOCK;
  // ... sHaloColour[tid]: the colour halo cell (side, t) = (tid >> 6, tid & 63) would have as a seed, published ahead of barriers
  // that exist anyway -- top and bottom rows by the halo threads in phase 1, left and right columns by the lanes of the
  // tile's first and last patch column in phase 4 -- and picked up by the halo threads in phase 5.
  uint32_t *const sHaloColour = sB + RL_ROWS * RL_P;      // (16-byte aligned: RL_ROWS * RL_P % 4 == 0)
  uint32_t seedbits = 0;                         // TABLES: which pixels of the patch are seeds
  uint32_t tab_mask[4] = {0u, 0u, 0u, 0u}, tab_base[4] = {0u, 0u, 0u, 0u};   // TABLES, vec: the table words of the 4 patch rows
  const bool vec = (W & 3) == 0 && ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  if (vec) {          // W % 4 == 0: a patch is wholly inside or wholly outside the plane in x
    const int gxc = min(gx0, W - 4);
    u32x4_r kv[4], lv[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const size_t g = (size_t)min(gy0 + r, H - 1) * W + gxc;
      kv[r] = *reinterpret_cast<const u32x4_r *>(keys + g);
      if (TABLES) {      // requested with the stamps (a late load would stall the whole workgroup after the rounds);
        tab_mask[r] = seed_mask[g >> 5];      // 8 registers across the jumping rounds instead of 16 colours
        tab_base[r] = word_base[g >> 5];
        lv[r] = u32x4_r{0u, 0u, 0u, 0u};
      } else {
        lv[r] = *reinterpret_cast<const u32x4_r *>(labels + g);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      K[r][0] = kv[r].x; K[r][1] = kv[r].y; K[r][2] = kv[r].z; K[r][3] = kv[r].w;
      Lb[r][0] = lv[r].x; Lb[r][1] = lv[r].y; Lb[r][2] = lv[r].z; Lb[r][3] = lv[r].w;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const size_t g = (size_t)min(gy0 + r, H - 1) * W + min(gx0 + c, W - 1);
        K[r][c] = keys[g];
        Lb[r][c] = TABLES ? 0u : labels[g];
      }
  }
  {
    // halo ring: thread t loads (top, bottom, left, right)[t & 63]
    const int side = tid >> 6, t = tid & 63;
    const int hy = side == 0 ? y0 - 1 : (side == 1 ? y0 + TS : y0 + t);
    const int hx = side == 2 ? x0 - 1 : (side == 3 ? x0 + TS : x0 + t);
    const size_t hg = (size_t)min(max(hy, 0), H - 1) * W + min(max(hx, 0), W - 1);
    const uint32_t hv = keys[hg];
    const bool hok = hy >= 0 && hy < H && hx >= 0 && hx < W;
    // the table words of a top / bottom halo row: requested with the stamps, two coalesced loads in waves 0 and 1 only (`side`
    // is wave uniform; the row's 64 cells lie in two or three consecutive words, one cache line per table)
    uint32_t hmask = 0u, hbase = 0u;
    if (HALO_SEEDS && vec && side < 2) { hmask = seed_mask[hg >> 5]; hbase = word_base[hg >> 5]; }
    // (workgroup uniform: a tile that lies wholly inside the plane has nothing to mask -- this kernel is bound by vector issue)
    if (!(x0 + TS <= W && y0 + TS <= H)) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (!(gy0 + r < H && gx0 + c < W)) { K[r][c] = KEY_INF; Lb[r][c] = 0u; }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (TABLES && K[r][c] == 0u) seedbits |= 1u << (r * 4 + c);      // only a seed (stamp 0) has a colour of its own
      *reinterpret_cast<u32x4_r *>(&sB[(ly0 + r) * RL_P + lx0]) = u32x4_r{K[r][0], K[r][1], K[r][2], K[r][3]};
    }
    sB[(hy - (y0 - 1)) * RL_P + (hx - (x0 - 1)) + (RL_X0 - 1)] = hok ? hv : KEY_INF;
    // phase 4's formula gives the colour of any pixel that is a seed
    if (HALO_SEEDS && vec && side < 2) sHaloColour[tid] = hbase + __popc(hmask & ((1u << (hg & 31u)) - 1u)) + 1u;
  }
  __syncthreads();
  WS_STAMP(1);

  // ---- phase 2, parents: the parent pointer of every pixel of the patch.  A pointer carries RL_FINAL when its target is a
  // root of the in-tile forest (a seed, or a halo cell = where the chain leaves the tile): such a
  // pixel never enters the jumping rounds.  Roots point at themselves.
  uint32_t P[4][4];
  uint32_t carried = 0u;
  uint32_t live = 0;                             // pixels whose pointer may still move
  {
    const u32x4_r up4 = *reinterpret_cast<const u32x4_r *>(&sB[(ly0 - 1) * RL_P + lx0]);
    const u32x4_r dn4 = *reinterpret_cast<const u32x4_r *>(&sB[(ly0 + 4) * RL_P + lx0]);
    const uint32_t up[4] = {up4.x, up4.y, up4.z, up4.w}, dn[4] = {dn4.x, dn4.y, dn4.z, dn4.w};
    uint32_t Lc[4], Rc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { Lc[r] = sB[(ly0 + r) * RL_P + lx0 - 1]; Rc[r] = sB[(ly0 + r) * RL_P + lx0 + 4]; }
    // Branch-free on purpose, 0/1 words and selects only: written with `if` / `&&` this block compiled
    // to ~75 instructions per pixel of exec-mask juggling and was the longest phase of the kernel.
    const uint32_t top_halo = pr == 0, bot_halo = pr == 15, left_halo = pc == 0, right_halo = pc == 15;
    uint32_t row_int[4], col_int[4];
    const int ry0 = SH == H ? gy0 : gy0 % SH;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ry = ry0 + i >= SH ? ry0 + i - SH : ry0 + i;       // row inside its slice (SH == H: one image)
      row_int[i] = (uint32_t)(ry >= 1) & (uint32_t)(ry < SH - 1) & (uint32_t)(gy0 + i < H);
      col_int[i] = (uint32_t)(gx0 + i >= 1) & (uint32_t)(gx0 + i < W - 1);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const uint32_t cell = (uint32_t)((ly0 + r) * RL_P + lx0 + c);
        const uint32_t k = K[r][c];
        // flooded pixels are interior pixels (lib.rs:220-222) with a finite, non-seed stamp.  The relaxation never lowers the
        // stamp of a border pixel of the image (or of a slice of a stack: its base is KEY_INF), so such a pixel is a seed or
        // never coloured and the stamp alone says "not flooded"; only a row block's halo rows hold finite stamps on a border
        // row (a neighbour rank's): BLOCK keeps the masks.
        const uint32_t flood = BLOCK ? (uint32_t)(k - 1u < KEY_INF - 1u) & row_int[r] & col_int[c] : (uint32_t)(k - 1u < KEY_INF - 1u);
        // a finite stamp of a flooded pixel with ring 0 -- a carry out of the 24-bit ring field -- or with ring 2^24 - 1, the
        // last before one: out of level 254 the carry itself is KEY_INF, "never coloured", and shows nowhere (the relaxation
        // of a whole transform leaves this test to the one kernel that reads the finished plane)
        // (largest, over the flooded pixels, of the ring field of stamp - 1 moved to the top of the word: 0xFFFFFF00 = ring 0,
        // 0xFFFFFE00 = ring 2^24 - 1, every other ring less; stamp - 1 is there already, for `flood`: a shift, a select and the
        // maximum per pixel.  The same test on stamp + 1 with a minimum flipped this kernel's register allocation.)
        carried = max(carried, flood ? (k - 1u) << 8 : 0u);
        const uint32_t d = r == 3 ? dn[c] : K[r + 1][c];
        const uint32_t rr = c == 3 ? Rc[r] : K[r][c + 1];
        const uint32_t l = c == 0 ? Lc[r] : K[r][c - 1];
        const uint32_t u = r == 0 ? up[c] : K[r - 1][c];
        // first earlier neighbour in D,R,L,U (lib.rs:190, 245); "up" is the fall-through: at a
        // fixpoint one of the four is earlier
        const uint32_t td = d < k, tr = rr < k, tl = l < k;
        const uint32_t tgt = cell + (uint32_t)(td ? RL_P : (tr ? 1 : (tl ? -1 : -RL_P)));
        const uint32_t kp = td ? d : (tr ? rr : (tl ? l : u));
        // does the chosen step leave the tile?  (r, c are compile-time: most terms vanish)
        uint32_t out_of_tile = 0;
        if (r == 3) out_of_tile |= td & bot_halo;
        if (c == 3) out_of_tile |= (td ^ 1u) & tr & right_halo;
        if (c == 0) out_of_tile |= (td ^ 1u) & (tr ^ 1u) & tl & left_halo;
        if (r == 0) out_of_tile |= (td ^ 1u) & (tr ^ 1u) & (tl ^ 1u) & top_halo;
        const uint32_t fin = (uint32_t)(kp == 0u) | out_of_tile;
        const uint32_t moving = tgt | (fin ? RL_FINAL : 0u) | (out_of_tile ? RL_HALO : 0u);
        P[r][c] = flood ? moving : (cell | RL_FINAL);
        live |= (flood & (fin ^ 1u)) << (r * 4 + c);
      }
    }
  }
  if (carry_flag && carried >= 0xFFFFFE00u) atomicExch(carry_flag, 1u);      // never taken on sane inputs (tests/test_gpu_planted_stamps.py plants the others)
  __syncthreads();                               // every stamp has been read: the tile becomes pointers
#pragma unroll
  for (int r = 0; r < 4; ++r)
    *reinterpret_cast<u32x4_r *>(&sB[(ly0 + r) * RL_P + lx0]) = u32x4_r{P[r][0], P[r][1], P[r][2], P[r][3]};
  __syncthreads();
  WS_STAMP(2);

  // ---- phase 3, jump.  Pointer jumping, P <- P(P), until P's target is a root -- WITHOUT rounds: every value a pixel can
  // read from the tile, old or freshly compressed by its owner, is a pointer to one of its ancestors
  // (flagged when that ancestor is a root), so threads neither wait for each other nor agree on
  // when to stop; a thread is done when its own 16 pointers are final.  One barrier after the loop
  // (the tile is reused for colours), none inside.
  for (uint32_t it = 0; live != 0 && it < max_rounds; ++it) {       // max_rounds: timing experiments only (WS_DEBUG_MAXIT)
    // (tried: all 16 reads issued up front on clamped cells, no per-pixel branch -- the extra LDS traffic
    // of the pixels that are done cost more than the serialised waits)
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if ((live >> (r * 4 + c)) & 1u) {
          const uint32_t g = sB[P[r][c]];        // live pointers carry no flag: the value is the cell index
          P[r][c] = g;
          sB[(ly0 + r) * RL_P + lx0 + c] = g;
          if (g & RL_FINAL) live &= ~(1u << (r * 4 + c));
        }
      }
    WS_STAMP_VALUE(6, it + 1);
  }
  if (!HALO_SEEDS) __syncthreads();
  WS_STAMP(3);
  if (TABLES) {      // ---- phase 4, colours
    // seed colours from the side tables; with W % 4 == 0 a patch row sits in one mask word
    uint32_t side_first[4] = {0u, 0u, 0u, 0u};      // HALO_SEEDS, vec: `first` of the 4 patch rows
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gyc = min(gy0 + r, H - 1);
      if (vec) {
        const size_t g = (size_t)gyc * W + min(gx0, W - 4);
        // (the asm pins the colour arithmetic here: computed early it holds 16 registers through the rounds)
        asm volatile("" : "+v"(tab_mask[r]), "+v"(tab_base[r]));
        const uint32_t mw = tab_mask[r], wb = tab_base[r], sh = (uint32_t)(g & 31u);
        // colour of the row's first seed; the seeds after it in the row count on from there (one table popcount per
        // row instead of one per pixel: the kernel is VALU-bound)
        const uint32_t first = wb + __popc(mw & ((1u << sh) - 1u)) + 1u;
        const uint32_t nib = (seedbits >> (r * 4)) & 15u;
        Lb[r][0] = nib & 1u ? first : 0u;
        Lb[r][1] = nib & 2u ? first + (nib & 1u) : 0u;
        Lb[r][2] = nib & 4u ? first + __popc(nib & 3u) : 0u;
        Lb[r][3] = nib & 8u ? first + __popc(nib & 7u) : 0u;
        if (HALO_SEEDS) side_first[r] = first;
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const size_t g = (size_t)gyc * W + min(gx0 + c, W - 1);
          const uint32_t col = word_base[g >> 5] + __popc(seed_mask[g >> 5] & ((1u << (g & 31u)) - 1u)) + 1u;
          Lb[r][c] = (seedbits >> (r * 4 + c)) & 1u ? col : 0u;
        }
      }
    }
    // The left and right halo columns' colours.  The list is strictly increasing, so colours are consecutive along a row:
    // `first` is the number of seeds before the patch row's first pixel g, plus one.  Left, (y, x0 - 1): if g - 1 is a seed it
    // is the last seed before g, colour first - 1.  Right, (y, x0 + 64): the seeds of the patch row x0 + 60 .. 63 come
    // first, colour first + popc(nibble).  Same row, hence the same slice of a stack and the same colour base.
    if (HALO_SEEDS && vec && (pc == 0 || pc == 15)) {
      uint32_t cand[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) cand[r] = pc == 0 ? side_first[r] - 1u : side_first[r] + __popc((seedbits >> (r * 4)) & 15u);
      *reinterpret_cast<u32x4_r *>(&sHaloColour[(pc == 0 ? 128 : 192) + pr * 4]) = u32x4_r{cand[0], cand[1], cand[2], cand[3]};
    }
  }
  if (HALO_SEEDS) __syncthreads();      // (phase 4 ahead of phase 3's closing barrier: it touches no LDS but sHaloColour)
  if (BLOCK && TABLES) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gy = gy0 + r;
      const bool halo_row = (gy == 0 && (halo_flags & 1)) || (gy == H - 1 && (halo_flags & 2));
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (halo_row && gx0 + c < W && K[r][c] != 0u && K[r][c] != KEY_INF) Lb[r][c] = REF_BIT | (uint32_t)((size_t)gy * W + gx0 + c);
    }
  }
  // ---- phase 5, store.  Every pointer is final and in registers: the tile now becomes COLOURS -- a pixel's own colour (a seed's, or
  // none), and in the halo ring a REFERENCE to the global pixel the cell stands for -- so that whatever a
  // pointer ends at, the answer is one unconditional LDS read of its target: no decode of the cell index, no
  // select chain, no branch (this phase was 39 instructions per pixel with them)
  {
    const int side = tid >> 6, t = tid & 63;
    const int hy = side == 0 ? y0 - 1 : (side == 1 ? y0 + TS : y0 + t);
    const int hx = side == 2 ? x0 - 1 : (side == 3 ? x0 + TS : x0 + t);
    const int hyc = min(max(hy, 0), H - 1), hxc = min(max(hx, 0), W - 1);
    // HALO_SEEDS, 16-byte path: a halo cell that is a SEED of the plane holds the seed's colour instead -- a third of the
    // leaving chains of a random field end there (8192^2 bench field: 34 %, tools/count_halo_seed_refs.py), read a colour
    // without REF_BIT and so drop out of refmask, the lists and the chase.  The cell still holds the halo pixel's stamp
    // (phases 2 and 3 rewrite patch cells only; outside the plane it is KEY_INF): stamp 0 means seed.  The colour costs no
    // load of its own for the left and right columns (phase 4) and two coalesced ones per top / bottom row (phase 1).
    // 8192^2 bench field, per launch: k_resolve_chase 37.1 -> 29.3 us (77 -> 55 MB fetched, 37 -> 27 MB written) and this
    // kernel 168.9 -> 160.5 us (profiles/halo_seeds_kernel_stats_*.csv, halo_seeds_pmc_hbm_bytes.json; the first form, with
    // two table words loaded per halo cell, the left and right columns' a cache line each, was chase 41 -> 27 us and this
    // kernel 170 -> 183 us and was dropped).
    if (HALO_SEEDS && vec) {
      const int cell = (hy - (y0 - 1)) * RL_P + (hx - (x0 - 1)) + (RL_X0 - 1);
      sB[cell] = sB[cell] == 0u ? sHaloColour[tid] : REF_BIT | (uint32_t)((size_t)hyc * W + hxc);
    } else {
      sB[(hy - (y0 - 1)) * RL_P + (hx - (x0 - 1)) + (RL_X0 - 1)] = REF_BIT | (uint32_t)((size_t)hyc * W + hxc);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
    *reinterpret_cast<u32x4_r *>(&sB[(ly0 + r) * RL_P + lx0]) = u32x4_r{Lb[r][0], Lb[r][1], Lb[r][2], Lb[r][3]};
  __syncthreads();

  uint32_t refmask = 0;                          // pixels whose chain leaves the tile
  uint32_t out[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) out[r][c] = sB[P[r][c] & (RL_HALO - 1u)];      // 16 independent reads, one wait
  const bool whole = x0 + TS <= W && y0 + TS <= H;      // workgroup uniform
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gy = gy0 + r;
    if (whole) {
#pragma unroll
      for (int c = 0; c < 4; ++c) refmask |= (out[r][c] >> 31) << (r * 4 + c);      // REF_BIT is the top bit
    } else {
#pragma unroll
      for (int c = 0; c < 4; ++c)
        refmask |= ((uint32_t)((out[r][c] & REF_BIT) != 0u) & (uint32_t)(gy < H) & (uint32_t)(gx0 + c < W)) << (r * 4 + c);
    }
    if (gy < H) {
      if (vec) {
        if (gx0 < W) *reinterpret_cast<u32x4_r *>(labels + (size_t)gy * W + gx0) = u32x4_r{out[r][0], out[r][1], out[r][2], out[r][3]};
      } else {
#pragma unroll
        for (int c = 0; c < 4; ++c)
          if (gx0 + c < W && (TABLES || (P[r][c] & (RL_HALO - 1u)) != (uint32_t)((ly0 + r) * RL_P + lx0 + c)))
            labels[(size_t)gy * W + gx0 + c] = out[r][c];
      }
    }
  }
  if (MERGE) {      // ---- phase 6, classify
    // min and max of (label - 1) over the patch: an uncoloured pixel (0) wraps to the top, a reference lies at or
    // above REF_BIT - 1; so max == ~0 says "a hole", min < REF_BIT - 1 is a colour that needs no chase
    __shared__ uint32_t sTileLo[NTHREADS / 64], sTileHi[NTHREADS / 64], sTileAny[NTHREADS / 64];
    const bool border_tile = x0 == 0 || y0 == 0 || x0 + TS >= W || y0 + TS >= H;      // uniform
    uint32_t lo = 0xFFFFFFFFu, hi = 0u;
    bool any_interior = !border_tile;
    if (!border_tile) {
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) { const uint32_t t = out[r][c] - 1u; lo = min(lo, t); hi = max(hi, t); }
    } else {
      // image-border pixels never flood (the flood step only visits 3x3 window centres, lib.rs:220-222; edge correction pads
      // with zeros, lib.rs:1340-1352, whose ring is then the border): only interior pixels decide "one lake";
      // a corner pixel touches no interior pixel, its colour never merges and must not stand for the tile
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const int gy = gy0 + r, gx = gx0 + c;
          const bool in_plane = gy < H && gx < W;
          const bool inter = gy >= 1 && gy < H - 1 && gx >= 1 && gx < W - 1;
          const bool corner = (gy == 0 || gy == H - 1) && (gx == 0 || gx == W - 1);
          const uint32_t t = out[r][c] - 1u;
          if (in_plane && !corner) lo = min(lo, t);
          if (inter) { hi = max(hi, t); any_interior = true; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
      lo = min(lo, (uint32_t)__shfl_xor(lo, o, 64));
      hi = max(hi, (uint32_t)__shfl_xor(hi, o, 64));
    }
    const bool wave_any = __ballot(any_interior) != 0ull;
    if (lane == 0) { sTileLo[wave] = lo; sTileHi[wave] = hi; sTileAny[wave] = wave_any ? 1u : 0u; }
    __syncthreads();
    if (tid == 0) {
      uint32_t l = sTileLo[0], h2 = sTileHi[0], a = sTileAny[0];
#pragma unroll
      for (int k = 1; k < NTHREADS / 64; ++k) { l = min(l, sTileLo[k]); h2 = max(h2, sTileHi[k]); a |= sTileAny[k]; }
      const bool one_lake = h2 != 0xFFFFFFFFu && a != 0u;
      tile_min[tile] = !one_lake ? 0u : (l < REF_BIT - 1u ? l + 1u : RL_TILE_UNDECIDED);
    }
  }
  WS_STAMP(4);
  // ---- phase 7, references.  Work list of the reference pixels for k_resolve_chase: every WAVE owns a fixed region of the list
  // (64 lanes x 16 pixels) and a count word -- no reservation atomic, no barrier, no cross-wave offsets
  // (a returning atomicAdd per workgroup kept all four waves waiting ~1.5 us)
  const uint32_t cnt = __popc(refmask);
  const uint32_t incl = wave_inclusive_sum(cnt);
  const size_t region = (size_t)blockIdx.x * (NTHREADS / 64) + wave;
  // A quarter or more of the wave's pixels references (a smooth map: all of them, in a tile without a seed): no list --
  // k_resolve_chase reads the wave's 64 x 16 pixels from the label plane itself, 16 bytes a lane and row, instead of 8
  // bytes of list per reference written here and read there, and stores whole rows instead of single words (at 8192^2 and
  // a correlation length of 64 px the lists were 1 GB of a transform's traffic: resolve 1.05 -> 0.44 ms).
  const bool all_refs = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63) >= REF_DENSE;      // wave uniform
  if (lane == 63) ref_count[region] = all_refs ? REF_ALL : incl;
  if (refmask && !all_refs) {      // (the list writes are 8 of this kernel's 165 us on the bench field)
    // (pixel, what it refers to): the chase starts at the target without reading the pixel's own label first
    uint2 *dst = reinterpret_cast<uint2 *>(ref_list) + region * REF_REGION + (incl - cnt);
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if ((refmask >> i) & 1u) *dst++ = make_uint2((uint32_t)((size_t)(gy0 + (i >> 2)) * W + gx0 + (i & 3)), out[i >> 2][i & 3] & ~REF_BIT);
  }
  WS_STAMP(5);
}

// A wave per CH_R consecutive list regions (grid-stride).  A reference always points to a pixel with a strictly
// smaller stamp, so chains end at a seed; a racing reader sees either the reference or what it
// resolves to.
// On the bench field a region holds ~20 references and nearly every chain is one hop long: the kernel is three dependent
// memory round trips (count, entry, target) per wave and nothing else, so a wave takes the counts of CH_R regions in one
// load, walks their entries as ONE flattened list, CH_U entries per lane in flight, and issues the first hop of all of
// them before it waits (one region at a time, four per wave one after the other: 48 us at 8192^2, 75 MB of traffic; this
// form 41 us, whatever CH_R and CH_U: reading the lists is 6 us of it, the scattered 4-byte loads of the first hop ~10-17 and
// the scattered 4-byte stores ~18-28 -- partial writes into lines k_resolve_local has just sent to HBM; profiles/r2_v7_chase_ab.log).
// With halo seeds' colours written by k_resolve_local a region of the bench field holds ~24 references for ~37 and this
// kernel is 29 us for 37; CH_R / CH_U looked at again with the shorter lists (profiles/halo_seeds_chase_pairs.txt): 4 / 4
// 27.5-29.1 us, 4 / 2 27.4, 8 / 4 31.7, 8 / 2 34.6, 2 / 4 34.8 -- 4 / 4 stays.
// (groups of 8 regions balance badly on smooth maps, where every pixel is a reference and a region holds 1024: 8192^2 at
// correlation 64 / 256 px 344 / 212 us against 301 / 144 with 4 and 269 / 259 for the old one-region walk; bench field 38 us either way)
__global__ __launch_bounds__(256) void k_resolve_chase(uint32_t *labels, const uint32_t *__restrict__ ref_count,
                                const uint32_t *__restrict__ ref_list, size_t nregions, size_t n,
                                const uint32_t *__restrict__ gate, const uint32_t *__restrict__ seed_err,
                                size_t follow_from, size_t follow_to, int H, int W, int tilesX, uint32_t ntiles, int halve,
                                ReadBack rb0, ReadBack rb1) {
  // The read-backs of a replayed transform (ResolveJob::read_back: the lookahead pass's convergence slot, the error words) ride
  // here instead of in a launch of their own behind this one: every such word is final before this kernel starts (the slot
  // by the last pass, the seed errors by k_seed_tables, the carry word by k_resolve_local; nothing below raises one).  Ahead
  // of both early returns: a closed gate is exactly when the host needs the slot.
  if (blockIdx.x == 0) {
    for (uint32_t i = threadIdx.x; i < rb0.count; i += blockDim.x) rb0.host[i] = rb0.src[i];
    for (uint32_t i = threadIdx.x; i < rb1.count; i += blockDim.x) rb1.host[i] = rb1.src[i];
  }
  // [follow_from, follow_to): the pixels a chain may be followed THROUGH -- the whole plane [0, n), or, for a row block
  // whose halo rows still hold references to themselves, the plane without those rows: a chain stops at a halo pixel.
  const int lane = threadIdx.x & 63;
  if (seed_err && (seed_err[0] | seed_err[2]) != 0u) return;      // invalid side tables: k_resolve_local wrote no lists (see there)
  if (gate && __builtin_amdgcn_ballot_w64(gate[lane * STRIPE_STRIDE] != 0u) != 0ull) return;      // see k_resolve_local
  const size_t wave0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((size_t)gridDim.x * blockDim.x) >> 6;
  const size_t ngroups = (nregions + CH_R - 1) / CH_R;
  const size_t span = follow_to - follow_from;
  for (size_t grp = wave0; grp < ngroups; grp += nwaves) {
    // (last region first: the labels k_resolve_local wrote last are the ones still in the memory-side cache -- 43 -> 38 us)
    const size_t r0 = (ngroups - 1 - grp) * CH_R;
    uint32_t cnt = 0;
    if (lane < CH_R && r0 + lane < nregions) cnt = ref_count[r0 + lane];
    const unsigned long long all_refs = __builtin_amdgcn_ballot_w64(cnt == REF_ALL);      // regions without a list (k_resolve_local)
    cnt = cnt == REF_ALL ? 0u : min(cnt, (uint32_t)REF_REGION);
    const uint32_t incl = wave_inclusive_sum(cnt);      // lanes >= CH_R: the total
    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    uint32_t ends[CH_R - 1];                             // uniform: where region i + 1 starts in the flattened list
#pragma unroll
    for (int i = 0; i < CH_R - 1; ++i) ends[i] = (uint32_t)__builtin_amdgcn_readlane((int)incl, i);
    // ---- the lists of the group
    for (uint32_t jb = 0; jb < tot; jb += 64 * CH_U) {
      uint2 e[CH_U];
      uint32_t v[CH_U];
      bool ok[CH_U];
#pragma unroll
      for (int u = 0; u < CH_U; ++u) {
        const uint32_t j = jb + u * 64 + lane;
        ok[u] = j < tot;
        uint32_t reg = 0, base = 0;
#pragma unroll
        for (int i = 0; i < CH_R - 1; ++i)
          if (j >= ends[i]) { reg = i + 1; base = ends[i]; }
        // (a lane past the end reads entry 0 of the group's first region: inside the list, ignored)
        e[u] = reinterpret_cast<const uint2 *>(ref_list)[(r0 + (ok[u] ? reg : 0u)) * REF_REGION + (ok[u] ? j - base : 0u)];
      }
      // A reference points at a pixel with a strictly smaller stamp, so a chain visits a pixel at most once: fewer than n
      // hops.  The range test and the hop bound are belt and braces: with invalid side tables (the only source of words
      // that are not colours or references of this plane) both resolve kernels have already left.
      // first hop of every entry: unconditional loads (pixel 0 for a lane with nothing to follow), one wait
      bool follow[CH_U];
      uint32_t first[CH_U];
#pragma unroll
      for (int u = 0; u < CH_U; ++u) {
        v[u] = e[u].y | REF_BIT;
        follow[u] = ok[u] && n != 0 && (size_t)e[u].y - follow_from < span;
        first[u] = __hip_atomic_load(labels + (follow[u] ? e[u].y : (uint32_t)follow_from), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < CH_U; ++u) {
        if (follow[u]) v[u] = follow_chain<false>(labels, first[u], follow_from, span, n);      // (lists: short chains, a hop or two)
      }
#pragma unroll
      for (int u = 0; u < CH_U; ++u)
        if (ok[u]) labels[e[u].x] = v[u];
    }
    // ---- the dense regions, those without a list: the wave of k_resolve_local that owned region r held the 4 x 4 patches (lane & 15,
    // 4 (r & 3) + lane / 16) of tile xcd_span_index(r / 4); a label that is no reference is left alone
    for (unsigned long long m = all_refs; m != 0ull; m &= m - 1ull) {
      const size_t region = r0 + (size_t)__builtin_ctzll(m);
      const uint32_t tile = xcd_span_index((uint32_t)(region / (NTHREADS / 64)), ntiles);
      const int gx0 = (int)(tile % (uint32_t)tilesX) * TS + (lane & 15) * 4;
      const int gy0 = (int)(tile / (uint32_t)tilesX) * TS + ((int)(region % (NTHREADS / 64)) * 4 + (lane >> 4)) * 4;
      const bool vec = (W & 3) == 0 && (reinterpret_cast<uintptr_t>(labels) & 15u) == 0;
      // (pixels outside the plane -- a tile at its right or lower edge -- read as label 0: no reference, never stored)
      uint32_t L[4][4];
      if (vec) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          u32x4_r q = u32x4_r{0u, 0u, 0u, 0u};
          if (gy0 + r < H && gx0 < W) q = *reinterpret_cast<const u32x4_r *>(labels + (size_t)(gy0 + r) * W + gx0);
          L[r][0] = q.x; L[r][1] = q.y; L[r][2] = q.z; L[r][3] = q.w;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c) L[r][c] = gy0 + r < H && gx0 + c < W ? labels[(size_t)(gy0 + r) * W + gx0 + c] : 0u;
      }
      // first hops: sixteen unconditional loads, one wait; neighbouring pixels mostly leave the tile by the same halo pixel
      uint32_t first[4][4];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const uint32_t t = L[r][c] & ~REF_BIT;
          const bool go = (L[r][c] & REF_BIT) && n != 0 && (size_t)t - follow_from < span;
          first[r][c] = __hip_atomic_load(labels + (go ? t : (uint32_t)follow_from), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
      // ... and the rest of a chain once per run of pixels that share it (the hop bound as above)
      uint32_t memo_from = 0u, memo_to = 0u;      // (0 is not a reference: never matches)
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const uint32_t t = L[r][c] & ~REF_BIT;
          if ((L[r][c] & REF_BIT) && n != 0 && (size_t)t - follow_from < span) {
            uint32_t v = first[r][c];
            if ((v & REF_BIT) && (size_t)(v & ~REF_BIT) - follow_from < span) {
              if (v == memo_from) v = memo_to;
              else {
                const uint32_t from = v;
                v = halve ? follow_chain<true>(labels, v, follow_from, span, n) : follow_chain<false>(labels, v, follow_from, span, n);
                memo_from = from; memo_to = v;
              }
            }
            L[r][c] = v;
          }
        }
      if (vec) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (gy0 + r < H && gx0 < W) *reinterpret_cast<u32x4_r *>(labels + (size_t)(gy0 + r) * W + gx0) = u32x4_r{L[r][0], L[r][1], L[r][2], L[r][3]};
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            if (gy0 + r < H && gx0 + c < W) labels[(size_t)(gy0 + r) * W + gx0 + c] = L[r][c];
      }
    }
  }
}

// words of scratch the two-launch resolve needs: a count and a REF_REGION-entry list per wave of k_resolve_local
size_t resolve_ref_capacity(int h, int w) {
  const size_t nregions = (size_t)tiles_of(w) * tiles_of(h) * (NTHREADS / 64);
  return nregions * (1 + 2 * REF_REGION);      // a count and REF_REGION (pixel, target) pairs per wave
}

static unsigned chase_grid(size_t nregions) { return (unsigned)std::min<size_t>(((nregions + CH_R - 1) / CH_R + 3) / 4, 4096); }

template <bool TABLES, bool MERGE, bool BLOCK>
static hipError_t launch_resolve_local(hipStream_t s, const ResolveJob &j, int halo_rows) {
  const int tx = tiles_of(j.w), ty = tiles_of(j.h);
  uint32_t *ref_count = j.ref_scratch, *ref_list = j.ref_scratch + (size_t)tx * ty * (NTHREADS / 64);
  k_resolve_local<TABLES, MERGE, BLOCK><<<tx * ty, NTHREADS, 0, s>>>(j.keys, j.labels, j.h, j.w, tx, ref_count, ref_list, j.max_rounds,
                                                                    TABLES ? j.seed_mask : nullptr, TABLES ? j.word_base : nullptr,
                                                                    MERGE ? j.tile_min : nullptr, j.gate, /* SH */ j.h, j.carry_flag,
                                                                    TABLES ? j.seed_err : nullptr, BLOCK && TABLES ? halo_rows : 0);
  return hipGetLastError();
}

// Which k_resolve_local runs.  ring = no seed tables and halo_flags & 4; halo rows = halo_flags & 3:
//
//   seed tables  ring  halo rows  tile_min | TABLES MERGE BLOCK
//   no           yes   any        any      |   -      -     x     the ring form: tile_min is ignored (and there are no tables)
//   yes          -     set        any      |   x      -     x     a row block: tile_min is ignored
//   yes          -     none       set      |   x      x     -
//   yes          -     none       no       |   x      -     -
//   no           no    any        set      |   -      x     -     (halo rows without tables: only the chase stops at them)
//   no           no    any        no       |   -      -     -
hipError_t resolve_two_launch(hipStream_t s, const ResolveJob &job) {
  const int tx = tiles_of(job.w), ty = tiles_of(job.h);
  const size_t n = (size_t)job.h * job.w;
  if (n == 0) return hipSuccess;
  const size_t nregions = (size_t)tx * ty * (NTHREADS / 64);
  // halo_flags 4 (a tile of a field cut in both directions, painted labels): the plane's border RING holds other ranks' pixels
  // with whatever label is known of them so far -- not flooded here (the BLOCK masks), roots like seeds; chains end there
  const bool tables = job.seed_mask != nullptr;
  const bool ring = !tables && (job.halo_flags & 4) != 0;
  const int halo_rows = job.halo_flags & 3;
  const bool block = ring || (tables && halo_rows != 0);
  const bool merge = !block && job.tile_min != nullptr;
  hipError_t e = hipErrorInvalidValue;
  switch ((tables ? 4 : 0) | (merge ? 2 : 0) | (block ? 1 : 0)) {      // (block excludes merge: six instantiations)
    case 0: e = launch_resolve_local<false, false, false>(s, job, halo_rows); break;
    case 1: e = launch_resolve_local<false, false, true>(s, job, halo_rows); break;
    case 2: e = launch_resolve_local<false, true, false>(s, job, halo_rows); break;
    case 4: e = launch_resolve_local<true, false, false>(s, job, halo_rows); break;
    case 5: e = launch_resolve_local<true, false, true>(s, job, halo_rows); break;
    case 6: e = launch_resolve_local<true, true, false>(s, job, halo_rows); break;
  }
  if (e != hipSuccess) return e;
  const size_t from = (halo_rows & 1) ? (size_t)job.w : 0, to = (halo_rows & 2) ? n - (size_t)job.w : n;
  k_resolve_chase<<<chase_grid(nregions), 256, 0, s>>>(job.labels, job.ref_scratch, job.ref_scratch + nregions, nregions, n, job.gate,
                                                       tables ? job.seed_err : nullptr, from, to, job.h, job.w, tx, (uint32_t)(tx * ty),
                                                       halo_rows == 0 && !ring ? 1 : 0, job.read_back[0], job.read_back[1]);
  return hipGetLastError();
}

// the chase alone, over the lists the last resolve_two_launch left in ref_scratch: every chain is followed to its end
// (a row block after ws_block_import_boundary has put the neighbours' colours into its halo rows)
hipError_t resolve_chase_again(hipStream_t s, uint32_t *labels, int h, int w, uint32_t *ref_scratch) {
  const size_t n = (size_t)h * w;
  if (n == 0) return hipSuccess;
  const size_t nregions = (size_t)tiles_of(w) * tiles_of(h) * (NTHREADS / 64);
  k_resolve_chase<<<chase_grid(nregions), 256, 0, s>>>(labels, ref_scratch, ref_scratch + nregions, nregions, n, nullptr, nullptr, 0, n, h, w, tiles_of(w), (uint32_t)(tiles_of(w) * tiles_of(h)), 0,
                                                       ReadBack(), ReadBack());
  return hipGetLastError();
}

}  // namespace wsk
