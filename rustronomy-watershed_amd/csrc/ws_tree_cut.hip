// ws_tree_cut.hip -- ws_tree_cut_device / ws_merge_tree_cut: the label planes and the lake lists of a merge
// tree pruned by lake size, number of leaves and level.  gfx950 kernels and their drivers; nothing here runs a flood or a union.
//
// A cut keeps node a iff a is alive or (area[a] >= min_area and n_leaves[a] >= min_leaves).  Pixel p with colour c = seg[p] and
// arrival level t goes to the first node on c's parent chain that is kept AND dies after max(t, merge_level).  Death levels,
// areas and leaves all grow strictly along `parent`, so both conditions are monotone up the chain and the two climbs commute:
// T[c] = the first kept node of c's chain depends on the cut alone (one table per distinct pair of thresholds), and a pixel
// walks on from T[seg[p]] while death <= max(t, merge_level).
//
// Nothing walks before k_cut_check has passed the records: parent < c bounds every walk and every index, and the host reads
// the verdict before the next launch.  A label above n_seeds is compared before it indexes anything.
//
// ws_tree_cut_stats_device / ws_merge_tree_stats_cut (section 4.4.1) add three thresholds on the lake catalogue of the same flood
// (ws_lake_cut): sum_w, w_max and depth = death_level - w_min.  The plane is DEFINED as table, then walk, so it is total whatever
// the catalogue holds; for the catalogue of the tree's own flood all five kept-quantities are monotone up the chain and the
// argument above stands.  Only the tables change: k_cut_keys packs what the keep test reads of a 72-byte record into 16 bytes a
// colour, and the table kernel gathers that next to the tree record; a call with a single such table reads the records themselves
// (cut_source).  Both entry points share one driver (cut_run).
//
// ws_tree_cut_catalogue_device / ws_merge_tree_cut_catalogue (section 4.4.2) measure the regions the cuts show: after the lists are
// compacted the counters hold every record's position (k_cut_compact<CUT_INDEX>), k_cut_measure walks again and folds every pixel
// into the accumulator entry of its region's record (the LakePart fold of ws_lake_part.hpp), and k_cut_measure_write turns the
// entries into ws_lake_stats records next to d_lakes, the cuts' hidden pixels behind them.  The same driver, with a CutMeasure.
//
// ws_tree_cut_catalogue_batch_device (section 4.4.3) is all of that for a cube of slices in one call: the records of every slice
// checked within their slice and copied with parents as indices into the whole array (k_cut_check_slices), the tables and the walk
// unchanged on that forest, a pixel's slice found per pixel (CutQuad), counters slice, then cut, then colour and ONE compaction
// (k_cut_compact_slices).  Its driver (cube_run) is what the cube forms of ws_batch.hip call per group (cut_cube_run).
#include "ws_ctx.hpp"
#include "ws_uf.hpp"
#include "ws_lake_part.hpp"
#include "ws_lists.hpp"

#include <type_traits>

namespace wsk {

constexpr int CUT_MAX = 32;            // cuts of one call
constexpr uint32_t CUT_STEPS = 256;    // a valid chain holds at most 255 hooks (death levels 0 .. 254 strictly increase)
// the flag words of a call
constexpr int CUT_F_TREE = 0;          // k_cut_check: a record that is no merge-tree record
constexpr int CUT_F_LABEL = 1;         // k_render_cut: a label above n_seeds
constexpr int CUT_F_STEPS = 2;         // a walk that hit CUT_STEPS (cannot happen on a checked tree)
constexpr int CUT_F_WORDS = 4;

// The cuts in the order the render takes them: by table, then by merge_level, so that a pixel's walk for one cut goes on from
// the node the previous cut of the same table left it on.  slot: the cut's place in the caller's list (its plane, its counters).
struct CutEntry {
  uint32_t table;
  uint8_t merge_level, show_level, slot, pad;
};
struct CutPlan {
  uint32_t n, n_tables;
  CutEntry e[CUT_MAX];
  uint32_t min_area[CUT_MAX], min_leaves[CUT_MAX], min_w_max[CUT_MAX], min_depth[CUT_MAX];      // per table
  u64c min_sum_w[CUT_MAX];
};
// What the keep test reads of colour c's catalogue record, as one 16-byte load: sum_w, w_max and the depth, which needs the tree
// record (death_level - w_min where the lake died above its smallest weight, else 0) and is therefore folded in once, here.
struct alignas(16) CutKey {
  u64c sum_w;
  uint32_t w_max, depth;
};
// how the table kernel tests the catalogue thresholds: not at all, from the packed keys, or from the records themselves
enum CutSource { CUT_TREE_ONLY = 0, CUT_KEYS = 1, CUT_RECORDS = 2 };

// ---- the records, checked ---------------------------------------------------------------------------------------------------------
// One lane, one record (16 bytes, as one load where the array is 16-byte aligned).  A merge-tree record is either alive with no
// parent, or dies at a level <= 254 into a SMALLER colour that dies strictly later.  The parent's record is read only once
// parent < c is known: every index stays below n_colours.
__global__ __launch_bounds__(256) void k_cut_check(const TreeRec *__restrict__ tree, size_t n_colours, bool aligned, uint32_t *flags) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_colours) return;
  TreeRec r;
  if (aligned) {
    const u32x4_m v = reinterpret_cast<const u32x4_m *>(tree)[c];
    r = TreeRec{v.x, v.y, v.z, v.w};
  } else {
    r = tree[c];
  }
  bool ok;
  if (r.death_level == TREE_ALIVE) ok = r.parent == 0u;
  else ok = r.death_level <= 254u && r.parent != 0u && r.parent < c && tree[r.parent].death_level > r.death_level;
  if (!ok) atomicOr(&flags[CUT_F_TREE], 1u);
}

// ---- the tables ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cut_depth(uint32_t death_level, uint32_t w_min) {
  return death_level != TREE_ALIVE && death_level > w_min ? death_level - w_min : 0u;
}

// One streaming pass over the catalogue: a lane reads the 16 bytes of its 72-byte record that the keep test needs (two 8-byte
// loads: the records are 8-byte aligned and no more) and the death level of its tree record, and stores one key.
__global__ __launch_bounds__(256) void k_cut_keys(const TreeRec *__restrict__ tree, const LakeRec *__restrict__ stats, size_t n_colours, CutKey *keys) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_colours) return;
  const u64c sum_w = stats[c].sum_w;
  const uint32_t w_min = stats[c].w_min, w_max = stats[c].w_max;
  reinterpret_cast<u32x4_m *>(keys)[c] = u32x4_m{(uint32_t)sum_w, (uint32_t)(sum_w >> 32), w_max, cut_depth(tree[c].death_level, w_min)};
}

// T_j[c] for every table j of the plan (blockIdx.y): up `parent` while the node is not kept.  The chain ends at an alive node,
// which is kept; at most 255 steps on a checked tree, and the cap holds whatever the records say.  SRC == CUT_KEYS: a table with a
// catalogue threshold (workgroup uniform) gathers the node's 16-byte key next to its 16-byte tree record, both loads in flight
// together; a table without one reads the tree alone, as CUT_TREE_ONLY does for every table.  CUT_RECORDS reads sum_w, w_min and
// w_max from the 72-byte record itself, two cache lines a step: the form of a call with ONE such table (cut_source).
template <int SRC>
__global__ __launch_bounds__(256) void k_cut_table(const TreeRec *__restrict__ tree, const CutKey *__restrict__ ckeys, const LakeRec *__restrict__ stats,
                                                   size_t n_colours, CutPlan plan, uint32_t *tables, uint32_t *flags) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_colours) return;
  const uint32_t j = blockIdx.y, min_area = plan.min_area[j], min_leaves = plan.min_leaves[j];
  const uint32_t min_w_max = SRC != CUT_TREE_ONLY ? plan.min_w_max[j] : 0u, min_depth = SRC != CUT_TREE_ONLY ? plan.min_depth[j] : 0u;
  const u64c min_sum_w = SRC != CUT_TREE_ONLY ? plan.min_sum_w[j] : 0ull;
  const bool catalogue = SRC != CUT_TREE_ONLY && (min_sum_w != 0ull || min_w_max != 0u || min_depth != 0u);
  uint32_t a = (uint32_t)c, steps = 0;
  for (;;) {
    const TreeRec r = tree[a];
    bool keep = r.area >= min_area && r.n_leaves >= min_leaves;
    if constexpr (SRC == CUT_KEYS) {
      if (catalogue) {
        const u32x4_m k = reinterpret_cast<const u32x4_m *>(ckeys)[a];
        keep = keep && ((u64c)k.y << 32 | k.x) >= min_sum_w && k.z >= min_w_max && k.w >= min_depth;
      }
    } else if constexpr (SRC == CUT_RECORDS) {
      if (catalogue) {
        const u64c sum_w = stats[a].sum_w;
        const uint32_t w_min = stats[a].w_min, w_max = stats[a].w_max;
        keep = keep && sum_w >= min_sum_w && w_max >= min_w_max && cut_depth(r.death_level, w_min) >= min_depth;
      }
    }
    if (r.death_level == TREE_ALIVE || keep) break;
    if (++steps > CUT_STEPS || r.parent >= a) { atomicOr(&flags[CUT_F_STEPS], 1u); a = 0u; break; }
    a = r.parent;
  }
  tables[(size_t)j * n_colours + c] = a;
}

// ---- the planes and the counters ----------------------------------------------------------------------------------------------------
// Counting.  A cut's counter of lake v is word slot * n_colours + v of the counters, and that index (below 2^32 - 1: the host
// checks) is the key of a workgroup's LDS table, as k_tree_own's: a workgroup takes a contiguous run of pixels, whose lakes are few,
// and touches memory once per (cut, lake) it met.  A key that finds no slot within CUT_PROBES adds to memory itself: exact either way.
constexpr int CUT_SLOTS = 2048, CUT_PROBES = 4;
constexpr uint32_t CUT_EMPTY = 0xFFFFFFFFu;

template <bool SLICES = false>      // (an instantiation of its own for the cube's kernels: the single-plane kernels keep their code)
__device__ __forceinline__ void cut_add(uint32_t *s_key, uint32_t *s_cnt, uint32_t *s_used, uint32_t *counts, uint32_t key, uint32_t k) {
  const uint32_t h0 = (key * 2654435761u) >> 21;      // 11 bits
  for (int j = 0; j < CUT_PROBES; ++j) {
    const uint32_t slot = (h0 + (uint32_t)j) & (CUT_SLOTS - 1);
    const uint32_t old = atomicCAS(&s_key[slot], CUT_EMPTY, key);
    if (old == CUT_EMPTY) atomicAdd(s_used, 1u);
    if (old == CUT_EMPTY || old == key) { atomicAdd(&s_cnt[slot], k); return; }
  }
  atomicAdd(&counts[key], k);
}

// One pixel slot of every lane (weight k: the pixels of the lane's quad that share the key).  The lanes that agree with the wave's
// first live lane add once -- a coarse cut sends whole waves to a handful of lakes, a low show_level to entry 0 -- the others for
// themselves.  Called by whole waves.
template <bool SLICES = false>
__device__ __forceinline__ void cut_count(uint32_t *s_key, uint32_t *s_cnt, uint32_t *s_used, uint32_t *counts, bool live, uint32_t key, uint32_t k,
                                          int lane) {
  const unsigned long long todo = __builtin_amdgcn_ballot_w64(live);
  if (todo == 0) return;      // wave uniform
  const int leader = (int)__builtin_ctzll(todo);
  const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
  const bool same = live && key == k0;
  if (__popcll(__builtin_amdgcn_ballot_w64(same)) > 1) {      // wave uniform
    const uint32_t total = wave_sum_u32(same ? k : 0u);
    if (lane == leader) cut_add<SLICES>(s_key, s_cnt, s_used, counts, k0, total);
    else if (live && !same) cut_add<SLICES>(s_key, s_cnt, s_used, counts, key, k);
  } else if (live) {
    cut_add<SLICES>(s_key, s_cnt, s_used, counts, key, k);
  }
}

// ---- a thread's four pixels: the loads, the guard, the table entry and the walks, as k_render_cut and k_cut_measure share them -----
// Stamps and colours of the quad at pixels 4 * q .. 4 * q + 3: 16-byte loads where vec_in (keys and labels 16-byte aligned) and the
// quad is whole, pixel by pixel otherwise, with the same result.
__device__ __forceinline__ void cut_load(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, size_t n, size_t q, bool vec_in,
                                         uint32_t (&arr)[4], uint32_t (&col)[4], bool (&in)[4]) {
  const size_t i0 = 4 * q;
  if (vec_in && i0 + 3 < n) {
    const u32x4_m k = reinterpret_cast<const u32x4_m *>(keys)[q], l = reinterpret_cast<const u32x4_m *>(labels)[q];
    arr[0] = k.x >> 24; arr[1] = k.y >> 24; arr[2] = k.z >> 24; arr[3] = k.w >> 24;
    col[0] = l.x; col[1] = l.y; col[2] = l.z; col[3] = l.w;
    in[0] = in[1] = in[2] = in[3] = true;
  } else {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      in[p] = i0 + p < n;
      arr[p] = in[p] ? keys[i0 + p] >> 24 : 0xFFu;
      col[p] = in[p] ? labels[i0 + p] : 0u;
    }
  }
}

// The walk of one quad through the cuts of a plan: a pixel keeps the node it stands on and that node's parent and death level in
// registers, so a step of the walk is ONE dependent load; the four walks of a thread run side by side (one after the other they
// wait for each other's gathers); a cut of the same table as the one before it walks on from where that one stopped (merge levels
// ascend within a table), and a new table starts from its own entry.
struct CutWalk {
  uint32_t arr[4], col[4];
  bool walks[4];      // coloured: the pixel has a chain to walk
  uint32_t a[4], up[4], d[4];      // the node, its parent, its death level
  uint32_t table;

  __device__ __forceinline__ void start(uint32_t n_seeds, uint32_t *flags) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (col[p] > n_seeds) {      // before it indexes anything
        atomicOr(&flags[CUT_F_LABEL], 1u);
        col[p] = 0u;
      }
      walks[p] = col[p] != 0u && arr[p] != 0xFFu;      // (0xFF: never coloured, above every show_level)
      a[p] = up[p] = 0u;
      d[p] = TREE_ALIVE;
    }
    table = 0xFFFFFFFFu;
  }

  // the lakes v[] the four pixels show under cut e
  __device__ __forceinline__ void cut(const TreeRec *__restrict__ tree, const uint32_t *__restrict__ tables, size_t n_colours, const CutEntry e,
                                      uint32_t *flags, uint32_t (&v)[4]) {
    if (e.table != table) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (walks[p]) a[p] = tables[(size_t)e.table * n_colours + col[p]];
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (walks[p]) { up[p] = tree[a[p]].parent; d[p] = tree[a[p]].death_level; }
      table = e.table;
    }
    bool shown[4];
    uint32_t until[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      shown[p] = walks[p] && arr[p] <= (uint32_t)e.show_level;
      until[p] = max(arr[p], (uint32_t)e.merge_level);
    }
    for (uint32_t hops = 0;; ++hops) {      // the four walks side by side
      bool go[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) go[p] = shown[p] && d[p] <= until[p];
      if (!(go[0] || go[1] || go[2] || go[3])) break;
      if (hops >= CUT_STEPS) { atomicOr(&flags[CUT_F_STEPS], 1u); break; }
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (go[p]) a[p] = up[p];      // (k_cut_check: below the node it leaves, so inside the records)
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (go[p]) { up[p] = tree[a[p]].parent; d[p] = tree[a[p]].death_level; }
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) v[p] = shown[p] ? a[p] : 0u;
  }
};

// A workgroup takes `steps` consecutive runs of 1024 pixels, a thread four consecutive pixels of each: their stamps and colours once
// (cut_load), then cut after cut in the plan's order (CutWalk), and every plane gets its four pixels as one 16-byte store where out
// and plane_stride allow it.  The last, short quad of a plane and planes off 16-byte alignment load and store pixel by pixel, with
// the same result.
// LISTS: the counters of every cut, through the workgroup's table; it is written out when a step leaves it more than half full
// and at the end.  Every trip count and barrier is the same for all threads of a workgroup.
template <bool LISTS>
__global__ __launch_bounds__(256) void k_render_cut(const TreeRec *__restrict__ tree, uint32_t n_seeds, const uint32_t *__restrict__ tables,
                                                    const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, size_t n, size_t steps,
                                                    CutPlan plan, uint32_t *out, size_t plane_stride, uint32_t *counts, uint32_t *flags) {
  __shared__ uint32_t s_key[LISTS ? CUT_SLOTS : 1], s_cnt[LISTS ? CUT_SLOTS : 1], s_used;
  const size_t n_colours = (size_t)n_seeds + 1;
  const int lane = threadIdx.x & 63;
  if constexpr (LISTS) {
    for (int j = threadIdx.x; j < CUT_SLOTS; j += 256) { s_key[j] = CUT_EMPTY; s_cnt[j] = 0; }
    if (threadIdx.x == 0) s_used = 0;
    __syncthreads();
  }
  uint32_t flushed_at = 0;      // slots taken, over the run, when the table was last written out
  const bool vec_in = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  const bool vec_out = out && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (plane_stride & 3u) == 0;
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t q = ((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x, i0 = 4 * q;
    const bool whole = i0 + 3 < n;
    CutWalk wk;
    bool in[4];
    cut_load(keys, labels, n, q, vec_in, wk.arr, wk.col, in);
    wk.start(n_seeds, flags);
    for (uint32_t j = 0; j < plan.n; ++j) {
      const CutEntry e = plan.e[j];
      uint32_t v[4];
      wk.cut(tree, tables, n_colours, e, flags, v);
      if (out) {
        uint32_t *plane = out + (size_t)e.slot * plane_stride;
        if (vec_out && whole) {
          reinterpret_cast<u32x4_m *>(plane)[q] = u32x4_m{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (in[p]) plane[i0 + p] = v[p];
        }
      }
      if constexpr (LISTS) {
        const uint32_t first = (uint32_t)((size_t)e.slot * n_colours);
        bool live[4];
        uint32_t k[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) { live[p] = in[p]; k[p] = 1u; }
#pragma unroll
        for (int p = 1; p < 4; ++p)      // a quad mostly lies in one lake: the lane adds once
#pragma unroll
          for (int r = 0; r < p; ++r)
            if (live[p] && live[r] && v[p] == v[r]) { k[r] += k[p]; live[p] = false; }
#pragma unroll
        for (int p = 0; p < 4; ++p) cut_count(s_key, s_cnt, &s_used, counts, live[p], first + v[p], k[p], lane);
      }
    }
    if constexpr (LISTS) {
      __syncthreads();
      const uint32_t used = s_used;      // (nobody inserts between the two barriers: workgroup uniform)
      const bool full = used - flushed_at > CUT_SLOTS / 2;
      if (full || st + 1 == steps)
        for (int j = threadIdx.x; j < CUT_SLOTS; j += 256)
          if (s_key[j] != CUT_EMPTY) {
            atomicAdd(&counts[s_key[j]], s_cnt[j]);
            s_key[j] = CUT_EMPTY;
            s_cnt[j] = 0;
          }
      if (full) flushed_at = used;
      __syncthreads();
    }
  }
}

// ---- the lists ----------------------------------------------------------------------------------------------------------------------
// The counters in colour order are the records in colour order: a workgroup takes CUT_CHUNK colours of one cut (blockIdx.y),
// counts those with pixels (CUT_COUNT: block_n), and, once the host has summed the blocks into bases, writes them behind its base
// (CUT_WRITE).  CUT_INDEX (ws_tree_cut_catalogue_device) writes them too, where there is a list, and then OVERWRITES counter
// (k, a) of every colour with pixels with the record's position in the lists, and counter 0 of cut k with total + k: the index the
// measuring kernel looks a pixel's lake up in.  A thread reads its four counters before it writes them, and nobody else reads them.
constexpr int CUT_PER_THREAD = 4;
constexpr int CUT_CHUNK = 256 * CUT_PER_THREAD;
enum CutCompact { CUT_COUNT = 0, CUT_WRITE = 1, CUT_INDEX = 2 };

template <int MODE>
__global__ __launch_bounds__(256) void k_cut_compact(const uint32_t *__restrict__ counts, size_t n_colours, uint32_t blocks_per_cut, uint32_t *block_n,
                                                     const u64c *__restrict__ block_base, ws_lake *lakes, uint32_t *index, uint32_t total) {
  __shared__ uint32_t s_n[256];
  const uint32_t k = blockIdx.y, t = threadIdx.x;
  const uint32_t *cnt = (MODE == CUT_INDEX ? index : counts) + (size_t)k * n_colours;      // (CUT_INDEX: the counters, read and written through ONE pointer)
  const size_t c0 = (size_t)blockIdx.x * CUT_CHUNK + (size_t)t * CUT_PER_THREAD;
  uint32_t area[CUT_PER_THREAD], mine = 0;
#pragma unroll
  for (int j = 0; j < CUT_PER_THREAD; ++j) {
    const size_t c = c0 + j;
    area[j] = c != 0 && c < n_colours ? cnt[c] : 0u;      // (entry 0: the hidden pixels, no record)
    mine += area[j] != 0u;
  }
  s_n[t] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t v = t >= (uint32_t)o ? s_n[t - o] : 0u;
    __syncthreads();
    s_n[t] += v;
    __syncthreads();
  }
  const size_t b = (size_t)k * blocks_per_cut + blockIdx.x;
  if constexpr (MODE == CUT_COUNT) {
    if (t == 255) block_n[b] = s_n[255];
    if (t == 0 && blockIdx.x == 0) block_n[(size_t)gridDim.y * blocks_per_cut + k] = cnt[0];      // behind the blocks: the cut's hidden pixels
  } else {
    u64c at = block_base[b] + (s_n[t] - mine);
#pragma unroll
    for (int j = 0; j < CUT_PER_THREAD; ++j)
      if (area[j] != 0u) {
        if (MODE == CUT_WRITE || lakes) lakes[at] = ws_lake{(uint64_t)(c0 + j), (uint64_t)area[j]};
        if constexpr (MODE == CUT_INDEX) index[(size_t)k * n_colours + c0 + j] = (uint32_t)at;
        ++at;
      }
    if constexpr (MODE == CUT_INDEX)
      if (c0 == 0) index[(size_t)k * n_colours] = total + k;
  }
}

// ---- the regions measured (ws_tree_cut_catalogue_device) ---------------------------------------------------
// The fold of k_lake_own over the REGIONS of every cut: pixel p of cut k goes to accumulator entry index[k * n_colours + out_k(p)]
// -- the position of the region's record in the lists, total + k for the hidden pixels -- so the accumulators are sized by records
// (n_rec = total + n_cuts entries of LAKE_ACC_BYTES), not by cuts x colours.  The loads, the guard, the table entry and the walks
// are k_render_cut's (cut_load, CutWalk): the kernel walks again and reads no plane, so it does not need one.  A pixel's weight,
// row and column are taken once a step; per cut a lane joins the pixels of its quad that agree, a wave joins the lanes that agree
// with its first live lane, the rest goes to the workgroup's LAKE_SLOTS-entry table keyed by accumulator entry (lake_add:
// LAKE_PROBES, then memory itself), and the table is written out when a cut of a step leaves it more than half full and at the
// end (lake_flush; k_lake_own looks once a step).  index == nullptr (no record wanted: the hidden pixels alone): a hidden pixel of cut k goes to
// entry k and the others sit out.  n_seeds == 0: every pixel is hidden, no label is looked at.  Every trip count and barrier is the
// same for all threads of a workgroup.
template <typename T>
__global__ __launch_bounds__(256) void k_cut_measure(const TreeRec *__restrict__ tree, uint32_t n_seeds, const uint32_t *__restrict__ tables,
                                                     const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, size_t n, size_t steps,
                                                     CutPlan plan, const uint32_t *__restrict__ index, LakeWeights wt, uint32_t W, u64c *sum,
                                                     uint32_t *box, size_t n_rec, uint32_t *flags) {
  __shared__ u64c s_sum[6 * LAKE_SLOTS];
  __shared__ uint32_t s_box[5 * LAKE_SLOTS], s_key[LAKE_SLOTS], s_used;
  for (int j = threadIdx.x; j < LAKE_SLOTS; j += 256) {
    s_key[j] = LAKE_EMPTY;
    lake_store(s_sum, s_box, LAKE_SLOTS, j, lake_none());
  }
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  const size_t n_colours = (size_t)n_seeds + 1;
  const int lane = threadIdx.x & 63;
  const bool vec_in = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  uint32_t flushed_at = 0;      // slots taken, over the run, when the table was last written out
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t q = ((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x, i0 = 4 * q;
    CutWalk wk;
    bool in[4];
    cut_load(keys, labels, n, q, vec_in, wk.arr, wk.col, in);
    if (n_seeds == 0u) wk.col[0] = wk.col[1] = wk.col[2] = wk.col[3] = 0u;
    wk.start(n_seeds, flags);
    uint32_t wv[4], yy[4], xx[4];      // the four pixels' weights, rows and columns
    {
      uint32_t y = i0 < n ? (uint32_t)i0 / W : 0u, x = i0 < n ? (uint32_t)i0 % W : 0u;      // (n < 2^32)
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        wv[p] = in[p] ? lake_weight<T>(wt, y, x) : 0u;
        yy[p] = y; xx[p] = x;
        if (++x == W) { x = 0; ++y; }
      }
    }
    for (uint32_t j = 0; j < plan.n; ++j) {
      const CutEntry e = plan.e[j];
      uint32_t v[4];
      wk.cut(tree, tables, n_colours, e, flags, v);
      bool live[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) live[p] = in[p] && (index != nullptr || v[p] == 0u);
#pragma unroll
      for (int p = 0; p < 4; ++p) {      // one part at a time: the first pixel of a lake takes the later ones of its quad (a quad mostly lies in one lake)
        LakePart part = lake_pixel(wv[p], yy[p], xx[p], (uint32_t)i0 + (uint32_t)p);
#pragma unroll
        for (int r = p + 1; r < 4; ++r)
          if (live[p] && live[r] && v[r] == v[p]) {
            lake_join(part, lake_pixel(wv[r], yy[r], xx[r], (uint32_t)i0 + (uint32_t)r));
            live[r] = false;
          }
        const unsigned long long todo = __builtin_amdgcn_ballot_w64(live[p]);
        if (todo == 0) continue;      // wave uniform
        const uint32_t at = !live[p] ? 0u : index ? index[(size_t)e.slot * n_colours + v[p]] : (uint32_t)e.slot;      // ONE look-up a lake and lane
        const int leader = (int)__builtin_ctzll(todo);
        const uint32_t at0 = (uint32_t)__builtin_amdgcn_readlane((int)at, leader);
        const bool same = live[p] && at == at0;
        if (__popcll(__builtin_amdgcn_ballot_w64(same)) > 1) {      // wave uniform
          const LakePart total = lake_wave_total(same ? part : lake_none());
          if (lane == leader) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_rec, at0, total);
          else if (live[p] && !same) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_rec, at, part);
        } else if (live[p]) {
          lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_rec, at, part);
        }
      }
      // after every CUT, not every step: the entries of one cut are of no use to the next (its regions have entries of their own),
      // so the table fills by the regions of a run times the cuts, and a table that the cuts of one step have filled sends the
      // next step's newcomers to memory field by field (measured: DESIGN.md section 4.4.2)
      __syncthreads();
      const uint32_t used = s_used;      // (nobody inserts between the two barriers: workgroup uniform)
      const bool full = used - flushed_at > LAKE_SLOTS / 2;
      if (full || (st + 1 == steps && j + 1 == plan.n)) lake_flush(s_key, s_sum, s_box, sum, box, n_rec);
      if (full) flushed_at = used;
      __syncthreads();
    }
  }
}

// The accumulator entries as records: entry i < total is the record of d_lakes[i], entry total + k the hidden pixels of cut k, which
// go to a buffer of their own that the host reads.  An entry nobody added to is the identity of the fold, and so is its record.
__global__ __launch_bounds__(256) void k_cut_measure_write(const u64c *__restrict__ sum, const uint32_t *__restrict__ box, size_t n_rec, size_t total,
                                                           LakeRec *region, LakeRec *hidden) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_rec) return;
  const LakePart a = lake_load(sum, box, n_rec, i);
  const LakeRec r{a.w, a.wr, a.wc, a.r, a.c, a.r_min, a.r_max, a.c_min, a.c_max, a.w_min, (uint32_t)(a.peak >> 32), 0xFFFFFFFFu - (uint32_t)a.peak, 0u};
  if (i < total) region[i] = r;
  else hidden[i - total] = r;
}

// ---- a cube of slices (ws_tree_cut_catalogue_batch_device) -------------------------------------------------
// The records of n_slices trees lie one behind the other: slice k owns records rb[k] .. rb[k + 1] (rb strictly increases: every
// slice has its record 0), its pixels are plane * k .. plane * (k + 1) of the stamps and the labels.  k_cut_check_slices checks every
// record WITHIN its slice and writes a copy whose parents are indices into the whole array (the forest), so the table kernels and
// CutWalk run on it unchanged; a pixel enters at rb[k] + colour and shows a - rb[k].  The counters lie slice, then cut, then colour
// -- counter n_cuts * rb[k] + slot * (n_k + 1) + v -- so that ONE compaction in index order writes the caller's layout.
struct CutSlices {
  const uint32_t *rb;      // n_slices + 1 entries, device
  uint32_t n_slices, plane, n_cuts;
};

// the slice that owns entry f of an array in which slice k's entries begin at mul * rb[k]: the same trip count for every thread
__device__ __forceinline__ uint32_t cut_slice_of(const CutSlices &sl, uint32_t mul, size_t f) {
  uint32_t lo = 0;
  for (uint32_t len = sl.n_slices; len > 1;) {
    const uint32_t half = len >> 1;
    if ((size_t)mul * sl.rb[lo + half] <= f) lo += half;
    len -= half;
  }
  return lo;
}

// One lane, one record, as k_cut_check: record c of slice k is alive with no parent, or dies at a level <= 254 into a smaller colour
// OF THE SAME SLICE that dies strictly later.  The one record of a slice without seeds is not looked at (the single call reads no
// tree then).  forest[i]: the record with its parent as an index into the whole array, 16 bytes as one store.
__global__ __launch_bounds__(256) void k_cut_check_slices(const TreeRec *__restrict__ tree, size_t n_rec, CutSlices sl, bool aligned, TreeRec *forest,
                                                          uint32_t *flags) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const uint32_t k = cut_slice_of(sl, 1u, i < n_rec ? i : n_rec - 1);
  if (i >= n_rec) return;
  const uint32_t base = sl.rb[k], c = (uint32_t)i - base, n_k = sl.rb[k + 1] - base - 1u;
  TreeRec r;
  if (aligned) {
    const u32x4_m v = reinterpret_cast<const u32x4_m *>(tree)[i];
    r = TreeRec{v.x, v.y, v.z, v.w};
  } else {
    r = tree[i];
  }
  bool ok = true, dead = false;
  if (n_k != 0u) {
    if (r.death_level == TREE_ALIVE) ok = r.parent == 0u;
    else ok = dead = r.death_level <= 254u && r.parent != 0u && r.parent < c && tree[(size_t)base + r.parent].death_level > r.death_level;
  }
  if (!ok) atomicOr(&flags[CUT_F_TREE], 1u);
  reinterpret_cast<u32x4_m *>(forest)[i] = dead ? u32x4_m{base + r.parent, r.death_level, r.area, r.n_leaves} : u32x4_m{0u, TREE_ALIVE, r.area, r.n_leaves};
}

// The slices of a thread's four pixels i0 .. i0 + 3: slice, pixel within the slice, first record and seed count.  A quad lies in one
// slice where plane % 4 == 0; otherwise it may straddle two or more, so every pixel has its own.
struct CutQuad {
  uint32_t k[4], r[4], base[4], ns[4];
  __device__ __forceinline__ void locate(const CutSlices &sl, size_t i0, size_t n) {
    uint32_t kk = i0 < n ? (uint32_t)i0 / sl.plane : 0u, rr = i0 < n ? (uint32_t)i0 % sl.plane : 0u;      // (n < 2^32)
    uint32_t b = sl.rb[kk], e = sl.rb[kk + 1];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      k[p] = kk; r[p] = rr; base[p] = b; ns[p] = e - b - 1u;
      if (++rr == sl.plane && kk + 1u < sl.n_slices) { rr = 0u; ++kk; b = e; e = sl.rb[kk + 1]; }
    }
  }
  // the counter of lake v (0: hidden) of the pixel's slice under the cut at `slot`
  __device__ __forceinline__ uint32_t counter(const CutSlices &sl, int p, uint32_t slot, uint32_t v) const {
    return sl.n_cuts * base[p] + slot * (ns[p] + 1u) + v;
  }
};

// CutWalk::start for the pixels of a cube: the bound of a label is its OWN slice's seed count -- a label above it may be a valid
// record of the next slice -- compared before it indexes anything; a slice without seeds shows nothing and its labels are not
// looked at.  Afterwards col[] is the pixel's record in the forest.
__device__ __forceinline__ void cut_start_slices(CutWalk &wk, const CutQuad &qd, uint32_t *flags) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (qd.ns[p] == 0u) {
      wk.col[p] = 0u;
    } else if (wk.col[p] > qd.ns[p]) {
      atomicOr(&flags[CUT_F_LABEL], 1u);
      wk.col[p] = 0u;
    }
    wk.walks[p] = wk.col[p] != 0u && wk.arr[p] != 0xFFu;
    if (wk.walks[p]) wk.col[p] += qd.base[p];
    wk.a[p] = wk.up[p] = 0u;
    wk.d[p] = TREE_ALIVE;
  }
  wk.table = 0xFFFFFFFFu;
}

// k_render_cut over the pixels of every slice: the loads, the walks and the workgroup's counting table are its own; plane (k, slot) is
// at out + (k * n_cuts + slot) * plane_stride, 16-byte stores where out, plane_stride AND plane allow it (quads then lie in one slice).
template <bool LISTS>
__global__ __launch_bounds__(256) void k_render_cut_slices(const TreeRec *__restrict__ forest, size_t n_rec, CutSlices sl, const uint32_t *__restrict__ tables,
                                                           const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, size_t n, size_t steps,
                                                           CutPlan plan, uint32_t *out, size_t plane_stride, uint32_t *counts, uint32_t *flags) {
  __shared__ uint32_t s_key[LISTS ? CUT_SLOTS : 1], s_cnt[LISTS ? CUT_SLOTS : 1], s_used;
  const int lane = threadIdx.x & 63;
  if constexpr (LISTS) {
    for (int j = threadIdx.x; j < CUT_SLOTS; j += 256) { s_key[j] = CUT_EMPTY; s_cnt[j] = 0; }
    if (threadIdx.x == 0) s_used = 0;
    __syncthreads();
  }
  uint32_t flushed_at = 0;
  const bool vec_in = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  const bool vec_out = out && (reinterpret_cast<uintptr_t>(out) & 15u) == 0 && (plane_stride & 3u) == 0 && (sl.plane & 3u) == 0;
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t q = ((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x, i0 = 4 * q;
    const bool whole = i0 + 3 < n;
    CutWalk wk;
    CutQuad qd;
    bool in[4];
    cut_load(keys, labels, n, q, vec_in, wk.arr, wk.col, in);
    qd.locate(sl, i0, n);
    cut_start_slices(wk, qd, flags);
    for (uint32_t j = 0; j < plan.n; ++j) {
      const CutEntry e = plan.e[j];
      uint32_t v[4];
      wk.cut(forest, tables, n_rec, e, flags, v);
#pragma unroll
      for (int p = 0; p < 4; ++p) v[p] = v[p] ? v[p] - qd.base[p] : 0u;      // (a shown node is never a slice's record 0)
      if (out) {
        if (vec_out && whole) {
          uint32_t *plane = out + ((size_t)qd.k[0] * sl.n_cuts + e.slot) * plane_stride;
          reinterpret_cast<u32x4_m *>(plane)[qd.r[0] >> 2] = u32x4_m{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
          for (int p = 0; p < 4; ++p)
            if (in[p]) out[((size_t)qd.k[p] * sl.n_cuts + e.slot) * plane_stride + qd.r[p]] = v[p];
        }
      }
      if constexpr (LISTS) {
        bool live[4];
        uint32_t key[4], k[4];
#pragma unroll
        for (int p = 0; p < 4; ++p) { live[p] = in[p]; k[p] = 1u; key[p] = qd.counter(sl, p, e.slot, v[p]); }
#pragma unroll
        for (int p = 1; p < 4; ++p)
#pragma unroll
          for (int r = 0; r < p; ++r)
            if (live[p] && live[r] && key[p] == key[r]) { k[r] += k[p]; live[p] = false; }
#pragma unroll
        for (int p = 0; p < 4; ++p) cut_count<true>(s_key, s_cnt, &s_used, counts, live[p], key[p], k[p], lane);
      }
    }
    if constexpr (LISTS) {
      __syncthreads();
      const uint32_t used = s_used;      // (nobody inserts between the two barriers: workgroup uniform)
      const bool full = used - flushed_at > CUT_SLOTS / 2;
      if (full || st + 1 == steps)
        for (int j = threadIdx.x; j < CUT_SLOTS; j += 256)
          if (s_key[j] != CUT_EMPTY) {
            atomicAdd(&counts[s_key[j]], s_cnt[j]);
            s_key[j] = CUT_EMPTY;
            s_cnt[j] = 0;
          }
      if (full) flushed_at = used;
      __syncthreads();
    }
  }
}

// k_cut_compact over the counters of the whole cube in index order, CUT_CHUNK of them a workgroup: a thread finds the slice, the cut
// and the colour of its first counter by one search and steps on from there (no segment is empty: a slice has its record 0).  Entry
// 0 of a (slice, cut) segment is its hidden counter and has no record; it sits exactly where that list begins, so the thread that
// holds it writes seg_first[k * n_cuts + slot] and seg_hidden[...] in the writing pass, and CUT_INDEX leaves total + k * n_cuts +
// slot there: the accumulator entry of that cut's hidden pixels.
template <int MODE>
__global__ __launch_bounds__(256) void k_cut_compact_slices(const uint32_t *__restrict__ counts, size_t n_counters, CutSlices sl, uint32_t *block_n,
                                                            const u64c *__restrict__ block_base, ws_lake *lakes, uint32_t *index, uint32_t total,
                                                            u64c *seg_first, u64c *seg_hidden) {
  __shared__ uint32_t s_n[256];
  const uint32_t t = threadIdx.x;
  const uint32_t *cnt = MODE == CUT_INDEX ? index : counts;      // (CUT_INDEX: the counters, read and written through ONE pointer)
  const size_t f0 = (size_t)blockIdx.x * CUT_CHUNK + (size_t)t * CUT_PER_THREAD;
  uint32_t k = cut_slice_of(sl, sl.n_cuts, f0 < n_counters ? f0 : n_counters - 1);
  uint32_t per = sl.rb[k + 1] - sl.rb[k];      // counters of a cut in this slice
  const uint32_t rel = (uint32_t)((f0 < n_counters ? f0 : n_counters - 1) - (size_t)sl.n_cuts * sl.rb[k]);
  uint32_t slot = rel / per, v = rel % per;
  uint32_t area[CUT_PER_THREAD], colour[CUT_PER_THREAD], seg[CUT_PER_THREAD], mine = 0;
  bool head[CUT_PER_THREAD];
#pragma unroll
  for (int j = 0; j < CUT_PER_THREAD; ++j) {
    const bool valid = f0 + j < n_counters;
    const uint32_t n = valid ? cnt[f0 + j] : 0u;
    head[j] = valid && v == 0u;
    colour[j] = v;
    seg[j] = k * sl.n_cuts + slot;
    area[j] = n;
    mine += !head[j] && n != 0u;
    if (++v == per) {
      v = 0u;
      if (++slot == sl.n_cuts) {
        slot = 0u;
        if (++k < sl.n_slices) per = sl.rb[k + 1] - sl.rb[k];
      }
    }
  }
  s_n[t] = mine;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const uint32_t x = t >= (uint32_t)o ? s_n[t - o] : 0u;
    __syncthreads();
    s_n[t] += x;
    __syncthreads();
  }
  if constexpr (MODE == CUT_COUNT) {
    if (t == 255) block_n[blockIdx.x] = s_n[255];
  } else {
    u64c at = block_base[blockIdx.x] + (s_n[t] - mine);
#pragma unroll
    for (int j = 0; j < CUT_PER_THREAD; ++j) {
      if (head[j]) {
        seg_first[seg[j]] = at;
        seg_hidden[seg[j]] = area[j];
        if constexpr (MODE == CUT_INDEX) index[f0 + j] = total + seg[j];
      } else if (area[j] != 0u) {
        if (MODE == CUT_WRITE || lakes) lakes[at] = ws_lake{(uint64_t)colour[j], (uint64_t)area[j]};
        if constexpr (MODE == CUT_INDEX) index[f0 + j] = (uint32_t)at;
        ++at;
      }
    }
  }
}

// k_cut_measure over the pixels of every slice: rows, columns and peak_pixel are those of the pixel's own slice, its weight that of
// the slice's weight plane (lake_weight_of_slice), its accumulator entry index[its counter]; index == nullptr (the hidden pixels
// alone): entry k * n_cuts + slot.  Every trip count and barrier is the same for all threads of a workgroup.
template <typename T>
__global__ __launch_bounds__(256) void k_cut_measure_slices(const TreeRec *__restrict__ forest, size_t n_colours, CutSlices sl, const uint32_t *__restrict__ tables,
                                                            const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels, size_t n, size_t steps,
                                                            CutPlan plan, const uint32_t *__restrict__ index, LakeWeights wt, uint32_t W, u64c *sum,
                                                            uint32_t *box, size_t n_rec, uint32_t *flags) {
  __shared__ u64c s_sum[6 * LAKE_SLOTS];
  __shared__ uint32_t s_box[5 * LAKE_SLOTS], s_key[LAKE_SLOTS], s_used;
  for (int j = threadIdx.x; j < LAKE_SLOTS; j += 256) {
    s_key[j] = LAKE_EMPTY;
    lake_store(s_sum, s_box, LAKE_SLOTS, j, lake_none());
  }
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool vec_in = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  uint32_t flushed_at = 0;
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t q = ((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x, i0 = 4 * q;
    CutWalk wk;
    CutQuad qd;
    bool in[4];
    cut_load(keys, labels, n, q, vec_in, wk.arr, wk.col, in);
    qd.locate(sl, i0, n);
    cut_start_slices(wk, qd, flags);
    uint32_t wv[4], yy[4], xx[4];      // the four pixels' weights, rows and columns within their slices
    {
      uint32_t y = qd.r[0] / W, x = qd.r[0] % W;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (p && qd.r[p] == 0u) y = x = 0u;      // the next slice begins
        wv[p] = in[p] ? lake_weight_of_slice<T>(wt, qd.k[p], y, x) : 0u;
        yy[p] = y; xx[p] = x;
        if (++x == W) { x = 0; ++y; }
      }
    }
    for (uint32_t j = 0; j < plan.n; ++j) {
      const CutEntry e = plan.e[j];
      uint32_t v[4], key[4];
      wk.cut(forest, tables, n_colours, e, flags, v);
      bool live[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        v[p] = v[p] ? v[p] - qd.base[p] : 0u;
        live[p] = in[p] && (index != nullptr || v[p] == 0u);
        key[p] = index ? qd.counter(sl, p, e.slot, v[p]) : qd.k[p] * sl.n_cuts + e.slot;
      }
#pragma unroll
      for (int p = 0; p < 4; ++p) {      // one part at a time, as k_cut_measure
        LakePart part = lake_pixel(wv[p], yy[p], xx[p], qd.r[p]);
#pragma unroll
        for (int r = p + 1; r < 4; ++r)
          if (live[p] && live[r] && key[r] == key[p]) {
            lake_join(part, lake_pixel(wv[r], yy[r], xx[r], qd.r[r]));
            live[r] = false;
          }
        const unsigned long long todo = __builtin_amdgcn_ballot_w64(live[p]);
        if (todo == 0) continue;      // wave uniform
        const uint32_t at = !live[p] ? 0u : index ? index[key[p]] : key[p];      // ONE look-up a lake and lane
        const int leader = (int)__builtin_ctzll(todo);
        const uint32_t at0 = (uint32_t)__builtin_amdgcn_readlane((int)at, leader);
        const bool same = live[p] && at == at0;
        if (__popcll(__builtin_amdgcn_ballot_w64(same)) > 1) {      // wave uniform
          const LakePart total = lake_wave_total(same ? part : lake_none());
          if (lane == leader) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_rec, at0, total);
          else if (live[p] && !same) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_rec, at, part);
        } else if (live[p]) {
          lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_rec, at, part);
        }
      }
      __syncthreads();
      const uint32_t used = s_used;      // (nobody inserts between the two barriers: workgroup uniform)
      const bool full = used - flushed_at > LAKE_SLOTS / 2;
      if (full || (st + 1 == steps && j + 1 == plan.n)) lake_flush(s_key, s_sum, s_box, sum, box, n_rec);
      if (full) flushed_at = used;
      __syncthreads();
    }
  }
}

}  // namespace wsk

namespace {

using namespace wsapi;

static_assert(sizeof(ws_tree_cut) == 12, "ws_tree_cut is part of the ABI");
static_assert(sizeof(ws_lake_cut) == 32, "ws_lake_cut is part of the ABI");

// The cuts of a call as the driver takes them -- a ws_tree_cut is the ws_lake_cut without catalogue thresholds -- with what the
// entry points check of them before anything runs: `refused` is the reason, reported where the checks of a call have always stood.
struct Cuts {
  ws_lake_cut v[CUT_MAX];
  size_t n = 0;
  const char *refused = nullptr;
  bool catalogue = false;      // some cut has a threshold on sum_w, w_max or depth
};

template <class C>
Cuts take_cuts(const C *cuts, size_t n_cuts) {
  Cuts cs;
  cs.n = n_cuts;
  if (n_cuts > (size_t)CUT_MAX) { cs.refused = "more than 32 cuts"; return cs; }
  if (n_cuts && !cuts) { cs.refused = "null pointer"; return cs; }
  for (size_t k = 0; k < n_cuts; ++k) {
    const C &in = cuts[k];
    ws_lake_cut &o = cs.v[k];
    o = ws_lake_cut{};
    o.min_area = in.min_area; o.min_leaves = in.min_leaves; o.show_level = in.show_level; o.merge_level = in.merge_level;
    if constexpr (std::is_same_v<C, ws_lake_cut>) { o.min_sum_w = in.min_sum_w; o.min_w_max = in.min_w_max; o.min_depth = in.min_depth; }
    if (in.show_level > 254 || in.merge_level > 254) { cs.refused = "a cut's level is above 254"; return cs; }
    for (uint8_t r : in.reserved)
      if (r) { cs.refused = "a cut's reserved bytes must be zero"; return cs; }
    cs.catalogue = cs.catalogue || o.min_sum_w || o.min_w_max || o.min_depth;
  }
  return cs;
}

int check_cuts(ws_ctx *c, const Cuts &cs) { return cs.refused ? fail(c, WS_ERR_BAD_ARG, cs.refused) : WS_OK; }

// one table per distinct five thresholds; the entries by table, then merge level (stable: repeats keep their order)
CutPlan make_plan(const Cuts &cs) {
  CutPlan p{};
  p.n = (uint32_t)cs.n;
  for (size_t k = 0; k < cs.n; ++k) {
    const ws_lake_cut &cut = cs.v[k];
    uint32_t j = 0;
    while (j < p.n_tables && !(p.min_area[j] == cut.min_area && p.min_leaves[j] == cut.min_leaves && p.min_sum_w[j] == cut.min_sum_w &&
                               p.min_w_max[j] == cut.min_w_max && p.min_depth[j] == cut.min_depth))
      ++j;
    if (j == p.n_tables) {
      p.min_area[j] = cut.min_area;
      p.min_leaves[j] = cut.min_leaves;
      p.min_sum_w[j] = cut.min_sum_w;
      p.min_w_max[j] = cut.min_w_max;
      p.min_depth[j] = cut.min_depth;
      ++p.n_tables;
    }
    p.e[k] = CutEntry{j, cut.merge_level, cut.show_level, (uint8_t)k, 0};
  }
  std::stable_sort(p.e, p.e + p.n, [](const CutEntry &a, const CutEntry &b) {
    return a.table != b.table ? a.table < b.table : a.merge_level < b.merge_level;
  });
  return p;
}

size_t cut_blocks(size_t n_colours) { return (n_colours + CUT_CHUNK - 1) / CUT_CHUNK; }

// Where the table kernel reads the catalogue.  The key pass costs about one table's walk over the records themselves (4096^2, 1.83 M
// colours: 30 us for the pass, then 27 us a table against 50 - 58 us a table from the 72-byte records: DESIGN.md section 4.4.1), so
// ONE table with a catalogue threshold reads the records and needs no keys; from two tables on the keys pay.
CutSource cut_source(const CutPlan &p) {
  uint32_t n = 0;
  for (uint32_t j = 0; j < p.n_tables; ++j) n += p.min_sum_w[j] != 0 || p.min_w_max[j] != 0 || p.min_depth[j] != 0;
  if (n == 0) return CUT_TREE_ONLY;
  static const char *forced = tuning_env("WS_CUT_TABLE_FROM_RECORDS");      // A/B knob for tools/: 1 always the records, 0 always the keys
  if (forced) return forced[0] == '1' ? CUT_RECORDS : CUT_KEYS;
  return n == 1 ? CUT_RECORDS : CUT_KEYS;
}

// the context's workspace of a call without measuring (with: measure_reserve on top): the tables (4 B a colour and cut at most), with lists the counters (the same) and 12 B per
// CUT_CHUNK colours and cut for the compaction, the flag words, and for CUT_KEYS the packed keys (16 B a colour)
int cut_reserve(ws_ctx *c, size_t n_seeds, size_t n_cuts, bool lists, CutSource src) {
  const size_t n_colours = n_seeds + 1;
  int rc;
  if ((rc = ensure(c, c->cut_tables, n_cuts * n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->cut_flags, CUT_F_WORDS * sizeof(uint32_t)))) return rc;
  if (src == CUT_KEYS && (rc = ensure(c, c->cut_keys, n_colours * sizeof(CutKey)))) return rc;
  if (lists) {
    if ((rc = ensure(c, c->cut_counts, n_cuts * n_colours * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->cut_blocks, n_cuts * cut_blocks(n_colours) * (sizeof(uint32_t) + sizeof(u64c)) + n_cuts * sizeof(uint32_t)))) return rc;
  }
  return WS_OK;
}

int read_flags(ws_ctx *c, uint32_t *host) {
  HIP_TRY(c, hipMemcpyAsync(host, c->cut_flags.p, CUT_F_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

// What ws_tree_cut_catalogue_device adds to a call: the weights and where the records go.  region (nullable): the caller's device
// records, next to d_lakes; hidden (nullable): n_cuts records on the HOST.
struct CutMeasure {
  LakeWeights wt;
  ws_lake_stats *region, *hidden;
};

const ws_lake_stats LAKE_IDENTITY{0, 0, 0, 0, 0, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};

// the most accumulator entries a measuring call can need: a record per list entry -- no more than cap, or a call would have
// ended with WS_ERR_CAPACITY before it measured, and no more than a cut shows (a colour, or a pixel, each) -- and one per cut
size_t measure_entries(size_t n_seeds, size_t n, size_t n_cuts, bool records, size_t cap) {
  return (records ? std::min(cap, n_cuts * std::min(n_seeds, n)) : 0) + n_cuts;
}

// the context's workspace of the measuring: LAKE_ACC_BYTES an entry, and the cuts' hidden records before they cross the bus
int measure_reserve(ws_ctx *c, size_t entries, size_t n_cuts) {
  if (int rc = ensure(c, c->cut_acc, entries * LAKE_ACC_BYTES)) return rc;
  return ensure(c, c->cut_hidden, n_cuts * sizeof(ws_lake_stats));
}

// The regions of plan's cuts measured into m.region[0 .. total) and, behind them, the hidden pixels of cut k into entry total + k:
// accumulators to the identity, the fold, the records; m.hidden is on its way when this returns (the caller waits for the stream).
// index: the counters as CUT_INDEX left them, or nullptr with total == 0 (the hidden records alone).
int measure_cuts(ws_ctx *c, const TreeRec *tree, size_t n_seeds, const uint32_t *tables, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t n,
                 size_t w, const CutPlan &plan, size_t n_cuts, const uint32_t *index, size_t total, const CutMeasure &m, uint32_t *flags) {
  const size_t n_rec = total + n_cuts;
  u64c *sum = (u64c *)c->cut_acc.p;
  uint32_t *box = (uint32_t *)(sum + 6 * n_rec);
  LakeRec *d_hidden = (LakeRec *)c->cut_hidden.p;
  const unsigned per_entry = (unsigned)((n_rec + 255) / 256);
  k_lake_init<<<per_entry, 256, 0, c->stream>>>(sum, box, n_rec);
  HIP_TRY(c, hipGetLastError());
  // the grid of the render with lists: a workgroup's table serves a run of several steps on a large plane
  const size_t runs = (n + 1023) / 1024, steps = std::max<size_t>((runs + 4095) / 4096, 1);
  const unsigned blocks = (unsigned)((runs + steps - 1) / steps);
  if (m.wt.u16)
    k_cut_measure<uint16_t><<<blocks, 256, 0, c->stream>>>(tree, (uint32_t)n_seeds, tables, d_keys, d_seg_labels, n, steps, plan, index, m.wt, (uint32_t)w, sum, box, n_rec, flags);
  else
    k_cut_measure<uint8_t><<<blocks, 256, 0, c->stream>>>(tree, (uint32_t)n_seeds, tables, d_keys, d_seg_labels, n, steps, plan, index, m.wt, (uint32_t)w, sum, box, n_rec, flags);
  HIP_TRY(c, hipGetLastError());
  k_cut_measure_write<<<per_entry, 256, 0, c->stream>>>(sum, box, n_rec, total, reinterpret_cast<LakeRec *>(m.region), d_hidden);
  HIP_TRY(c, hipGetLastError());
  if (m.hidden) HIP_TRY(c, hipMemcpyAsync(m.hidden, d_hidden, n_cuts * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  return WS_OK;
}

// ws_tree_cut_device, ws_tree_cut_stats_device and ws_tree_cut_catalogue_device: every check, the tree's verdict, the tables, the
// render, the lists and, with m, the measuring.  Without a catalogue threshold d_stats is never read and the launches are those of
// a call that has none; without m they are those of ws_tree_cut_stats_device.
int cut_run(ws_ctx *c, const ws_tree_node *d_tree, const ws_lake_stats *d_stats, size_t n_seeds, const uint32_t *d_keys, const uint32_t *d_seg_labels,
            size_t h, size_t w, const Cuts &cs, uint32_t *d_out, size_t plane_stride, ws_lake *d_lakes, size_t cap, size_t *n_lakes,
            uint64_t *offsets, uint64_t *hidden, const CutMeasure *m = nullptr) {
  const size_t n = h * w, n_cuts = cs.n;
  if ((!d_tree && n_seeds) || ((!d_keys || !d_seg_labels) && n)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (!d_out && !d_lakes) return fail(c, WS_ERR_BAD_ARG, "no output: d_out and d_lakes are both null");
  if (d_lakes && (!n_lakes || !offsets || !hidden)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (m && m->region && !d_lakes) return fail(c, WS_ERR_BAD_ARG, "d_region_stats needs d_lakes: the records lie next to the lists");
  if (int rc = check_cuts(c, cs)) return rc;
  if (cs.catalogue && !d_stats) return fail(c, WS_ERR_BAD_ARG, "a cut has a catalogue threshold and d_stats is null");
  if (h && n / h != w) return fail(c, WS_ERR_TOO_LARGE, "plane too large");
  if (n > 0xFFFFFFFFull || n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "the plane has 2^32 pixels or more, or too many seeds");
  if (d_out && plane_stride < n) return fail(c, WS_ERR_BAD_ARG, "plane_stride is shorter than the plane");
  if (d_out && n && (d_out == d_keys || d_out == d_seg_labels)) return fail(c, WS_ERR_BAD_ARG, "d_out must not be an input plane");
  if (n_cuts == 0) return WS_OK;
  const bool lists = d_lakes != nullptr;
  if (lists && n_cuts * (n_seeds + 1) > 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "lists: cuts x (seeds + 1) must stay below 2^32");
  HIP_TRY(c, hipSetDevice(c->device));
  if (m)
    if (int rc = measure_reserve(c, measure_entries(n_seeds, n, n_cuts, m->region != nullptr, cap), n_cuts)) return rc;
  if (n_seeds == 0 || n == 0) {      // no colour or no pixel: nothing is shown
    const bool fold = m && m->hidden && n;      // ... and every pixel is hidden: one fold of the plane, the same record for every cut
    if (fold)
      if (int rc = ensure(c, c->cut_flags, CUT_F_WORDS * sizeof(uint32_t))) return rc;
    for (size_t k = 0; d_out && n && k < n_cuts; ++k) HIP_TRY(c, hipMemsetAsync(d_out + k * plane_stride, 0, n * sizeof(uint32_t), c->stream));
    if (lists) {
      *n_lakes = 0;
      for (size_t k = 0; k < n_cuts; ++k) { offsets[k] = 0; hidden[k] = n; }
      offsets[n_cuts] = 0;
    }
    if (fold) {
      CutPlan one{};
      one.n = one.n_tables = 1;
      const CutMeasure first{m->wt, nullptr, m->hidden};
      if (int rc = measure_cuts(c, nullptr, 0, nullptr, d_keys, d_seg_labels, n, w, one, 1, nullptr, 0, first, (uint32_t *)c->cut_flags.p)) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t k = fold ? 1 : 0; m && m->hidden && k < n_cuts; ++k) m->hidden[k] = fold ? m->hidden[0] : LAKE_IDENTITY;
    return WS_OK;
  }
  const size_t n_colours = n_seeds + 1;
  const CutPlan plan = make_plan(cs);
  const CutSource src = cut_source(plan);
  if (int rc = cut_reserve(c, n_seeds, n_cuts, lists, src)) return rc;
  const TreeRec *tree = reinterpret_cast<const TreeRec *>(d_tree);
  uint32_t *flags = (uint32_t *)c->cut_flags.p, *tables = (uint32_t *)c->cut_tables.p, *counts = lists ? (uint32_t *)c->cut_counts.p : nullptr;
  uint32_t seen[CUT_F_WORDS];
  const unsigned per_colour = (unsigned)((n_colours + 255) / 256);
  // the records first, and the verdict on the host before anything walks
  HIP_TRY(c, hipMemsetAsync(flags, 0, CUT_F_WORDS * sizeof(uint32_t), c->stream));
  k_cut_check<<<per_colour, 256, 0, c->stream>>>(tree, n_colours, (reinterpret_cast<uintptr_t>(d_tree) & 15u) == 0, flags);
  HIP_TRY(c, hipGetLastError());
  if (int rc = read_flags(c, seen)) return rc;
  if (seen[CUT_F_TREE]) return fail(c, WS_ERR_BAD_ARG, "d_tree is not a merge tree (ws_merge_tree_device's records)");
  const dim3 table_grid(per_colour, plan.n_tables);
  const LakeRec *stats = reinterpret_cast<const LakeRec *>(d_stats);
  if (src == CUT_TREE_ONLY) {
    k_cut_table<CUT_TREE_ONLY><<<table_grid, 256, 0, c->stream>>>(tree, nullptr, nullptr, n_colours, plan, tables, flags);
  } else if (src == CUT_RECORDS) {
    k_cut_table<CUT_RECORDS><<<table_grid, 256, 0, c->stream>>>(tree, nullptr, stats, n_colours, plan, tables, flags);
  } else {
    CutKey *ckeys = (CutKey *)c->cut_keys.p;
    k_cut_keys<<<per_colour, 256, 0, c->stream>>>(tree, stats, n_colours, ckeys);
    HIP_TRY(c, hipGetLastError());
    k_cut_table<CUT_KEYS><<<table_grid, 256, 0, c->stream>>>(tree, ckeys, nullptr, n_colours, plan, tables, flags);
  }
  HIP_TRY(c, hipGetLastError());
  if (lists) HIP_TRY(c, hipMemsetAsync(counts, 0, n_cuts * n_colours * sizeof(uint32_t), c->stream));
  {      // 1024 pixels a step.  Planes alone: one step a workgroup, the finer grain evens out the walks (4096^2, 8 cuts: 1.17 ms
         // against 1.87 with 2048 workgroups).  Lists: at most 4096 workgroups on a large plane, so that a workgroup's table serves
         // a run of several steps (4096^2, 1 and 8 cuts with lists, wall: 0.51 / 3.21 ms at 2048, 0.50 / 2.86 at 4096, 0.62 / 2.74 at
         // 8192: more workgroups even out the walks, and write more tables out)
    const size_t runs = (n + 1023) / 1024, steps = lists ? std::max<size_t>((runs + 4095) / 4096, 1) : 1;
    const unsigned blocks = (unsigned)((runs + steps - 1) / steps);
    if (lists) k_render_cut<true><<<blocks, 256, 0, c->stream>>>(tree, (uint32_t)n_seeds, tables, d_keys, d_seg_labels, n, steps, plan, d_out, plane_stride, counts, flags);
    else k_render_cut<false><<<blocks, 256, 0, c->stream>>>(tree, (uint32_t)n_seeds, tables, d_keys, d_seg_labels, n, steps, plan, d_out, plane_stride, nullptr, flags);
  }
  HIP_TRY(c, hipGetLastError());
  if (!lists) {
    if (int rc = read_flags(c, seen)) return rc;
    if (seen[CUT_F_LABEL]) return fail(c, WS_ERR_BAD_ARG, "a label above n_seeds in d_seg_labels");
    if (seen[CUT_F_STEPS]) return fail(c, WS_ERR_BAD_ARG, "a walk did not end: d_tree changed under the call");
    if (m) {      // (no list, so no record: the hidden pixels alone)
      if (int rc = measure_cuts(c, tree, n_seeds, tables, d_keys, d_seg_labels, n, w, plan, n_cuts, nullptr, 0, *m, flags)) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return WS_OK;
  }
  // the records: nonzero counters per block of colours, summed on the host (which owes the caller the offsets anyway)
  const size_t bpc = cut_blocks(n_colours), nb = n_cuts * bpc;
  uint32_t *block_n = (uint32_t *)((u64c *)c->cut_blocks.p + nb);
  u64c *block_base = (u64c *)c->cut_blocks.p;
  k_cut_compact<CUT_COUNT><<<dim3((unsigned)bpc, (unsigned)n_cuts), 256, 0, c->stream>>>(counts, n_colours, (uint32_t)bpc, block_n, nullptr, nullptr, nullptr, 0u);
  HIP_TRY(c, hipGetLastError());
  std::vector<uint32_t> host_n(nb + n_cuts);      // (behind the blocks' counts: entry 0 of every cut's counters)
  std::vector<u64c> host_base(nb);
  HIP_TRY(c, hipMemcpyAsync(host_n.data(), block_n, (nb + n_cuts) * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (int rc = read_flags(c, seen)) return rc;
  if (seen[CUT_F_LABEL]) return fail(c, WS_ERR_BAD_ARG, "a label above n_seeds in d_seg_labels");
  if (seen[CUT_F_STEPS]) return fail(c, WS_ERR_BAD_ARG, "a walk did not end: d_tree changed under the call");
  u64c total = 0;
  for (size_t b = 0; b < nb; ++b) { host_base[b] = total; total += host_n[b]; }
  *n_lakes = (size_t)total;
  if (total > cap) return fail(c, WS_ERR_CAPACITY, "lake buffer too small");
  for (size_t k = 0; k < n_cuts; ++k) { offsets[k] = host_base[k * bpc]; hidden[k] = host_n[nb + k]; }
  offsets[n_cuts] = total;
  const bool records = m && m->region;      // the counters become the records' positions (total == 0: the hidden entries still)
  if (total || records) {
    HIP_TRY(c, hipMemcpyAsync(block_base, host_base.data(), nb * sizeof(u64c), hipMemcpyHostToDevice, c->stream));
    const dim3 grid((unsigned)bpc, (unsigned)n_cuts);
    if (records) k_cut_compact<CUT_INDEX><<<grid, 256, 0, c->stream>>>(nullptr, n_colours, (uint32_t)bpc, nullptr, block_base, d_lakes, counts, (uint32_t)total);
    else k_cut_compact<CUT_WRITE><<<grid, 256, 0, c->stream>>>(counts, n_colours, (uint32_t)bpc, nullptr, block_base, d_lakes, nullptr, 0u);
    HIP_TRY(c, hipGetLastError());
  }
  if (m)
    if (int rc = measure_cuts(c, tree, n_seeds, tables, d_keys, d_seg_labels, n, w, plan, n_cuts, records ? counts : nullptr, records ? (size_t)total : 0, *m, flags))
      return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (host_base is read by the copy until here)
  return WS_OK;
}

// ---- the cut of a cube of slices --------------------------------------------------------------------------
// The context's workspace of a cube (or of one group of a cube) of n_slices slices with `seeds` seeds and n pixels in all: the
// forest (16 B a record), the tables and, with lists, the counters (4 B a record and cut each), 12 B per CUT_CHUNK counters, the
// slices' first records (4 B a slice) and 16 B per slice and cut for where a list begins and what it hides; measuring: the
// accumulators (68 B per record the call can end with and per slice and cut) and 72 B per slice and cut of hidden records.  No
// term pads a slice.
int cube_reserve(ws_ctx *c, size_t n_slices, size_t seeds, size_t n, const Cuts &cs, bool lists, bool measure, bool records, size_t cap) {
  const size_t n_rec = seeds + n_slices, n_cuts = cs.n, nsc = n_slices * n_cuts;
  const CutSource src = cut_source(make_plan(cs));
  int rc;
  if ((rc = ensure(c, c->cut_forest, n_rec * sizeof(TreeRec)))) return rc;
  if ((rc = ensure(c, c->cut_slices, 2 * nsc * sizeof(u64c) + (n_slices + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->cut_tables, n_cuts * n_rec * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->cut_flags, CUT_F_WORDS * sizeof(uint32_t)))) return rc;
  if (src == CUT_KEYS && (rc = ensure(c, c->cut_keys, n_rec * sizeof(CutKey)))) return rc;
  if (lists) {
    if ((rc = ensure(c, c->cut_counts, n_cuts * n_rec * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->cut_blocks, cut_blocks(n_cuts * n_rec) * (sizeof(uint32_t) + sizeof(u64c))))) return rc;
  }
  if (measure) {
    const size_t entries = (records ? std::min(cap, n_cuts * std::min(seeds, n)) : 0) + nsc;
    if ((rc = ensure(c, c->cut_acc, entries * LAKE_ACC_BYTES))) return rc;
    if ((rc = ensure(c, c->cut_hidden, nsc * sizeof(ws_lake_stats)))) return rc;
  }
  return WS_OK;
}

// What every cube form checks of its cut outputs before anything runs (the single call's refusals)
int cube_check_outputs(ws_ctx *c, const Cuts &cs, bool have_stats, const uint32_t *d_out, const ws_lake *d_lakes, const ws_lake_stats *region,
                       const size_t *n_lakes, const uint64_t *offsets, const uint64_t *hidden) {
  if (!d_out && !d_lakes) return fail(c, WS_ERR_BAD_ARG, "no output: d_out and d_lakes are both null");
  if (d_lakes && (!n_lakes || !offsets || !hidden)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (region && !d_lakes) return fail(c, WS_ERR_BAD_ARG, "d_region_stats needs d_lakes: the records lie next to the lists");
  if (int rc = check_cuts(c, cs)) return rc;
  if (cs.catalogue && !have_stats) return fail(c, WS_ERR_BAD_ARG, "a cut has a catalogue threshold and d_stats is null");
  return WS_OK;
}

// The driver of the cube forms on checked arguments: q.n_slices > 0, 1 .. 32 cuts, n_slices * h * w < 2^32 and, with lists,
// n_cuts * (seeds + n_slices) < 2^32.  Order: the slices' first records up, ONE check pass and ONE verdict for all records, the
// tables over the forest, the render, (lists) count -- host sums -- write, (measuring) init, fold, records.  Lists, offsets and
// hidden counts are the cube's own, from 0; q.cap too small: *n_lakes is the need, WS_ERR_CAPACITY, nothing else written.
int cube_run(ws_ctx *c, const CutCube &q, const Cuts &cs) {
  const size_t plane = q.h * q.w, n = q.n_slices * plane, n_cuts = cs.n, nsc = q.n_slices * n_cuts;
  const size_t seeds = q.seed_offsets[q.n_slices] - q.seed_offsets[0], n_rec = seeds + q.n_slices;
  const bool lists = q.d_lakes != nullptr, measure = q.measure && (q.d_region_stats || q.hidden_stats), records = measure && q.d_region_stats;
  HIP_TRY(c, hipSetDevice(c->device));
  if (n == 0) {      // no pixel: nothing is shown and nothing is hidden
    if (lists) {
      *q.n_lakes = 0;
      for (size_t i = 0; i < nsc; ++i) q.offsets[i] = q.hidden[i] = 0;
      q.offsets[nsc] = 0;
    }
    for (size_t i = 0; measure && q.hidden_stats && i < nsc; ++i) q.hidden_stats[i] = LAKE_IDENTITY;
    return WS_OK;
  }
  if (int rc = cube_reserve(c, q.n_slices, seeds, n, cs, lists, measure, records, q.cap)) return rc;
  const CutPlan plan = make_plan(cs);
  const CutSource src = cut_source(plan);
  std::vector<uint32_t> rb(q.n_slices + 1);
  for (size_t k = 0; k <= q.n_slices; ++k) rb[k] = (uint32_t)(q.seed_offsets[k] - q.seed_offsets[0] + k);
  u64c *seg_first = (u64c *)c->cut_slices.p, *seg_hidden = seg_first + nsc;
  uint32_t *d_rb = (uint32_t *)(seg_hidden + nsc);
  const CutSlices sl{d_rb, (uint32_t)q.n_slices, (uint32_t)plane, (uint32_t)n_cuts};
  const TreeRec *forest = (const TreeRec *)c->cut_forest.p;
  uint32_t *flags = (uint32_t *)c->cut_flags.p, *tables = (uint32_t *)c->cut_tables.p, *counts = lists ? (uint32_t *)c->cut_counts.p : nullptr;
  uint32_t seen[CUT_F_WORDS];
  HIP_TRY(c, hipMemcpyAsync(d_rb, rb.data(), rb.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipMemsetAsync(flags, 0, CUT_F_WORDS * sizeof(uint32_t), c->stream));
  if (seeds) {      // the records first, and the verdict on the host before anything walks (no seed at all: nothing walks, no record is read)
    const unsigned per_rec = (unsigned)((n_rec + 255) / 256);
    k_cut_check_slices<<<per_rec, 256, 0, c->stream>>>(reinterpret_cast<const TreeRec *>(q.d_tree), n_rec, sl, (reinterpret_cast<uintptr_t>(q.d_tree) & 15u) == 0,
                                                       (TreeRec *)c->cut_forest.p, flags);
    HIP_TRY(c, hipGetLastError());
    if (int rc = read_flags(c, seen)) return rc;
    if (seen[CUT_F_TREE]) return fail(c, WS_ERR_BAD_ARG, "d_tree is not a merge tree within every slice (ws_merge_tree_batch_device's records)");
    const dim3 table_grid(per_rec, plan.n_tables);
    const LakeRec *stats = reinterpret_cast<const LakeRec *>(q.d_stats);
    if (src == CUT_TREE_ONLY) {
      k_cut_table<CUT_TREE_ONLY><<<table_grid, 256, 0, c->stream>>>(forest, nullptr, nullptr, n_rec, plan, tables, flags);
    } else if (src == CUT_RECORDS) {
      k_cut_table<CUT_RECORDS><<<table_grid, 256, 0, c->stream>>>(forest, nullptr, stats, n_rec, plan, tables, flags);
    } else {
      CutKey *ckeys = (CutKey *)c->cut_keys.p;
      k_cut_keys<<<per_rec, 256, 0, c->stream>>>(forest, stats, n_rec, ckeys);
      HIP_TRY(c, hipGetLastError());
      k_cut_table<CUT_KEYS><<<table_grid, 256, 0, c->stream>>>(forest, ckeys, nullptr, n_rec, plan, tables, flags);
    }
    HIP_TRY(c, hipGetLastError());
  }
  const size_t n_counters = n_cuts * n_rec;
  if (lists) HIP_TRY(c, hipMemsetAsync(counts, 0, n_counters * sizeof(uint32_t), c->stream));
  // the grids of cut_run: 1024 pixels a step, with lists at most 4096 workgroups
  const size_t runs = (n + 1023) / 1024, list_steps = std::max<size_t>((runs + 4095) / 4096, 1), steps = lists ? list_steps : 1;
  {
    const unsigned blocks = (unsigned)((runs + steps - 1) / steps);
    if (lists) k_render_cut_slices<true><<<blocks, 256, 0, c->stream>>>(forest, n_rec, sl, tables, q.d_keys, q.d_seg_labels, n, steps, plan, q.d_out, q.plane_stride, counts, flags);
    else k_render_cut_slices<false><<<blocks, 256, 0, c->stream>>>(forest, n_rec, sl, tables, q.d_keys, q.d_seg_labels, n, steps, plan, q.d_out, q.plane_stride, nullptr, flags);
    HIP_TRY(c, hipGetLastError());
  }
  const auto measure_slices = [&](const uint32_t *index, size_t total) -> int {
    const size_t n_acc = total + nsc;
    u64c *sum = (u64c *)c->cut_acc.p;
    uint32_t *box = (uint32_t *)(sum + 6 * n_acc);
    LakeRec *d_hidden = (LakeRec *)c->cut_hidden.p;
    const unsigned per_entry = (unsigned)((n_acc + 255) / 256), blocks = (unsigned)((runs + list_steps - 1) / list_steps);
    k_lake_init<<<per_entry, 256, 0, c->stream>>>(sum, box, n_acc);
    HIP_TRY(c, hipGetLastError());
    if (q.wt.u16)
      k_cut_measure_slices<uint16_t><<<blocks, 256, 0, c->stream>>>(forest, n_rec, sl, tables, q.d_keys, q.d_seg_labels, n, list_steps, plan, index, q.wt, (uint32_t)q.w, sum, box, n_acc, flags);
    else
      k_cut_measure_slices<uint8_t><<<blocks, 256, 0, c->stream>>>(forest, n_rec, sl, tables, q.d_keys, q.d_seg_labels, n, list_steps, plan, index, q.wt, (uint32_t)q.w, sum, box, n_acc, flags);
    HIP_TRY(c, hipGetLastError());
    k_cut_measure_write<<<per_entry, 256, 0, c->stream>>>(sum, box, n_acc, total, reinterpret_cast<LakeRec *>(q.d_region_stats), d_hidden);
    HIP_TRY(c, hipGetLastError());
    if (q.hidden_stats) HIP_TRY(c, hipMemcpyAsync(q.hidden_stats, d_hidden, nsc * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
    return WS_OK;
  };
  if (!lists) {
    if (int rc = read_flags(c, seen)) return rc;
    if (seen[CUT_F_LABEL]) return fail(c, WS_ERR_BAD_ARG, "a label above its slice's seed count in d_seg_labels");
    if (seen[CUT_F_STEPS]) return fail(c, WS_ERR_BAD_ARG, "a walk did not end: d_tree changed under the call");
    if (measure) {      // (no list, so no record: the hidden pixels alone)
      if (int rc = measure_slices(nullptr, 0)) return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
    return WS_OK;
  }
  const size_t nb = cut_blocks(n_counters);
  u64c *block_base = (u64c *)c->cut_blocks.p;
  uint32_t *block_n = (uint32_t *)(block_base + nb);
  k_cut_compact_slices<CUT_COUNT><<<(unsigned)nb, 256, 0, c->stream>>>(counts, n_counters, sl, block_n, nullptr, nullptr, nullptr, 0u, nullptr, nullptr);
  HIP_TRY(c, hipGetLastError());
  std::vector<uint32_t> host_n(nb);
  std::vector<u64c> host_base(nb), host_seg(2 * nsc);
  HIP_TRY(c, hipMemcpyAsync(host_n.data(), block_n, nb * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
  if (int rc = read_flags(c, seen)) return rc;
  if (seen[CUT_F_LABEL]) return fail(c, WS_ERR_BAD_ARG, "a label above its slice's seed count in d_seg_labels");
  if (seen[CUT_F_STEPS]) return fail(c, WS_ERR_BAD_ARG, "a walk did not end: d_tree changed under the call");
  u64c total = 0;
  for (size_t b = 0; b < nb; ++b) { host_base[b] = total; total += host_n[b]; }
  *q.n_lakes = (size_t)total;
  if (total > q.cap) return fail(c, WS_ERR_CAPACITY, "lake buffer too small");
  HIP_TRY(c, hipMemcpyAsync(block_base, host_base.data(), nb * sizeof(u64c), hipMemcpyHostToDevice, c->stream));
  if (records) k_cut_compact_slices<CUT_INDEX><<<(unsigned)nb, 256, 0, c->stream>>>(nullptr, n_counters, sl, nullptr, block_base, q.d_lakes, counts, (uint32_t)total, seg_first, seg_hidden);
  else k_cut_compact_slices<CUT_WRITE><<<(unsigned)nb, 256, 0, c->stream>>>(counts, n_counters, sl, nullptr, block_base, q.d_lakes, nullptr, 0u, seg_first, seg_hidden);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(host_seg.data(), seg_first, 2 * nsc * sizeof(u64c), hipMemcpyDeviceToHost, c->stream));
  if (measure)
    if (int rc = measure_slices(records ? counts : nullptr, records ? (size_t)total : 0)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t i = 0; i < nsc; ++i) { q.offsets[i] = host_seg[i]; q.hidden[i] = host_seg[nsc + i]; }
  q.offsets[nsc] = total;
  return WS_OK;
}

// ws_merge_tree_cut and ws_merge_tree_stats_cut: the transform's host form (with lw: ws_merge_tree_stats, whose catalogue stays on
// the context next to the records, the labels and the stamps), the device call on what it left there, the download.
struct CutWeights {
  const void *weight;
  int dtype;
  size_t stride;
  ws_lake_stats *stats;      // nullable: where the caller wants the catalogue
  // ws_merge_tree_cut_catalogue: the regions' records next to `lakes` and the cuts' hidden records (host memory, both nullable)
  ws_lake_stats *region_stats = nullptr, *hidden_stats = nullptr;
};

int merge_tree_cut_host(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                        const ws_options *opt, const CutWeights *lw, const Cuts &cs, ws_tree_node *tree, uint64_t *out, ws_lake *lakes, size_t cap,
                        size_t *n_lakes, uint64_t *offsets, uint64_t *hidden) {
  if (!opt || (!img && h * w) || (!seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (!out && !lakes) return fail(c, WS_ERR_BAD_ARG, "no output: out and lakes are both null");
  if (lakes && (!n_lakes || !offsets || !hidden)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  const bool measure = lw && (lw->region_stats || lw->hidden_stats);
  if (measure && lw->region_stats && !lakes) return fail(c, WS_ERR_BAD_ARG, "region_stats needs lakes: the records lie next to the lists");
  if (int rc = check_cuts(c, cs)) return rc;
  size_t ph = 0, pw = 0;
  if (int rc = check_plane(c, h, w, row_stride, opt, &ph, &pw)) return rc;
  if (n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  const size_t n_cuts = cs.n;
  if (n_cuts == 0) return WS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = ph * pw;
  // every buffer before the transform: one that moves afterwards would not disturb it, but the level loop's graphs are keyed by them
  if (int rc = cut_reserve(c, n_seeds, n_cuts, lakes != nullptr, cut_source(make_plan(cs)))) return rc;
  if (out && n)
    if (int rc = ensure(c, c->cut_planes, n_cuts * n * sizeof(uint32_t))) return rc;
  if (lakes)
    if (int rc = ensure(c, c->cut_lakes, std::max<size_t>(cap, 1) * sizeof(ws_lake))) return rc;
  if (measure) {
    if (int rc = measure_reserve(c, measure_entries(n_seeds, n, n_cuts, lw->region_stats != nullptr, cap), n_cuts)) return rc;
    if (lw->region_stats)
      if (int rc = ensure(c, c->cut_region, std::max<size_t>(cap, 1) * sizeof(ws_lake_stats))) return rc;
  }
  std::vector<ws_tree_node> own;
  if (!tree) { own.resize(n_seeds + 1); tree = own.data(); }
  // upload, flood, stamped unions and the records; the segmenting labels, the stamps and the records stay on the context
  const ws_lake_stats *d_stats = nullptr;
  if (lw) {
    std::vector<ws_lake_stats> own_stats;
    ws_lake_stats *stats = lw->stats;
    if (!stats) { own_stats.resize(n_seeds + 1); stats = own_stats.data(); }
    if (int rc = ws_merge_tree_stats(c, img, h, w, row_stride, seeds_rc, n_seeds, opt, lw->weight, lw->dtype, lw->stride, tree, stats, nullptr)) return rc;
    d_stats = (const ws_lake_stats *)c->lake_out.p;
  } else if (int rc = ws_merge_tree(c, img, h, w, row_stride, seeds_rc, n_seeds, opt, tree, nullptr)) {
    return rc;
  }
  uint32_t *planes = out ? (uint32_t *)c->cut_planes.p : nullptr;
  ws_lake *d_lakes = lakes ? (ws_lake *)c->cut_lakes.p : nullptr;
  CutMeasure m{};
  if (measure) {      // the weights as ws_merge_tree_stats left them on the device: its own contiguous plane, or the image, w elements a row
    const bool own_plane = lw->weight && h * w;
    m = CutMeasure{LakeWeights{own_plane ? c->lake_weight.p : c->img.p, w, (uint32_t)h, (uint32_t)w, opt->edge_correction ? 1u : 0u,
                               own_plane && lw->dtype == WS_U16},
                   lw->region_stats ? (ws_lake_stats *)c->cut_region.p : nullptr, lw->hidden_stats};
  }
  if (int rc = cut_run(c, (const ws_tree_node *)c->tree_out.p, d_stats, n_seeds, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, ph, pw, cs,
                       planes, n, d_lakes, cap, n_lakes, offsets, hidden, measure ? &m : nullptr))
    return rc;
  if (lakes && *n_lakes) HIP_TRY(c, hipMemcpyAsync(lakes, d_lakes, *n_lakes * sizeof(ws_lake), hipMemcpyDeviceToHost, c->stream));
  if (measure && lw->region_stats && *n_lakes)
    HIP_TRY(c, hipMemcpyAsync(lw->region_stats, m.region, *n_lakes * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  if (out && n) {
    if (host_copy_in_chunks(c, n_cuts * n)) {
      if (int rc = labels_to_host_u64(c, planes, out, n_cuts * n)) return rc;
    } else {
      for (size_t k = 0; k < n_cuts; ++k)
        if (int rc = labels_to_host_u64(c, planes + k * n, out + k * n, n)) return rc;
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

}  // namespace

namespace wsapi {

// what ws_batch.hip calls of the cube's cut (ws_lists.hpp)
int cut_cube_check(ws_ctx *c, const CutCube &q, bool have_stats) {
  return cube_check_outputs(c, take_cuts(q.cuts, q.n_cuts), have_stats, q.d_out, q.d_lakes, q.measure ? q.d_region_stats : nullptr, q.n_lakes, q.offsets,
                            q.hidden);
}

int cut_cube_sizes(ws_ctx *c, size_t n_slices, size_t seeds, size_t plane, size_t n_cuts, bool lists) {
  if (plane && n_slices > 0xFFFFFFFFull / plane) return fail(c, WS_ERR_TOO_LARGE, "the cube has 2^32 pixels or more");
  if (seeds + n_slices >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (lists && n_cuts * (seeds + n_slices) > 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "lists: cuts x (seeds + slices) must stay below 2^32");
  return WS_OK;
}

int cut_cube_reserve(ws_ctx *c, size_t n_slices, size_t seeds, size_t n, const CutCube &q) {
  const bool measure = q.measure && (q.d_region_stats || q.hidden_stats);
  return cube_reserve(c, n_slices, seeds, n, take_cuts(q.cuts, q.n_cuts), q.d_lakes != nullptr, measure, measure && q.d_region_stats, q.cap);
}

int cut_cube_run(ws_ctx *c, const CutCube &q) { return cube_run(c, q, take_cuts(q.cuts, q.n_cuts)); }

}  // namespace wsapi

extern "C" {

int ws_tree_cut_catalogue_batch_device(ws_ctx *c, const ws_tree_node *d_tree, const ws_lake_stats *d_stats, size_t n_slices, const size_t *seed_offsets,
                                       const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w, const void *d_weight, int weight_dtype,
                                       size_t weight_row_stride, size_t weight_slice_stride, const ws_lake_cut *cuts, size_t n_cuts, uint32_t *d_out,
                                       size_t plane_stride, ws_lake *d_lakes, ws_lake_stats *d_region_stats, size_t cap, size_t *n_lakes,
                                       uint64_t *offsets, uint64_t *hidden, ws_lake_stats *hidden_stats) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (n_slices && !seed_offsets) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  for (size_t k = 0; k < n_slices; ++k)
    if (seed_offsets[k + 1] < seed_offsets[k]) return fail(c, WS_ERR_BAD_ARG, "seed_offsets must not decrease");
  const size_t seeds = n_slices ? seed_offsets[n_slices] - seed_offsets[0] : 0;
  if (h && h * w / h != w) return fail(c, WS_ERR_TOO_LARGE, "plane too large");
  const size_t plane = h * w;
  if ((!d_tree && seeds) || ((!d_keys || !d_seg_labels) && plane && n_slices)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  CutCube q;
  q.d_tree = d_tree; q.d_stats = d_stats; q.n_slices = n_slices; q.seed_offsets = seed_offsets; q.d_keys = d_keys; q.d_seg_labels = d_seg_labels;
  q.h = h; q.w = w; q.cuts = cuts; q.n_cuts = n_cuts; q.d_out = d_out; q.plane_stride = plane_stride; q.d_lakes = d_lakes;
  q.d_region_stats = d_region_stats; q.cap = cap; q.n_lakes = n_lakes; q.offsets = offsets; q.hidden = hidden; q.hidden_stats = hidden_stats;
  q.measure = d_region_stats || hidden_stats;
  if (int rc = cut_cube_check(c, q, d_stats != nullptr)) return rc;
  if (int rc = cut_cube_sizes(c, n_slices, seeds, plane, n_cuts, d_lakes != nullptr)) return rc;
  if (d_out && plane_stride < plane) return fail(c, WS_ERR_BAD_ARG, "plane_stride is shorter than the plane");
  if (d_out && plane && n_slices && (d_out == d_keys || d_out == d_seg_labels)) return fail(c, WS_ERR_BAD_ARG, "d_out must not be an input plane");
  if (q.measure) {      // (nothing to measure: the weight arguments are not looked at)
    if (!d_weight) return fail(c, WS_ERR_BAD_ARG, "this form has no image: d_weight is null");
    if (int rc = check_lake_weights(c, w, h, w, d_weight, weight_dtype, weight_row_stride)) return rc;
    if (n_slices > 1 && weight_slice_stride < h * weight_row_stride) return fail(c, WS_ERR_BAD_ARG, "weight_slice_stride < h * weight_row_stride");
    q.wt = LakeWeights{d_weight, weight_row_stride, (uint32_t)h, (uint32_t)w, 0u, weight_dtype == WS_U16, weight_slice_stride};
  }
  if (n_slices == 0 || n_cuts == 0) return WS_OK;
  return cut_cube_run(c, q);
}

int ws_tree_cut_device(ws_ctx *c, const ws_tree_node *d_tree, size_t n_seeds, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h,
                       size_t w, const ws_tree_cut *cuts, size_t n_cuts, uint32_t *d_out, size_t plane_stride, ws_lake *d_lakes, size_t cap,
                       size_t *n_lakes, uint64_t *offsets, uint64_t *hidden) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  return cut_run(c, d_tree, nullptr, n_seeds, d_keys, d_seg_labels, h, w, take_cuts(cuts, n_cuts), d_out, plane_stride, d_lakes, cap, n_lakes, offsets,
                 hidden);
}

int ws_tree_cut_stats_device(ws_ctx *c, const ws_tree_node *d_tree, const ws_lake_stats *d_stats, size_t n_seeds, const uint32_t *d_keys,
                             const uint32_t *d_seg_labels, size_t h, size_t w, const ws_lake_cut *cuts, size_t n_cuts, uint32_t *d_out,
                             size_t plane_stride, ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  return cut_run(c, d_tree, d_stats, n_seeds, d_keys, d_seg_labels, h, w, take_cuts(cuts, n_cuts), d_out, plane_stride, d_lakes, cap, n_lakes, offsets,
                 hidden);
}

int ws_merge_tree_cut(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                      const ws_options *opt, const ws_tree_cut *cuts, size_t n_cuts, ws_tree_node *tree, uint64_t *out, ws_lake *lakes, size_t cap,
                      size_t *n_lakes, uint64_t *offsets, uint64_t *hidden) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  return merge_tree_cut_host(c, img, h, w, row_stride, seeds_rc, n_seeds, opt, nullptr, take_cuts(cuts, n_cuts), tree, out, lakes, cap, n_lakes, offsets,
                             hidden);
}

int ws_merge_tree_stats_cut(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                            const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride, const ws_lake_cut *cuts,
                            size_t n_cuts, ws_tree_node *tree, ws_lake_stats *stats, uint64_t *out, ws_lake *lakes, size_t cap, size_t *n_lakes,
                            uint64_t *offsets, uint64_t *hidden) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  const CutWeights lw{weight, weight_dtype, weight_row_stride, stats};
  return merge_tree_cut_host(c, img, h, w, row_stride, seeds_rc, n_seeds, opt, &lw, take_cuts(cuts, n_cuts), tree, out, lakes, cap, n_lakes, offsets,
                             hidden);
}

int ws_tree_cut_catalogue_device(ws_ctx *c, const ws_tree_node *d_tree, const ws_lake_stats *d_stats, size_t n_seeds, const uint32_t *d_keys,
                                 const uint32_t *d_seg_labels, size_t h, size_t w, const void *d_weight, int weight_dtype, size_t weight_row_stride,
                                 const ws_lake_cut *cuts, size_t n_cuts, uint32_t *d_out, size_t plane_stride, ws_lake *d_lakes,
                                 ws_lake_stats *d_region_stats, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden,
                                 ws_lake_stats *hidden_stats) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!d_region_stats && !hidden_stats)      // nothing to measure: ws_tree_cut_stats_device, the weights are not looked at
    return cut_run(c, d_tree, d_stats, n_seeds, d_keys, d_seg_labels, h, w, take_cuts(cuts, n_cuts), d_out, plane_stride, d_lakes, cap, n_lakes, offsets,
                   hidden);
  if (!d_weight) return fail(c, WS_ERR_BAD_ARG, "this form has no image: d_weight is null");
  if (h && h * w / h != w) return fail(c, WS_ERR_TOO_LARGE, "plane too large");
  if (int rc = check_lake_weights(c, w, h, w, d_weight, weight_dtype, weight_row_stride)) return rc;
  const CutMeasure m{LakeWeights{d_weight, weight_row_stride, (uint32_t)h, (uint32_t)w, 0u, weight_dtype == WS_U16}, d_region_stats, hidden_stats};
  return cut_run(c, d_tree, d_stats, n_seeds, d_keys, d_seg_labels, h, w, take_cuts(cuts, n_cuts), d_out, plane_stride, d_lakes, cap, n_lakes, offsets,
                 hidden, &m);
}

int ws_merge_tree_cut_catalogue(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                                const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride, const ws_lake_cut *cuts,
                                size_t n_cuts, ws_tree_node *tree, ws_lake_stats *stats, uint64_t *out, ws_lake *lakes, ws_lake_stats *region_stats,
                                size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden, ws_lake_stats *hidden_stats) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  CutWeights lw{weight, weight_dtype, weight_row_stride, stats};
  lw.region_stats = region_stats;
  lw.hidden_stats = hidden_stats;
  return merge_tree_cut_host(c, img, h, w, row_stride, seeds_rc, n_seeds, opt, &lw, take_cuts(cuts, n_cuts), tree, out, lakes, cap, n_lakes, offsets,
                             hidden);
}

}  // extern "C"
