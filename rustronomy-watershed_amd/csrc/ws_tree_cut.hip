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
#include "ws_ctx.hpp"
#include "ws_uf.hpp"

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
  uint32_t min_area[CUT_MAX], min_leaves[CUT_MAX];      // per table
};

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
// T_j[c] for every table j of the plan (blockIdx.y): up `parent` while the node is not kept.  The chain ends at an alive node,
// which is kept; at most 255 steps on a checked tree, and the cap holds whatever the records say.
__global__ __launch_bounds__(256) void k_cut_table(const TreeRec *__restrict__ tree, size_t n_colours, CutPlan plan, uint32_t *tables, uint32_t *flags) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_colours) return;
  const uint32_t j = blockIdx.y, min_area = plan.min_area[j], min_leaves = plan.min_leaves[j];
  uint32_t a = (uint32_t)c, steps = 0;
  for (;;) {
    const TreeRec r = tree[a];
    if (r.death_level == TREE_ALIVE || (r.area >= min_area && r.n_leaves >= min_leaves)) break;
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
__device__ __forceinline__ void cut_count(uint32_t *s_key, uint32_t *s_cnt, uint32_t *s_used, uint32_t *counts, bool live, uint32_t key, uint32_t k,
                                          int lane) {
  const unsigned long long todo = __builtin_amdgcn_ballot_w64(live);
  if (todo == 0) return;      // wave uniform
  const int leader = (int)__builtin_ctzll(todo);
  const uint32_t k0 = (uint32_t)__builtin_amdgcn_readlane((int)key, leader);
  const bool same = live && key == k0;
  if (__popcll(__builtin_amdgcn_ballot_w64(same)) > 1) {      // wave uniform
    const uint32_t total = wave_sum_u32(same ? k : 0u);
    if (lane == leader) cut_add(s_key, s_cnt, s_used, counts, k0, total);
    else if (live && !same) cut_add(s_key, s_cnt, s_used, counts, key, k);
  } else if (live) {
    cut_add(s_key, s_cnt, s_used, counts, key, k);
  }
}

// A workgroup takes `steps` consecutive runs of 1024 pixels, a thread four consecutive pixels of each: their stamps and colours once
// (16-byte loads where keys and labels are 16-byte aligned), then cut after cut in the plan's order, and every plane gets its four
// pixels as one 16-byte store where out and plane_stride allow it.  A pixel keeps the node it stands on and that node's parent and
// death level in registers: a step of the walk is ONE dependent load, the four walks of a thread run side by side (one after the
// other they wait for each other's gathers), a cut of the same table as the one before it walks on from where that one stopped
// (merge levels ascend within a table), and a new table starts from its own entry.  The last, short quad of a plane and planes
// off 16-byte alignment load and store pixel by pixel, with the same result.
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
    uint32_t arr[4], col[4];
    bool in[4];
    if (vec_in && whole) {
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
    bool walks[4];      // coloured: the pixel has a chain to walk
    uint32_t a[4], up[4], d[4];      // the node, its parent, its death level
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
    uint32_t table = 0xFFFFFFFFu;
    for (uint32_t j = 0; j < plan.n; ++j) {
      const CutEntry e = plan.e[j];
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
      uint32_t v[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) v[p] = shown[p] ? a[p] : 0u;
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
// counts those with pixels (pass 0: block_n), and, once the host has summed the blocks into bases, writes them behind its base.
constexpr int CUT_PER_THREAD = 4;
constexpr int CUT_CHUNK = 256 * CUT_PER_THREAD;

template <bool WRITE>
__global__ __launch_bounds__(256) void k_cut_compact(const uint32_t *__restrict__ counts, size_t n_colours, uint32_t blocks_per_cut, uint32_t *block_n,
                                                     const u64c *__restrict__ block_base, ws_lake *lakes) {
  __shared__ uint32_t s_n[256];
  const uint32_t k = blockIdx.y, t = threadIdx.x;
  const uint32_t *cnt = counts + (size_t)k * n_colours;
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
  if constexpr (!WRITE) {
    if (t == 255) block_n[b] = s_n[255];
    if (t == 0 && blockIdx.x == 0) block_n[(size_t)gridDim.y * blocks_per_cut + k] = cnt[0];      // behind the blocks: the cut's hidden pixels
  } else {
    u64c at = block_base[b] + (s_n[t] - mine);
#pragma unroll
    for (int j = 0; j < CUT_PER_THREAD; ++j)
      if (area[j] != 0u) lakes[at++] = ws_lake{(uint64_t)(c0 + j), (uint64_t)area[j]};
  }
}

}  // namespace wsk

namespace {

using namespace wsapi;

static_assert(sizeof(ws_tree_cut) == 12, "ws_tree_cut is part of the ABI");

// what both forms check of the cuts before anything runs
int check_cuts(ws_ctx *c, const ws_tree_cut *cuts, size_t n_cuts) {
  if (n_cuts > (size_t)CUT_MAX) return fail(c, WS_ERR_BAD_ARG, "more than 32 cuts");
  if (n_cuts && !cuts) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  for (size_t k = 0; k < n_cuts; ++k) {
    if (cuts[k].show_level > 254 || cuts[k].merge_level > 254) return fail(c, WS_ERR_BAD_ARG, "a cut's level is above 254");
    if (cuts[k].reserved[0] || cuts[k].reserved[1]) return fail(c, WS_ERR_BAD_ARG, "ws_tree_cut.reserved must be zero");
  }
  return WS_OK;
}

// one table per distinct (min_area, min_leaves); the entries by table, then merge level (stable: repeats keep their order)
CutPlan make_plan(const ws_tree_cut *cuts, size_t n_cuts) {
  CutPlan p{};
  p.n = (uint32_t)n_cuts;
  for (size_t k = 0; k < n_cuts; ++k) {
    uint32_t j = 0;
    while (j < p.n_tables && !(p.min_area[j] == cuts[k].min_area && p.min_leaves[j] == cuts[k].min_leaves)) ++j;
    if (j == p.n_tables) {
      p.min_area[j] = cuts[k].min_area;
      p.min_leaves[j] = cuts[k].min_leaves;
      ++p.n_tables;
    }
    p.e[k] = CutEntry{j, cuts[k].merge_level, cuts[k].show_level, (uint8_t)k, 0};
  }
  std::stable_sort(p.e, p.e + p.n, [](const CutEntry &a, const CutEntry &b) {
    return a.table != b.table ? a.table < b.table : a.merge_level < b.merge_level;
  });
  return p;
}

size_t cut_blocks(size_t n_colours) { return (n_colours + CUT_CHUNK - 1) / CUT_CHUNK; }

// the context's workspace of a call: the tables (4 B a colour and cut at most), with lists the counters (the same) and 12 B per
// CUT_CHUNK colours and cut for the compaction, and the flag words
int cut_reserve(ws_ctx *c, size_t n_seeds, size_t n_cuts, bool lists) {
  const size_t n_colours = n_seeds + 1;
  int rc;
  if ((rc = ensure(c, c->cut_tables, n_cuts * n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->cut_flags, CUT_F_WORDS * sizeof(uint32_t)))) return rc;
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

}  // namespace

extern "C" {

int ws_tree_cut_device(ws_ctx *c, const ws_tree_node *d_tree, size_t n_seeds, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h,
                       size_t w, const ws_tree_cut *cuts, size_t n_cuts, uint32_t *d_out, size_t plane_stride, ws_lake *d_lakes, size_t cap,
                       size_t *n_lakes, uint64_t *offsets, uint64_t *hidden) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  const size_t n = h * w;
  if ((!d_tree && n_seeds) || ((!d_keys || !d_seg_labels) && n)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (!d_out && !d_lakes) return fail(c, WS_ERR_BAD_ARG, "no output: d_out and d_lakes are both null");
  if (d_lakes && (!n_lakes || !offsets || !hidden)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int rc = check_cuts(c, cuts, n_cuts)) return rc;
  if (h && n / h != w) return fail(c, WS_ERR_TOO_LARGE, "plane too large");
  if (n > 0xFFFFFFFFull || n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "the plane has 2^32 pixels or more, or too many seeds");
  if (d_out && plane_stride < n) return fail(c, WS_ERR_BAD_ARG, "plane_stride is shorter than the plane");
  if (d_out && n && (d_out == d_keys || d_out == d_seg_labels)) return fail(c, WS_ERR_BAD_ARG, "d_out must not be an input plane");
  if (n_cuts == 0) return WS_OK;
  const bool lists = d_lakes != nullptr;
  if (lists && n_cuts * (n_seeds + 1) > 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "lists: cuts x (seeds + 1) must stay below 2^32");
  HIP_TRY(c, hipSetDevice(c->device));
  if (n_seeds == 0 || n == 0) {      // no colour or no pixel: nothing is shown
    for (size_t k = 0; d_out && n && k < n_cuts; ++k) HIP_TRY(c, hipMemsetAsync(d_out + k * plane_stride, 0, n * sizeof(uint32_t), c->stream));
    if (lists) {
      *n_lakes = 0;
      for (size_t k = 0; k < n_cuts; ++k) { offsets[k] = 0; hidden[k] = n; }
      offsets[n_cuts] = 0;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WS_OK;
  }
  const size_t n_colours = n_seeds + 1;
  if (int rc = cut_reserve(c, n_seeds, n_cuts, lists)) return rc;
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
  const CutPlan plan = make_plan(cuts, n_cuts);
  k_cut_table<<<dim3(per_colour, plan.n_tables), 256, 0, c->stream>>>(tree, n_colours, plan, tables, flags);
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
    return WS_OK;
  }
  // the records: nonzero counters per block of colours, summed on the host (which owes the caller the offsets anyway)
  const size_t bpc = cut_blocks(n_colours), nb = n_cuts * bpc;
  uint32_t *block_n = (uint32_t *)((u64c *)c->cut_blocks.p + nb);
  u64c *block_base = (u64c *)c->cut_blocks.p;
  k_cut_compact<false><<<dim3((unsigned)bpc, (unsigned)n_cuts), 256, 0, c->stream>>>(counts, n_colours, (uint32_t)bpc, block_n, nullptr, nullptr);
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
  if (total) {
    HIP_TRY(c, hipMemcpyAsync(block_base, host_base.data(), nb * sizeof(u64c), hipMemcpyHostToDevice, c->stream));
    k_cut_compact<true><<<dim3((unsigned)bpc, (unsigned)n_cuts), 256, 0, c->stream>>>(counts, n_colours, (uint32_t)bpc, nullptr, block_base, d_lakes);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));      // (host_base is read by the copy until here)
  return WS_OK;
}

int ws_merge_tree_cut(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                      const ws_options *opt, const ws_tree_cut *cuts, size_t n_cuts, ws_tree_node *tree, uint64_t *out, ws_lake *lakes, size_t cap,
                      size_t *n_lakes, uint64_t *offsets, uint64_t *hidden) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || (!img && h * w) || (!seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (!out && !lakes) return fail(c, WS_ERR_BAD_ARG, "no output: out and lakes are both null");
  if (lakes && (!n_lakes || !offsets || !hidden)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int rc = check_cuts(c, cuts, n_cuts)) return rc;
  size_t ph = 0, pw = 0;
  if (int rc = check_plane(c, h, w, row_stride, opt, &ph, &pw)) return rc;
  if (n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (n_cuts == 0) return WS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = ph * pw;
  // every buffer before the transform: one that moves afterwards would not disturb it, but the level loop's graphs are keyed by them
  if (int rc = cut_reserve(c, n_seeds, n_cuts, lakes != nullptr)) return rc;
  if (out && n)
    if (int rc = ensure(c, c->cut_planes, n_cuts * n * sizeof(uint32_t))) return rc;
  if (lakes)
    if (int rc = ensure(c, c->cut_lakes, std::max<size_t>(cap, 1) * sizeof(ws_lake))) return rc;
  std::vector<ws_tree_node> own;
  if (!tree) { own.resize(n_seeds + 1); tree = own.data(); }
  // upload, flood, stamped unions and the records; the segmenting labels, the stamps and the records stay on the context
  if (int rc = ws_merge_tree(c, img, h, w, row_stride, seeds_rc, n_seeds, opt, tree, nullptr)) return rc;
  uint32_t *planes = out ? (uint32_t *)c->cut_planes.p : nullptr;
  ws_lake *d_lakes = lakes ? (ws_lake *)c->cut_lakes.p : nullptr;
  if (int rc = ws_tree_cut_device(c, (const ws_tree_node *)c->tree_out.p, n_seeds, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, ph, pw, cuts,
                                  n_cuts, planes, n, d_lakes, cap, n_lakes, offsets, hidden))
    return rc;
  if (lakes && *n_lakes) HIP_TRY(c, hipMemcpyAsync(lakes, d_lakes, *n_lakes * sizeof(ws_lake), hipMemcpyDeviceToHost, c->stream));
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

}  // extern "C"
