// ws_merge_tree.hip -- gfx950 kernels that read the stamped forest of a merging transform_history run (k_union_stamped,
// ws_merge.hip: hook[b] = the root b was hooked under, death[b] = the level): the history planes, the merge tree and the lake
// statistics and the lakes' second moments, each for one plane and for a stack of slices.  Nothing here changes the union-find.
#include "ws_uf.hpp"
#include "ws_lake_part.hpp"
#include "ws_shape_part.hpp"

namespace wsk {

// ---- history planes (ws_transform_history_device) ----------------------------------------------------------------------------------
// One pass for every requested level: a pixel's stamp and colour are read once, then the levels are walked in ascending order
// and every plane gets its four pixels as one 16-byte store.  The merging colour follows the stamped forest up as L grows:
// the walk only ever moves on, and death[] of the colour it stands on is kept in a register, so a level at which the lake did
// not merge costs no load.
// STACKED (ws_transform_history_batch_device): keys / labels are slices of st.plane pixels, labels in each slice's own colours;
// slice kr's colour c is c + st.base[kr] in the forest, and its planes start at out + kr * st.per_slice * plane_stride.
// st.plane % 4 == 0, so a quad never straddles two slices.
template <bool MERGING, bool STACKED>
__global__ __launch_bounds__(256) void k_render_history(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                        const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook,
                                                        HistoryTable tab, uint32_t *out, size_t plane_stride, size_t n, HistoryStack st) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const bool vec = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0 &&
                   (plane_stride & 3u) == 0 && (!STACKED || (st.plane & 3u) == 0);
  const size_t nq = vec ? n / 4 : 0;
  for (size_t q = tid; q < nq; q += step) {
    const u32x4_m k = reinterpret_cast<const u32x4_m *>(keys)[q], l = reinterpret_cast<const u32x4_m *>(labels)[q];
    uint32_t arr[4] = {k.x >> 24, k.y >> 24, k.z >> 24, k.w >> 24};      // arrival level; KEY_INF: 255, above every level
    uint32_t col[4] = {l.x, l.y, l.z, l.w}, d[4];
    size_t o = 0;      // (STACKED) the quad's word in its slice's first plane
    uint32_t b = 0;    // (STACKED, MERGING) the slice's colour base
    if constexpr (STACKED) {
      const uint32_t i = (uint32_t)(4 * q), kr = i / st.plane;
      o = (size_t)kr * st.per_slice * plane_stride + (i - kr * st.plane);
      if constexpr (MERGING) b = st.base[kr];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      if (col[p] == 0u) arr[p] = 0xFFu;
      if constexpr (STACKED && MERGING) col[p] += b;      // (colour 0 is never shown: arr = 0xFF)
      d[p] = MERGING && arr[p] != 0xFFu ? death[col[p]] : 0xFFFFFFFFu;
    }
    for (uint32_t j = 0; j < tab.n; ++j) {
      const uint32_t e = tab.e[j], L = e & 0xFFu;
      uint32_t v[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        if (MERGING && arr[p] <= L)
          while (d[p] <= L) { col[p] = hook[col[p]]; d[p] = death[col[p]]; }
        v[p] = arr[p] <= L ? col[p] - b : 0u;
      }
      if constexpr (STACKED)
        *reinterpret_cast<u32x4_m *>(out + (size_t)(e >> 8) * plane_stride + o) = u32x4_m{v[0], v[1], v[2], v[3]};
      else
        reinterpret_cast<u32x4_m *>(out + (size_t)(e >> 8) * plane_stride)[q] = u32x4_m{v[0], v[1], v[2], v[3]};
    }
  }
  for (size_t i = nq * 4 + tid; i < n; i += step) {      // the tail (all of the plane when a pointer or the stride is not 16-byte aligned)
    uint32_t a = keys[i] >> 24, c = labels[i];
    if (c == 0u) a = 0xFFu;
    size_t o = i;
    uint32_t b = 0;
    if constexpr (STACKED) {
      const uint32_t kr = (uint32_t)i / st.plane;
      o = (size_t)kr * st.per_slice * plane_stride + ((uint32_t)i - kr * st.plane);
      if constexpr (MERGING) b = st.base[kr];
      c += b;
    }
    uint32_t dc = MERGING && a != 0xFFu ? death[c] : 0xFFFFFFFFu;
    for (uint32_t j = 0; j < tab.n; ++j) {
      const uint32_t e = tab.e[j], L = e & 0xFFu;
      if (MERGING && a <= L)
        while (dc <= L) { c = hook[c]; dc = death[c]; }
      out[(size_t)(e >> 8) * plane_stride + o] = a <= L ? c - b : 0u;
    }
  }
}

hipError_t render_history(hipStream_t s, bool merging, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                          const HistoryTable &tab, uint32_t *out, size_t plane_stride, size_t n) {
  if (n == 0 || tab.n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  if (merging) k_render_history<true, false><<<blocks, 256, 0, s>>>(keys, labels, death, hook, tab, out, plane_stride, n, HistoryStack{});
  else k_render_history<false, false><<<blocks, 256, 0, s>>>(keys, labels, nullptr, nullptr, tab, out, plane_stride, n, HistoryStack{});
  return hipGetLastError();
}

hipError_t render_history_stack(hipStream_t s, bool merging, const uint32_t *keys, const uint32_t *labels, const uint32_t *death,
                                const uint32_t *hook, const HistoryTable &tab, uint32_t *out, size_t plane_stride, size_t n,
                                const HistoryStack &st) {
  if (n == 0 || tab.n == 0) return hipSuccess;
  if (st.plane == 0 || n % st.plane != 0 || n > 0xFFFFFFFFull) return hipErrorInvalidValue;      // (slice indices are u32 divisions)
  const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  if (merging) k_render_history<true, true><<<blocks, 256, 0, s>>>(keys, labels, death, hook, tab, out, plane_stride, n, st);
  else k_render_history<false, true><<<blocks, 256, 0, s>>>(keys, labels, nullptr, nullptr, tab, out, plane_stride, n, st);
  return hipGetLastError();
}

// ---- merge tree (ws_merge_tree_device) ----------------------------------------------------------------------------------------------
//
// The stamped forest of a merging transform_history run IS the lake hierarchy, up to two things: hook[b] is whatever root the racing
// CAS read, not the canonical id, and nothing has counted pixels.  Three steps turn it into one record per colour:
// canonical parents (one walk per colour), own counts (one pass over the stamps), and a fold up the tree in ascending death level.

constexpr int TREE_PER_THREAD = 16;      // colours per thread of the per-colour kernels: a workgroup adds once per level to 256 shared counters
constexpr int TREE_CHUNK = 256 * TREE_PER_THREAD;

// STACKED (ws_merge_tree_batch_device): the forest is that of a stack of st.g slices of st.plane pixels (H = g x slice rows); colour
// c of the forest is colour c - st.base[k] of its slice k, seeds_rc are the stacked seed pairs (flood_stack) and seg holds every
// slice's own colours.  Record 0 of the forest belongs to nobody: every slice's own comes from k_tree_unstack.
template <bool STACKED>
__global__ __launch_bounds__(256) void k_tree_init(const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook,
                                                   const uint32_t *__restrict__ seeds_rc, const uint32_t *__restrict__ seg, int H, int W,
                                                   const u64c *__restrict__ arrived, TreeRec *tree, size_t n_colours, u64c *hist, TreeStack st) {
  __shared__ uint32_t s_h[NLEVELS];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  for (int k = 0; k < TREE_PER_THREAD; ++k) {
    const size_t c = (size_t)blockIdx.x * TREE_CHUNK + (size_t)k * 256 + threadIdx.x;
    if (c >= n_colours) break;
    TreeRec r{0u, TREE_ALIVE, 0u, 0u};
    if (c == 0) {
      if constexpr (!STACKED) r.area = (uint32_t)((u64c)H * (u64c)W - arrived[0]);      // what the last level left uncoloured
    } else {
      const uint32_t y = seeds_rc[2 * (c - 1)], x = seeds_rc[2 * (c - 1) + 1];
      uint32_t own = (uint32_t)c;      // the colour in the plane's own numbering
      if constexpr (STACKED) own -= st.base[slice_of_colour(st.base, st.g, (uint32_t)c)];
      // a later seed on the same pixel overwrites (lib.rs:1670-1677): such a colour never was
      r.n_leaves = y < (uint32_t)H && x < (uint32_t)W && seg[(size_t)y * W + x] == own ? 1u : 0u;
      const uint32_t d = death[c];
      if (d != TREE_ALIVE) {
        uint32_t p = hook[c];
        while (death[p] <= d) p = hook[p];      // <=: a colour that dies at the same level is not that level's root
        r.parent = p;
        r.death_level = d;
        atomicAdd(&s_h[d & (NLEVELS - 1)], 1u);
      }
    }
    tree[c] = r;
  }
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (u64c)s_h[threadIdx.x]);
}

hipError_t tree_init(hipStream_t s, const uint32_t *death, const uint32_t *hook, const uint32_t *seeds_rc, const uint32_t *seg_labels, int h, int w,
                     const u64c *arrived, TreeRec *tree, size_t n_colours, u64c *ws) {
  if (n_colours == 0) return hipSuccess;
  k_tree_init<false><<<(unsigned)((n_colours + TREE_CHUNK - 1) / TREE_CHUNK), 256, 0, s>>>(death, hook, seeds_rc, seg_labels, h, w, arrived, tree, n_colours, ws,
                                                                                           TreeStack{});
  return hipGetLastError();
}

hipError_t tree_init_stack(hipStream_t s, const uint32_t *death, const uint32_t *hook, const uint32_t *stacked_rc, const uint32_t *seg_labels, int h, int w,
                           TreeRec *tree, size_t n_colours, u64c *ws, const TreeStack &st) {
  if (n_colours == 0) return hipSuccess;
  if (st.g == 0 || st.plane == 0 || (size_t)h * (size_t)w != (size_t)st.g * st.plane) return hipErrorInvalidValue;
  k_tree_init<true><<<(unsigned)((n_colours + TREE_CHUNK - 1) / TREE_CHUNK), 256, 0, s>>>(death, hook, stacked_rc, seg_labels, h, w, nullptr, tree, n_colours, ws, st);
  return hipGetLastError();
}

// The seed pixels of a finished transform, from its planes alone (ws_merge_tree_from_arrival_device).  A seed is coloured before
// level 0 (lib.rs:1675-1677) and nothing else is: stamp 0 marks exactly the painted pixels, and the label there is the colour that
// survived the painting.  So every colour that exists has ONE stamp-0 pixel, which writes its (row, col) pair -- no atomics -- and
// a colour that never was keeps the pair the fill left, which k_tree_init reads as "outside the plane".  A plain stream over the
// stamps, 16 bytes a lane; the labels are read only where a stamp is 0.  A label outside 1 .. n_seeds is never an index.
__device__ __forceinline__ void seed_pixel_at(const uint32_t *__restrict__ seg, size_t i, uint32_t W, uint32_t n_seeds, uint2 *out_rc) {
  const uint32_t c = seg[i];
  if (c - 1u < n_seeds) out_rc[c - 1u] = make_uint2((uint32_t)(i / W), (uint32_t)(i % W));
}

__global__ __launch_bounds__(256) void k_seed_pixels(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ seg, size_t n, uint32_t W,
                                                     uint32_t n_seeds, uint2 *out_rc) {
  const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, step = (size_t)gridDim.x * blockDim.x;
  const size_t nq = (reinterpret_cast<uintptr_t>(keys) & 15u) == 0 ? n / 4 : 0;
  for (size_t q = tid; q < nq; q += step) {
    const u32x4_m k = reinterpret_cast<const u32x4_m *>(keys)[q];
    if (k.x != 0u && k.y != 0u && k.z != 0u && k.w != 0u) continue;
    if (k.x == 0u) seed_pixel_at(seg, 4 * q, W, n_seeds, out_rc);
    if (k.y == 0u) seed_pixel_at(seg, 4 * q + 1, W, n_seeds, out_rc);
    if (k.z == 0u) seed_pixel_at(seg, 4 * q + 2, W, n_seeds, out_rc);
    if (k.w == 0u) seed_pixel_at(seg, 4 * q + 3, W, n_seeds, out_rc);
  }
  for (size_t i = nq * 4 + tid; i < n; i += step)      // the tail (all of the plane when the stamps are a view off 16-byte alignment)
    if (keys[i] == 0u) seed_pixel_at(seg, i, W, n_seeds, out_rc);
}

hipError_t seed_pixels_from_planes(hipStream_t s, const uint32_t *keys, const uint32_t *seg, int h, int w, size_t n_colours, uint32_t *out_rc) {
  if (n_colours <= 1) return hipSuccess;
  if (n_colours > 0xFFFFFFFFull || (reinterpret_cast<uintptr_t>(out_rc) & 7u) != 0) return hipErrorInvalidValue;
  const size_t n = (size_t)h * (size_t)w, n_seeds = n_colours - 1;
  hipError_t e = hipMemsetAsync(out_rc, 0xFF, 2 * n_seeds * sizeof(uint32_t), s);
  if (e != hipSuccess || n == 0) return e;
  const unsigned blocks = (unsigned)std::min<size_t>((n / 4 + 255) / 256 + 1, 16384);
  k_seed_pixels<<<blocks, 256, 0, s>>>(keys, seg, n, (uint32_t)w, (uint32_t)n_seeds, reinterpret_cast<uint2 *>(out_rc));
  return hipGetLastError();
}

// Own counts.  Around the percolation level most pixels of the plane land on ONE root, and a same-address atomic retires every ~12 ns:
// a workgroup takes a contiguous run of pixels, counts in an LDS table keyed by root (a wave first adds up the lanes that agree with
// its first lane) and adds to memory once per root it met.  A root that finds no slot within OWN_PROBES adds for itself: exact either way.
constexpr int OWN_SLOTS = 2048, OWN_PROBES = 4;
constexpr uint32_t OWN_EMPTY = 0xFFFFFFFFu;

__device__ __forceinline__ void own_add(uint32_t *s_key, uint32_t *s_cnt, TreeRec *tree, uint32_t r, uint32_t k) {
  const uint32_t h0 = (r * 2654435761u) >> 21;      // 11 bits
  for (int j = 0; j < OWN_PROBES; ++j) {
    const uint32_t slot = (h0 + (uint32_t)j) & (OWN_SLOTS - 1);
    const uint32_t old = atomicCAS(&s_key[slot], OWN_EMPTY, r);
    if (old == OWN_EMPTY || old == r) { atomicAdd(&s_cnt[slot], k); return; }
  }
  atomicAdd(&tree[r].area, k);
}

// STACKED: labels hold every slice's own colours; a quad's slice is i0 / stack.plane (stack.plane % 4 == 0: a quad never straddles two
// slices, a workgroup's runs may) and its colours move to the forest's numbering before the walk, so the table is keyed by forest root.
template <bool STACKED>
__global__ __launch_bounds__(256) void k_tree_own(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                  const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook, TreeRec *tree,
                                                  size_t n, size_t steps, TreeStack stack) {
  __shared__ uint32_t s_key[OWN_SLOTS], s_cnt[OWN_SLOTS];
  for (int j = threadIdx.x; j < OWN_SLOTS; j += 256) { s_key[j] = OWN_EMPTY; s_cnt[j] = 0; }
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool vec = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t i0 = (((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x) * 4;
    uint32_t arr[4], col[4];
    if (vec && i0 + 3 < n) {
      const u32x4_m k = *reinterpret_cast<const u32x4_m *>(keys + i0), l = *reinterpret_cast<const u32x4_m *>(labels + i0);
      arr[0] = k.x >> 24; arr[1] = k.y >> 24; arr[2] = k.z >> 24; arr[3] = k.w >> 24;
      col[0] = l.x; col[1] = l.y; col[2] = l.z; col[3] = l.w;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool in = i0 + p < n;
        arr[p] = in ? keys[i0 + p] >> 24 : 0xFFu;
        col[p] = in ? labels[i0 + p] : 0u;
      }
    }
    if constexpr (STACKED) {
      const uint32_t b = i0 < n ? stack.base[(uint32_t)i0 / stack.plane] : 0u;      // (n < 2^32: tree_own_counts_stack)
#pragma unroll
      for (int p = 0; p < 4; ++p) col[p] += col[p] != 0u ? b : 0u;
    }
    // the four walks side by side (a walk is a chain of dependent gathers: one after the other they were most of the kernel)
    uint32_t r[4], d[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      r[p] = col[p];
      d[p] = col[p] != 0u && arr[p] != 0xFFu ? death[col[p]] : TREE_ALIVE;      // (as k_render_history: KEY_INF and colour 0 are never shown)
    }
    for (;;) {      // the root at the pixel's arrival level
      bool go[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) go[p] = d[p] <= arr[p];
      if (!(go[0] || go[1] || go[2] || go[3])) break;
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) r[p] = hook[r[p]];
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) d[p] = death[r[p]];
    }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool active = col[p] != 0u && arr[p] != 0xFFu;
      const unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
      if (todo == 0) continue;      // wave uniform
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r[p], leader);
      const unsigned long long same = __builtin_amdgcn_ballot_w64(active && r[p] == r0);
      if (lane == leader) own_add(s_key, s_cnt, tree, r0, (uint32_t)__popcll(same));
      else if (active && r[p] != r0) own_add(s_key, s_cnt, tree, r[p], 1u);
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < OWN_SLOTS; j += 256)
    if (s_cnt[j]) atomicAdd(&tree[s_key[j]].area, s_cnt[j]);
}

hipError_t tree_own_counts(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, TreeRec *tree, size_t n) {
  if (n == 0) return hipSuccess;
  // at most two thousand workgroups on a large plane (that many adds reach the surviving lake's word), 1024 pixels a step
  const size_t quads = (n + 1023) / 1024;
  const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
  k_tree_own<false><<<(unsigned)((quads + steps - 1) / steps), 256, 0, s>>>(keys, labels, death, hook, tree, n, steps, TreeStack{});
  return hipGetLastError();
}

hipError_t tree_own_counts_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, TreeRec *tree,
                                 size_t n, const TreeStack &st) {
  if (n == 0) return hipSuccess;
  if (st.plane == 0 || (st.plane & 3u) != 0 || n != (size_t)st.g * st.plane || n > 0xFFFFFFFFull) return hipErrorInvalidValue;      // (slice indices are u32 divisions)
  const size_t quads = (n + 1023) / 1024;
  const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
  k_tree_own<true><<<(unsigned)((quads + steps - 1) / steps), 256, 0, s>>>(keys, labels, death, hook, tree, n, steps, st);
  return hipGetLastError();
}

// bounds of the death levels' buckets (ws + NLEVELS + 1: NLEVELS + 1 words) and the scatter's cursors (behind them), from the counts
__global__ __launch_bounds__(NLEVELS) void k_tree_offsets(u64c *ws) {
  __shared__ u64c s_a[NLEVELS];
  const int t = threadIdx.x;
  const u64c a0 = ws[t];
  s_a[t] = a0;
  __syncthreads();
  for (int o = 1; o < NLEVELS; o <<= 1) {
    const u64c a = t >= o ? s_a[t - o] : 0ull;
    __syncthreads();
    s_a[t] += a;
    __syncthreads();
  }
  u64c *off = ws + NLEVELS + 1, *cur = off + NLEVELS + 1;
  off[t] = cur[t] = s_a[t] - a0;
  if (t == NLEVELS - 1) off[NLEVELS] = s_a[t];
}

// order[]: the dying colours by death level; a workgroup reserves once per level for its TREE_CHUNK colours
__global__ __launch_bounds__(256) void k_tree_scatter(const TreeRec *__restrict__ tree, size_t n_colours, u64c *cursor, uint32_t *order) {
  __shared__ uint32_t s_n[NLEVELS];
  __shared__ u64c s_base[NLEVELS];
  s_n[threadIdx.x] = 0;
  __syncthreads();
  uint32_t d[TREE_PER_THREAD];
#pragma unroll
  for (int k = 0; k < TREE_PER_THREAD; ++k) {
    const size_t c = (size_t)blockIdx.x * TREE_CHUNK + (size_t)k * 256 + threadIdx.x;
    d[k] = c < n_colours ? tree[c].death_level : TREE_ALIVE;
    if (d[k] != TREE_ALIVE) atomicAdd(&s_n[d[k] & (NLEVELS - 1)], 1u);
  }
  __syncthreads();
  {
    const uint32_t cnt = s_n[threadIdx.x];
    s_base[threadIdx.x] = cnt ? atomicAdd(&cursor[threadIdx.x], (u64c)cnt) : 0ull;
  }
  __syncthreads();
  s_n[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < TREE_PER_THREAD; ++k) {
    if (d[k] == TREE_ALIVE) continue;
    const uint32_t l = d[k] & (NLEVELS - 1);
    order[s_base[l] + atomicAdd(&s_n[l], 1u)] = (uint32_t)((size_t)blockIdx.x * TREE_CHUNK + (size_t)k * 256 + threadIdx.x);
  }
}

// One death level: every colour of the bucket hands its area and its leaves to its parent.  Late levels hand thousands of lakes to ONE
// parent: a wave adds up the lanes that share a parent (two rounds of leader election) before it adds, as k_fold_and_add_sd does.
// A colour that dies at level 0 never was a lake after a flood: it hands on no pixel (its seed pixel was counted for the root of
// level 0) and keeps area 1, the seed alone.
__global__ __launch_bounds__(256) void k_tree_fold(TreeRec *tree, const uint32_t *__restrict__ order, const u64c *__restrict__ range, uint32_t level) {
  const u64c first = range[0];
  const size_t n = (size_t)(range[1] - first);
  const int lane = threadIdx.x & 63;
  order += first;
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {      // uniform trip count per wave
    const size_t i = base + threadIdx.x;
    const bool active = i < n;
    const uint32_t c = active ? order[i] : 0u;
    uint32_t p = 0xFFFFFFFFu, area = 0, leaves = 0;
    if (active) {
      const TreeRec r = tree[c];
      p = r.parent; area = r.area; leaves = r.n_leaves;
      if (level == 0) tree[c].area = 1u;
    }
    unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
    for (int round = 0; round < 2 && todo != 0; ++round) {
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)p, leader);
      const bool same = active && p == p0;
      const uint32_t sa = wave_sum_u32(same ? area : 0u), sl = wave_sum_u32(same ? leaves : 0u);
      if (lane == leader) {
        if (sa) atomicAdd(&tree[p0].area, sa);
        if (sl) atomicAdd(&tree[p0].n_leaves, sl);
      }
      todo &= ~__builtin_amdgcn_ballot_w64(same);
    }
    if ((todo >> lane) & 1ull) {
      if (area) atomicAdd(&tree[p].area, area);
      if (leaves) atomicAdd(&tree[p].n_leaves, leaves);
    }
  }
}

hipError_t tree_fold(hipStream_t s, TreeRec *tree, size_t n_colours, uint32_t levels, u64c *ws, uint32_t *order) {
  if (n_colours <= 1) return hipSuccess;
  k_tree_offsets<<<1, NLEVELS, 0, s>>>(ws);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  u64c *off = ws + NLEVELS + 1;
  k_tree_scatter<<<(unsigned)((n_colours + TREE_CHUNK - 1) / TREE_CHUNK), 256, 0, s>>>(tree, n_colours, off + NLEVELS + 1, order);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  // a level's bucket is known on the device only: a fixed grid that strides (an even spread would be colours / levels per level)
  const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
  for (uint32_t l = 0; l < levels; ++l) {
    k_tree_fold<<<grid, 256, 0, s>>>(tree, order, off + l, l);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  return hipSuccess;
}

// ---- lake statistics (ws_merge_tree_stats_device) ------------------------------------------------------------
//
// What carries `area` up the tree carries any commutative per-pixel quantity: five u64 sums, a box, the smallest weight and the
// packed peak (weight << 32 | 0xFFFFFFFF - pixel: its maximum is the FIRST pixel in row-major order that holds the largest weight).
// Sums, minima and maxima of integers do not depend on the order the atomics arrive in: every record is reproducible to the bit.
// The accumulators are planes of n_colours entries (sum: w, wr, wc, r, c, peak; box: r_min, r_max, c_min, c_max, w_min), so that the
// lanes of a wave that update neighbouring colours touch neighbouring words; k_lake_write turns them into the 72-byte records.

// Own statistics: every pixel to the root of its colour at its arrival level (the walks of k_tree_own), an uncoloured pixel to
// record 0.  Around the percolation level most of the plane lands on ONE root and a pixel brings eleven atomics, not one: a lane
// first joins those of its four pixels that share a root, a wave joins the lanes that agree with its first lane, the workgroup's
// table takes the rest, and memory is touched once per root and workgroup.  The table lives across the workgroup's steps (the big
// lake keeps its slot) until a step leaves it more than half full: below the percolation level a long run meets thousands of small
// roots, and a table they have filled sends every newcomer to memory field by field; it is written out and starts again empty.
// STACKED (lake_stats_stack): labels hold every slice's own colours and the accumulator planes have n_colours = the forest's colours
// + stack.g entries.  A quad's slice is k = i0 / stack.plane (stack.plane % 4 == 0: a quad never straddles two slices, a workgroup's
// step may); its colours move to the forest's numbering before the walk, its uncoloured pixels go to entry n_colours - stack.g + k
// -- the slice's own record 0, which stands in for the root in the lane's join, the wave's and the table -- and rows, columns, the
// pixel index of the peak and the weight plane are those of the slice.
template <typename T, bool STACKED>
__global__ __launch_bounds__(256) void k_lake_own(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                  const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook, LakeWeights wt,
                                                  uint32_t W, u64c *sum, uint32_t *box, size_t n_colours, size_t n, size_t steps,
                                                  TreeStack stack) {
  __shared__ u64c s_sum[6 * LAKE_SLOTS];
  __shared__ uint32_t s_box[5 * LAKE_SLOTS], s_key[LAKE_SLOTS], s_used;
  for (int j = threadIdx.x; j < LAKE_SLOTS; j += 256) {
    s_key[j] = LAKE_EMPTY;
    lake_store(s_sum, s_box, LAKE_SLOTS, j, lake_none());
  }
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool vec = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  uint32_t flushed_at = 0;      // slots taken, over the run, when the table was last written out
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t i0 = (((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x) * 4;
    uint32_t arr[4], col[4];
    if (vec && i0 + 3 < n) {
      const u32x4_m k = *reinterpret_cast<const u32x4_m *>(keys + i0), l = *reinterpret_cast<const u32x4_m *>(labels + i0);
      arr[0] = k.x >> 24; arr[1] = k.y >> 24; arr[2] = k.z >> 24; arr[3] = k.w >> 24;
      col[0] = l.x; col[1] = l.y; col[2] = l.z; col[3] = l.w;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool in = i0 + p < n;
        arr[p] = in ? keys[i0 + p] >> 24 : 0xFFu;
        col[p] = in ? labels[i0 + p] : 0u;
      }
    }
    uint32_t slice = 0, none = 0;      // the quad's slice and where its uncoloured pixels go
    if constexpr (STACKED) {
      slice = i0 < n ? (uint32_t)i0 / stack.plane : 0u;      // (n < 2^32: lake_stats_stack)
      none = (uint32_t)n_colours - stack.g + slice;
      const uint32_t b = stack.base[slice];
#pragma unroll
      for (int p = 0; p < 4; ++p) col[p] += col[p] != 0u ? b : 0u;
    }
    uint32_t r[4], d[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool coloured = col[p] != 0u && arr[p] != 0xFFu;      // (as k_tree_own)
      r[p] = coloured ? col[p] : none;
      d[p] = coloured ? death[col[p]] : TREE_ALIVE;
    }
    for (;;) {      // the root at the pixel's arrival level, four walks side by side
      bool go[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) go[p] = d[p] <= arr[p];
      if (!(go[0] || go[1] || go[2] || go[3])) break;
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) r[p] = hook[r[p]];
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) d[p] = death[r[p]];
    }
    const uint32_t in0 = STACKED ? (uint32_t)i0 - slice * stack.plane : (uint32_t)i0;      // the quad's first pixel within its plane
    uint32_t y = i0 < n ? in0 / W : 0u, x = i0 < n ? in0 % W : 0u;      // (n < 2^32)
    LakePart part[4];
    bool live[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      live[p] = i0 + p < n;
      uint32_t v = 0u;
      if constexpr (STACKED) v = live[p] ? lake_weight_of_slice<T>(wt, slice, y, x) : 0u;
      else v = live[p] ? lake_weight<T>(wt, y, x) : 0u;
      part[p] = lake_pixel(v, y, x, in0 + (uint32_t)p);
      if (++x == W) { x = 0; ++y; }
    }
#pragma unroll
    for (int p = 1; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < p; ++q)
        if (live[p] && live[q] && r[p] == r[q]) { lake_join(part[q], part[p]); live[p] = false; }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned long long todo = __builtin_amdgcn_ballot_w64(live[p]);
      if (todo == 0) continue;      // wave uniform
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r[p], leader);
      const bool same = live[p] && r[p] == r0;
      if (__popcll(__builtin_amdgcn_ballot_w64(same)) > 1) {      // wave uniform
        const LakePart total = lake_wave_total(same ? part[p] : lake_none());
        if (lane == leader) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_colours, r0, total);
        else if (live[p] && !same) lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_colours, r[p], part[p]);
      } else if (live[p]) {
        lake_add(s_key, s_sum, s_box, &s_used, sum, box, n_colours, r[p], part[p]);
      }
    }
    __syncthreads();
    const uint32_t used = s_used;      // (nobody inserts between the two barriers: workgroup uniform)
    const bool full = used - flushed_at > LAKE_SLOTS / 2;
    if (full || st + 1 == steps) lake_flush(s_key, s_sum, s_box, sum, box, n_colours);
    if (full) flushed_at = used;
    __syncthreads();
  }
}

// One death level from 1 up: every colour of the bucket joins its record into its parent's (children die strictly before their
// parents: nobody reads a record another lane is adding to).  Lanes that share a parent are joined in the wave first, as k_tree_fold.
__global__ __launch_bounds__(256) void k_lake_fold(const TreeRec *__restrict__ tree, u64c *sum, uint32_t *box, size_t n_colours,
                                                   const uint32_t *__restrict__ order, const u64c *__restrict__ range) {
  const u64c first = range[0];
  const size_t n = (size_t)(range[1] - first);
  const int lane = threadIdx.x & 63;
  order += first;
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {      // uniform trip count per wave
    const size_t i = base + threadIdx.x;
    const bool active = i < n;
    uint32_t p = 0xFFFFFFFFu;
    LakePart part = lake_none();
    if (active) {
      const uint32_t c = order[i];
      p = tree[c].parent;
      part = lake_load(sum, box, n_colours, c);
    }
    unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
    for (int round = 0; round < 2 && todo != 0; ++round) {
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)p, leader);
      const bool same = active && p == p0;
      const unsigned long long with = __builtin_amdgcn_ballot_w64(same);
      if (__popcll(with) > 1) {      // wave uniform
        const LakePart total = lake_wave_total(same ? part : lake_none());
        if (lane == leader) lake_apply(sum, box, n_colours, p0, total);
      } else if (lane == leader) {
        lake_apply(sum, box, n_colours, p0, part);
      }
      todo &= ~with;
    }
    if ((todo >> lane) & 1ull) lake_apply(sum, box, n_colours, p, part);
  }
}

// The records.  A colour that dies at level 0 handed on nothing and was never the root of a pixel: it takes its seed pixel alone.
// STACKED: entry c of the n_colours accumulator entries is forest colour c (1 .. n_colours - stack.g - 1: the record at
// out[c + its slice], its seed pair in stacked rows) or slice k's uncoloured pixels (n_colours - stack.g + k: the record at
// out[base[k] + k]); entry 0 of the forest is nobody's.
template <typename T, bool STACKED>
__global__ __launch_bounds__(256) void k_lake_write(const TreeRec *__restrict__ tree, const uint32_t *__restrict__ seeds_rc, LakeWeights wt, uint32_t W,
                                                    const u64c *__restrict__ sum, const uint32_t *__restrict__ box, size_t n_colours, LakeRec *out,
                                                    TreeStack stack) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_colours) return;
  LakePart a = lake_load(sum, box, n_colours, c);
  size_t at = c;
  if constexpr (STACKED) {
    const size_t forest = n_colours - stack.g;
    if (c == 0) return;
    if (c >= forest) {
      const uint32_t k = (uint32_t)(c - forest);
      at = (size_t)stack.base[k] + k;
    } else {
      const uint32_t k = slice_of_colour(stack.base, stack.g, (uint32_t)c);
      at = c + k;
      const TreeRec t = tree[c];
      if (t.death_level == 0u && t.n_leaves != 0u) {
        const uint32_t y = seeds_rc[2 * (c - 1)] - k * (stack.plane / W), x = seeds_rc[2 * (c - 1) + 1];
        a = lake_pixel(lake_weight_of_slice<T>(wt, k, y, x), y, x, y * W + x);
      }
    }
  } else if (c != 0) {
    const TreeRec t = tree[c];
    if (t.death_level == 0u && t.n_leaves != 0u) {
      const uint32_t y = seeds_rc[2 * (c - 1)], x = seeds_rc[2 * (c - 1) + 1];
      a = lake_pixel(lake_weight<T>(wt, y, x), y, x, y * W + x);
    }
  }
  out[at] = LakeRec{a.w, a.wr, a.wc, a.r, a.c, a.r_min, a.r_max, a.c_min, a.c_max, a.w_min, (uint32_t)(a.peak >> 32),
                    0xFFFFFFFFu - (uint32_t)a.peak, 0u};
}

hipError_t lake_stats(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, const TreeRec *tree,
                      const uint32_t *seeds_rc, size_t n_colours, uint32_t levels, const u64c *ws, const uint32_t *order, const LakeWeights &wt, int h,
                      int w, void *acc, LakeRec *out) {
  if (n_colours == 0) return hipSuccess;
  const size_t n = (size_t)h * (size_t)w;
  if (n > 0xFFFFFFFFull || (reinterpret_cast<uintptr_t>(acc) & 7u) != 0) return hipErrorInvalidValue;      // (rows and columns are u32 divisions)
  u64c *sum = (u64c *)acc;
  uint32_t *box = (uint32_t *)(sum + 6 * n_colours);
  const unsigned per_colour = (unsigned)((n_colours + 255) / 256);
  k_lake_init<<<per_colour, 256, 0, s>>>(sum, box, n_colours);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (n) {      // the grid of tree_own_counts: at most two thousand workgroups, 1024 pixels a step
    const size_t quads = (n + 1023) / 1024;
    const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
    const unsigned grid = (unsigned)((quads + steps - 1) / steps);
    if (wt.u16) k_lake_own<uint16_t, false><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_colours, n, steps, TreeStack{});
    else k_lake_own<uint8_t, false><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_colours, n, steps, TreeStack{});
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_colours > 1) {      // (tree_fold built order[] and its bounds under the same condition)
    const u64c *off = ws + NLEVELS + 1;
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
    for (uint32_t l = 1; l < levels; ++l) {
      k_lake_fold<<<grid, 256, 0, s>>>(tree, sum, box, n_colours, order, off + l);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  if (wt.u16) k_lake_write<uint16_t, false><<<per_colour, 256, 0, s>>>(tree, seeds_rc, wt, (uint32_t)w, sum, box, n_colours, out, TreeStack{});
  else k_lake_write<uint8_t, false><<<per_colour, 256, 0, s>>>(tree, seeds_rc, wt, (uint32_t)w, sum, box, n_colours, out, TreeStack{});
  return hipGetLastError();
}

hipError_t lake_stats_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                            const TreeRec *forest, const uint32_t *stacked_rc, size_t n_colours, uint32_t levels, const u64c *ws,
                            const uint32_t *order, const LakeWeights &wt, const TreeStack &st, int w, void *acc, LakeRec *out) {
  if (n_colours == 0 || st.g == 0) return hipSuccess;
  const size_t n = (size_t)st.g * st.plane, n_acc = n_colours + st.g;      // every slice's record 0 behind the forest's colours
  // (slices, rows and columns are u32 divisions; a quad must not straddle two slices, a row must not either)
  if (n > 0xFFFFFFFFull || n_acc > 0xFFFFFFFFull || st.plane == 0 || (st.plane & 3u) != 0 || w <= 0 || st.plane % (uint32_t)w != 0 ||
      (reinterpret_cast<uintptr_t>(acc) & 7u) != 0)
    return hipErrorInvalidValue;
  u64c *sum = (u64c *)acc;
  uint32_t *box = (uint32_t *)(sum + 6 * n_acc);
  const unsigned per_entry = (unsigned)((n_acc + 255) / 256);
  k_lake_init<<<per_entry, 256, 0, s>>>(sum, box, n_acc);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  {      // the grid of tree_own_counts_stack
    const size_t quads = (n + 1023) / 1024;
    const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
    const unsigned grid = (unsigned)((quads + steps - 1) / steps);
    if (wt.u16) k_lake_own<uint16_t, true><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_acc, n, steps, st);
    else k_lake_own<uint8_t, true><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, (uint32_t)w, sum, box, n_acc, n, steps, st);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (n_colours > 1) {      // ONE launch per level for the whole stack: parents are the forest's, the planes are n_acc long
    const u64c *off = ws + NLEVELS + 1;
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
    for (uint32_t l = 1; l < levels; ++l) {
      k_lake_fold<<<grid, 256, 0, s>>>(forest, sum, box, n_acc, order, off + l);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  if (wt.u16) k_lake_write<uint16_t, true><<<per_entry, 256, 0, s>>>(forest, stacked_rc, wt, (uint32_t)w, sum, box, n_acc, out, st);
  else k_lake_write<uint8_t, true><<<per_entry, 256, 0, s>>>(forest, stacked_rc, wt, (uint32_t)w, sum, box, n_acc, out, st);
  return hipGetLastError();
}

// ---- lake shapes (ws_merge_tree_shapes_device) -------------------------------------------------------------
//
// The second moments of every lake: six exact 128-bit sums a record, carried as twelve carry-less u64 limbs (ws_shape_part.hpp), in
// passes of their own after lake_stats over the same death[] / hook[] forest and the same order[] buckets.  Sums of integers do not
// depend on the order the atomics arrive in: every record is reproducible to the bit.

// Own shapes: k_lake_own's grid, loads, walks and three joins (the quad's pixels that share a root, the lanes that agree with the
// wave's first lane, the workgroup's table keyed by root) with a ShapePart for a LakePart; an uncoloured pixel goes to record 0.
// FLAT: both sides of the plane are below 65 536 (shape_wave_total).
// STACKED (lake_shapes_stack), as k_lake_own's: labels hold every slice's own colours and the accumulator planes have n_colours = the
// forest's colours + stack.g entries.  A quad's slice is k = i0 / stack.plane (stack.plane % 4 == 0: a quad never straddles two
// slices, a workgroup's step may); its colours move to the forest's numbering before the walk, its uncoloured pixels go to entry
// n_colours - stack.g + k -- the slice's own record 0, which stands in for the root in the lane's join, the wave's and the table --
// and rows, columns and the weight plane are those of the slice.  FLAT is then about the sides of ONE slice.
template <typename T, bool FLAT, bool STACKED>
__global__ __launch_bounds__(256) void k_shape_own(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ labels,
                                                   const uint32_t *__restrict__ death, const uint32_t *__restrict__ hook, LakeWeights wt,
                                                   uint32_t W, u64c *acc, size_t n_colours, size_t n, size_t steps,
                                                   TreeStack stack) {
  __shared__ u64c s_acc[SHAPE_LIMBS * SHAPE_SLOTS];
  __shared__ uint32_t s_key[SHAPE_SLOTS], s_used;
  for (int j = threadIdx.x; j < SHAPE_SLOTS; j += 256) {
    s_key[j] = LAKE_EMPTY;
    shape_store(s_acc, SHAPE_SLOTS, j, shape_none());
  }
  if (threadIdx.x == 0) s_used = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const bool vec = ((reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(labels)) & 15u) == 0;
  uint32_t flushed_at = 0;      // slots taken, over the run, when the table was last written out
  for (size_t st = 0; st < steps; ++st) {      // workgroup uniform
    const size_t i0 = (((size_t)blockIdx.x * steps + st) * 256 + threadIdx.x) * 4;
    uint32_t arr[4], col[4];
    if (vec && i0 + 3 < n) {
      const u32x4_m k = *reinterpret_cast<const u32x4_m *>(keys + i0), l = *reinterpret_cast<const u32x4_m *>(labels + i0);
      arr[0] = k.x >> 24; arr[1] = k.y >> 24; arr[2] = k.z >> 24; arr[3] = k.w >> 24;
      col[0] = l.x; col[1] = l.y; col[2] = l.z; col[3] = l.w;
    } else {
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        const bool in = i0 + p < n;
        arr[p] = in ? keys[i0 + p] >> 24 : 0xFFu;
        col[p] = in ? labels[i0 + p] : 0u;
      }
    }
    uint32_t slice = 0, none = 0;      // the quad's slice and where its uncoloured pixels go
    if constexpr (STACKED) {
      slice = i0 < n ? (uint32_t)i0 / stack.plane : 0u;      // (n < 2^32: lake_shapes_stack)
      none = (uint32_t)n_colours - stack.g + slice;
      const uint32_t b = stack.base[slice];
#pragma unroll
      for (int p = 0; p < 4; ++p) col[p] += col[p] != 0u ? b : 0u;
    }
    uint32_t r[4], d[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const bool coloured = col[p] != 0u && arr[p] != 0xFFu;      // (as k_tree_own)
      r[p] = coloured ? col[p] : none;
      d[p] = coloured ? death[col[p]] : TREE_ALIVE;
    }
    for (;;) {      // the root at the pixel's arrival level, four walks side by side
      bool go[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) go[p] = d[p] <= arr[p];
      if (!(go[0] || go[1] || go[2] || go[3])) break;
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) r[p] = hook[r[p]];
#pragma unroll
      for (int p = 0; p < 4; ++p) if (go[p]) d[p] = death[r[p]];
    }
    const uint32_t in0 = STACKED ? (uint32_t)i0 - slice * stack.plane : (uint32_t)i0;      // the quad's first pixel within its plane
    uint32_t y = i0 < n ? in0 / W : 0u, x = i0 < n ? in0 % W : 0u;      // (n < 2^32)
    ShapePart part[4];
    bool live[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      live[p] = i0 + p < n;
      uint32_t v = 0u;
      if constexpr (STACKED) v = live[p] ? lake_weight_of_slice<T>(wt, slice, y, x) : 0u;
      else v = live[p] ? lake_weight<T>(wt, y, x) : 0u;
      part[p] = shape_pixel(v, y, x);
      if (++x == W) { x = 0; ++y; }
    }
#pragma unroll
    for (int p = 1; p < 4; ++p)
#pragma unroll
      for (int q = 0; q < p; ++q)
        if (live[p] && live[q] && r[p] == r[q]) { shape_join(part[q], part[p]); live[p] = false; }
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const unsigned long long todo = __builtin_amdgcn_ballot_w64(live[p]);
      if (todo == 0) continue;      // wave uniform
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t r0 = (uint32_t)__builtin_amdgcn_readlane((int)r[p], leader);
      const bool same = live[p] && r[p] == r0;
      if (__popcll(__builtin_amdgcn_ballot_w64(same)) > 1) {      // wave uniform
        const ShapePart total = shape_wave_total<FLAT>(same ? part[p] : shape_none());
        if (lane == leader) shape_add(s_key, s_acc, &s_used, acc, n_colours, r0, total);
        else if (live[p] && !same) shape_add(s_key, s_acc, &s_used, acc, n_colours, r[p], part[p]);
      } else if (live[p]) {
        shape_add(s_key, s_acc, &s_used, acc, n_colours, r[p], part[p]);
      }
    }
    __syncthreads();
    const uint32_t used = s_used;      // (nobody inserts between the two barriers: workgroup uniform)
    const bool full = used - flushed_at > SHAPE_SLOTS / 2;
    if (full || st + 1 == steps) shape_flush(s_key, s_acc, acc, n_colours);
    if (full) flushed_at = used;
    __syncthreads();
  }
}

// One death level from 1 up: every colour of the bucket joins its limbs into its parent's (children die strictly before their
// parents: nobody reads a limb another lane is adding to).  Lanes that share a parent are joined in the wave first, as k_lake_fold.
__global__ __launch_bounds__(256) void k_shape_fold(const TreeRec *__restrict__ tree, u64c *acc, size_t n_colours,
                                                    const uint32_t *__restrict__ order, const u64c *__restrict__ range) {
  const u64c first = range[0];
  const size_t n = (size_t)(range[1] - first);
  const int lane = threadIdx.x & 63;
  order += first;
  for (size_t base = (size_t)blockIdx.x * 256; base < n; base += (size_t)gridDim.x * 256) {      // uniform trip count per wave
    const size_t i = base + threadIdx.x;
    const bool active = i < n;
    uint32_t p = 0xFFFFFFFFu;
    ShapePart part = shape_none();
    if (active) {
      const uint32_t c = order[i];
      p = tree[c].parent;
      part = shape_load(acc, n_colours, c);
    }
    unsigned long long todo = __builtin_amdgcn_ballot_w64(active);
    for (int round = 0; round < 2 && todo != 0; ++round) {
      const int leader = (int)__builtin_ctzll(todo);
      const uint32_t p0 = (uint32_t)__builtin_amdgcn_readlane((int)p, leader);
      const bool same = active && p == p0;
      const unsigned long long with = __builtin_amdgcn_ballot_w64(same);
      if (__popcll(with) > 1) {      // wave uniform
        const ShapePart total = shape_wave_total<false>(same ? part : shape_none());
        if (lane == leader) shape_apply(acc, n_colours, p0, total);
      } else if (lane == leader) {
        shape_apply(acc, n_colours, p0, part);
      }
      todo &= ~with;
    }
    if ((todo >> lane) & 1ull) shape_apply(acc, n_colours, p, part);
  }
}

// The records: every pair of limbs normalised to (low, high) once.  A colour that dies at level 0 handed on nothing and was never
// the root of a pixel: it takes its seed pixel alone (as k_lake_write).
// STACKED, as k_lake_write's: entry c of the n_colours accumulator entries is forest colour c (1 .. n_colours - stack.g - 1: the
// record at out[c + its slice], its seed pair in stacked rows of W columns) or slice k's uncoloured pixels (n_colours - stack.g + k:
// the record at out[base[k] + k]); entry 0 of the forest is nobody's.
template <typename T, bool STACKED>
__global__ __launch_bounds__(256) void k_shape_write(const TreeRec *__restrict__ tree, const uint32_t *__restrict__ seeds_rc, LakeWeights wt,
                                                     const u64c *__restrict__ acc, size_t n_colours, ShapeRec *out, uint32_t W,
                                                     TreeStack stack) {
  const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= n_colours) return;
  ShapePart a = shape_load(acc, n_colours, c);
  size_t at = c;
  if constexpr (STACKED) {
    const size_t forest = n_colours - stack.g;
    if (c == 0) return;
    if (c >= forest) {
      const uint32_t k = (uint32_t)(c - forest);
      at = (size_t)stack.base[k] + k;
    } else {
      const uint32_t k = slice_of_colour(stack.base, stack.g, (uint32_t)c);
      at = c + k;
      const TreeRec t = tree[c];
      if (t.death_level == 0u && t.n_leaves != 0u) {
        const uint32_t y = seeds_rc[2 * (c - 1)] - k * (stack.plane / W), x = seeds_rc[2 * (c - 1) + 1];
        a = shape_pixel(lake_weight_of_slice<T>(wt, k, y, x), y, x);
      }
    }
  } else if (c != 0) {
    const TreeRec t = tree[c];
    if (t.death_level == 0u && t.n_leaves != 0u) {
      const uint32_t y = seeds_rc[2 * (c - 1)], x = seeds_rc[2 * (c - 1) + 1];
      a = shape_pixel(lake_weight<T>(wt, y, x), y, x);
    }
  }
  ShapeRec rec;
#pragma unroll
  for (int k = 0; k < 6; ++k) shape_normal(a, k, &rec.s[k][0], &rec.s[k][1]);
  out[at] = rec;
}

// the grid of k_lake_own over n pixels and the launch of the instantiation the weights, the sides of ONE plane and the form ask for
template <bool STACKED>
hipError_t shape_own_launch(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                            const LakeWeights &wt, bool flat, uint32_t w, u64c *acc, size_t n_entries, size_t n, const TreeStack &st) {
  const size_t quads = (n + 1023) / 1024;
  const size_t steps = std::max<size_t>((quads + 2047) / 2048, 1);
  const unsigned grid = (unsigned)((quads + steps - 1) / steps);
  if (wt.u16) {
    if (flat) k_shape_own<uint16_t, true, STACKED><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, w, acc, n_entries, n, steps, st);
    else k_shape_own<uint16_t, false, STACKED><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, w, acc, n_entries, n, steps, st);
  } else {
    if (flat) k_shape_own<uint8_t, true, STACKED><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, w, acc, n_entries, n, steps, st);
    else k_shape_own<uint8_t, false, STACKED><<<grid, 256, 0, s>>>(keys, labels, death, hook, wt, w, acc, n_entries, n, steps, st);
  }
  return hipGetLastError();
}

hipError_t lake_shapes(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, const TreeRec *tree,
                       const uint32_t *seeds_rc, size_t n_colours, uint32_t levels, const u64c *ws, const uint32_t *order, const LakeWeights &wt, int h,
                       int w, void *acc_bytes, ShapeRec *out) {
  if (n_colours == 0) return hipSuccess;
  const size_t n = (size_t)h * (size_t)w;
  if (n > 0xFFFFFFFFull || ((reinterpret_cast<uintptr_t>(acc_bytes) | reinterpret_cast<uintptr_t>(out)) & 7u) != 0) return hipErrorInvalidValue;
  u64c *acc = (u64c *)acc_bytes;
  hipError_t e = hipMemsetAsync(acc, 0, n_colours * SHAPE_ACC_BYTES, s);      // the identity of the fold is twelve zeros
  if (e != hipSuccess) return e;
  if (n && (e = shape_own_launch<false>(s, keys, labels, death, hook, wt, h < 65536 && w < 65536, (uint32_t)w, acc, n_colours, n, TreeStack{})) != hipSuccess)
    return e;
  if (n_colours > 1) {      // (tree_fold built order[] and its bounds under the same condition)
    const u64c *off = ws + NLEVELS + 1;
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
    for (uint32_t l = 1; l < levels; ++l) {
      k_shape_fold<<<grid, 256, 0, s>>>(tree, acc, n_colours, order, off + l);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  const unsigned per_colour = (unsigned)((n_colours + 255) / 256);
  if (wt.u16) k_shape_write<uint16_t, false><<<per_colour, 256, 0, s>>>(tree, seeds_rc, wt, acc, n_colours, out, (uint32_t)w, TreeStack{});
  else k_shape_write<uint8_t, false><<<per_colour, 256, 0, s>>>(tree, seeds_rc, wt, acc, n_colours, out, (uint32_t)w, TreeStack{});
  return hipGetLastError();
}

hipError_t lake_shapes_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                             const TreeRec *forest, const uint32_t *stacked_rc, size_t n_colours, uint32_t levels, const u64c *ws,
                             const uint32_t *order, const LakeWeights &wt, const TreeStack &st, int w, void *acc_bytes, ShapeRec *out) {
  if (n_colours == 0 || st.g == 0) return hipSuccess;
  const size_t n = (size_t)st.g * st.plane, n_acc = n_colours + st.g;      // every slice's record 0 behind the forest's colours
  // (slices, rows and columns are u32 divisions; a quad must not straddle two slices, a row must not either)
  if (n > 0xFFFFFFFFull || n_acc > 0xFFFFFFFFull || st.plane == 0 || (st.plane & 3u) != 0 || w <= 0 || st.plane % (uint32_t)w != 0 ||
      ((reinterpret_cast<uintptr_t>(acc_bytes) | reinterpret_cast<uintptr_t>(out)) & 7u) != 0)
    return hipErrorInvalidValue;
  u64c *acc = (u64c *)acc_bytes;
  hipError_t e = hipMemsetAsync(acc, 0, n_acc * SHAPE_ACC_BYTES, s);      // the identity of the fold is twelve zeros
  if (e != hipSuccess) return e;
  // FLAT from the sides of a slice: rows restart in every slice, the stacked height g * ph never enters a term
  const bool flat = st.plane / (uint32_t)w < 65536u && w < 65536;
  if ((e = shape_own_launch<true>(s, keys, labels, death, hook, wt, flat, (uint32_t)w, acc, n_acc, n, st)) != hipSuccess) return e;
  if (n_colours > 1) {      // ONE launch per level for the whole stack: parents are the forest's, the planes are n_acc long
    const u64c *off = ws + NLEVELS + 1;
    const unsigned grid = (unsigned)std::min<size_t>(std::max<size_t>(n_colours / (256 * 64), 1), 128);
    for (uint32_t l = 1; l < levels; ++l) {
      k_shape_fold<<<grid, 256, 0, s>>>(forest, acc, n_acc, order, off + l);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  const unsigned per_entry = (unsigned)((n_acc + 255) / 256);
  if (wt.u16) k_shape_write<uint16_t, true><<<per_entry, 256, 0, s>>>(forest, stacked_rc, wt, acc, n_acc, out, (uint32_t)w, st);
  else k_shape_write<uint8_t, true><<<per_entry, 256, 0, s>>>(forest, stacked_rc, wt, acc, n_acc, out, (uint32_t)w, st);
  return hipGetLastError();
}

// ---- the merge tree of a stack, slice by slice ------------------------------------------------------------------------------------
// The forest's tree records (ws_merge_tree_batch_device) into the caller's slice-major layout in the slices' own colours: record c
// of the forest (1 .. n_seeds) is record c - base[k] of its slice k, at out[c + k] (every slice before it owns one record 0), its
// parent -- same slice: no pair crosses a slice border -- less the slice's base.  Thread n_seeds + k writes slice k's record 0 at
// out[base[k] + k]: the pixels of its plane that no level up to the last coloured (hist: k_slice_arrivals').
__global__ __launch_bounds__(256) void k_tree_unstack(const TreeRec *__restrict__ forest, size_t n_seeds, const uint32_t *__restrict__ base, uint32_t g,
                                                      const u64c *__restrict__ hist, uint32_t levels, uint32_t plane, TreeRec *out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n_seeds) {
    const uint32_t c = (uint32_t)i + 1u, k = slice_of_colour(base, g, c);
    TreeRec r = forest[c];
    if (r.death_level != TREE_ALIVE) r.parent -= base[k];
    out[(size_t)c + k] = r;
  } else if (i < n_seeds + g) {
    const uint32_t k = (uint32_t)(i - n_seeds);
    u64c arrived = 0;
    for (uint32_t l = 0; l < levels; ++l) arrived += hist[(size_t)k * NLEVELS + l];
    out[(size_t)base[k] + k] = TreeRec{0u, TREE_ALIVE, (uint32_t)((u64c)plane - arrived), 0u};
  }
}

hipError_t tree_unstack(hipStream_t s, const TreeRec *forest, size_t n_seeds, const uint32_t *base, size_t g, const u64c *hist, uint32_t levels,
                        size_t plane, TreeRec *out) {
  if (g == 0) return hipSuccess;
  if (levels > (uint32_t)NLEVELS || plane > 0xFFFFFFFFull || g > 0xFFFFFFFFull) return hipErrorInvalidValue;
  k_tree_unstack<<<(unsigned)((n_seeds + g + 255) / 256), 256, 0, s>>>(forest, n_seeds, base, (uint32_t)g, hist, levels, (uint32_t)plane, out);
  return hipGetLastError();
}

}  // namespace wsk
