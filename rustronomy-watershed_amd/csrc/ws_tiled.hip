// ws_tiled.hip -- several GPUs behind one call: ws_group_* and every ws_*_tiled* / ws_segment_batch_* entry point.
//
// The reference's drivers are ONE address space (lib.rs:1689-1748: a rayon loop over the windows of one array); what
// stands in for that across devices is a group of RANKS, each a ws_ctx on one device, running the block steps of
// ws_block_api.hip.  The file, top to bottom:
//
//   the cut         ws_tile_plan.hpp (plain C++): a field in py x px tiles, row blocks being px = 1 -- a rank's place, the
//                   gather layout, the image window under edge correction, the dealing of a host seed list
//   the group       RCCL resolved at run time, a breakable barrier, Rank (a context and its buffers), ws_group
//   the exchange    struct Exchange: swap + copy_ring_in (the halo), reduce (one word, ONE host read), gather (a table on every
//                   rank), gather_owned (what the ranks own -> rank 0's whole plane).  LOCAL: the ranks are host threads, the steps
//                   stream-ordered copies behind the barrier.  RCCL: one rank per process; ncclSend / Recv, AllReduce, AllGather
//   rank programs   tiled_rank (row blocks: the fast form or the general one, by a vote), tiled2d_rank (tiles), flood (either, or the
//                   single-device transform for a group of one); until_quiet is the round loop they share
//   flood_to_root   the flood on all ranks, the stamps and labels of the whole field gathered on rank 0: what the lists and the
//                   tree are made from
//   entry points    check_tiled_call (the one argument check), then the device forms: a flood, or flood_to_root and an arrival form
//   the host job    TiledHostJob and its stages (check, upload_block, flood, a delivery) behind the host-buffer forms
//   batches         ws_segment_batch_group / _host: independent slices, no exchange
#include "ws_ctx.hpp"
#include "ws_tile_plan.hpp"

#include <rccl/rccl.h>

#include <dlfcn.h>

#include <condition_variable>
#include <mutex>
#include <thread>
#include <type_traits>

using namespace wsapi;

namespace {

// ---- RCCL, resolved at run time -----------------------------------------------------------------------------------------
struct RcclApi {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*CommAbort)(ncclComm_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  ncclResult_t (*GroupStart)() = nullptr;
  ncclResult_t (*GroupEnd)() = nullptr;
  ncclResult_t (*Send)(const void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*Recv)(void *, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  std::string why;
};

RcclApi *rccl() {
  static RcclApi api;
  static std::once_flag once;
  std::call_once(once, [] {
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      api.lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (api.lib) break;
    }
    if (!api.lib) { api.why = std::string("dlopen(librccl.so): ") + (dlerror() ? dlerror() : "not found"); return; }
    bool ok = true;
    auto sym = [&](const char *n) { void *p = dlsym(api.lib, n); if (!p) { ok = false; api.why = std::string("librccl.so lacks ") + n; } return p; };
    api.GetUniqueId = (decltype(api.GetUniqueId))sym("ncclGetUniqueId");
    api.CommInitRank = (decltype(api.CommInitRank))sym("ncclCommInitRank");
    api.CommDestroy = (decltype(api.CommDestroy))sym("ncclCommDestroy");
    api.CommAbort = (decltype(api.CommAbort))sym("ncclCommAbort");
    api.GetErrorString = (decltype(api.GetErrorString))sym("ncclGetErrorString");
    api.GroupStart = (decltype(api.GroupStart))sym("ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))sym("ncclGroupEnd");
    api.Send = (decltype(api.Send))sym("ncclSend");
    api.Recv = (decltype(api.Recv))sym("ncclRecv");
    api.AllReduce = (decltype(api.AllReduce))sym("ncclAllReduce");
    api.AllGather = (decltype(api.AllGather))sym("ncclAllGather");
    if (!ok) { dlclose(api.lib); api.lib = nullptr; }
  });
  return &api;
}

// ---- a thread barrier that can be broken (a rank that fails must not leave the others waiting) ------------------------------
struct Barrier {
  std::mutex m;
  std::condition_variable cv;
  int n = 1, count = 0;
  uint64_t gen = 0;
  bool broken = false;
  bool wait() {
    std::unique_lock<std::mutex> l(m);
    if (broken) return false;
    const uint64_t g = gen;
    if (++count == n) { count = 0; ++gen; cv.notify_all(); return true; }
    cv.wait(l, [&] { return gen != g || broken; });
    return !broken;
  }
  void abort() { std::lock_guard<std::mutex> l(m); broken = true; cv.notify_all(); }
  void reset(int ranks) { std::lock_guard<std::mutex> l(m); n = ranks; count = 0; broken = false; }
};

struct Grow {      // a device buffer that only ever grows, and frees itself (on the device that is current then)
  void *p = nullptr;
  size_t cap = 0;
  Grow() = default;
  Grow(Grow &&o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  Grow &operator=(Grow &&o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); return *this; }
  ~Grow() { if (p) (void)hipFree(p); }
};

// a rank's buffers: a member added here is freed by ws_group_destroy without being named again
struct RankBuffers {
  Grow keys, labels, recv, rows, table, parent, img, seeds, colours, out64, cols, full_keys, full_labels, weight;
};

// one rank driven by this process
struct Rank : RankBuffers {
  int rank = 0, device = 0;
  ws_ctx *ctx = nullptr;
  uint32_t *flag = nullptr;           // device: 4 words (the exchange loop's stop word; reduce scratch)
  uint32_t *flag_host = nullptr;      // pinned mirror
  // what the LOCAL exchange steps read from their neighbours (published before the barrier)
  const uint32_t *pub_first = nullptr, *pub_last = nullptr, *pub_send = nullptr, *pub_cols = nullptr;
  uint32_t pub_word = 0;
};

}  // namespace

struct ws_group {
  bool is_rccl = false;
  int world = 1, first_local = 0;
  std::vector<Rank> ranks;      // the local ones
  Barrier barrier;
  ncclComm_t comm = nullptr;
  std::mutex err_m;
  std::string err;
};

namespace {

int gfail(ws_group *g, int code, const std::string &what) {
  if (g) { std::lock_guard<std::mutex> l(g->err_m); if (g->err.empty() || code != WS_ERR_HIP) g->err = what; }
  return code;
}

#define G_HIP(g, call)                                                                                          \
  do {                                                                                                          \
    hipError_t e_ = (call);                                                                                     \
    if (e_ != hipSuccess) return gfail((g), e_ == hipErrorOutOfMemory ? WS_ERR_OOM : WS_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)
#define G_NCCL(g, call)                                                                                         \
  do {                                                                                                          \
    ncclResult_t r_ = (call);                                                                                   \
    if (r_ != ncclSuccess) return gfail((g), WS_ERR_RCCL, std::string(#call) + ": " + rccl()->GetErrorString(r_)); \
  } while (0)
// a ws_* call on the rank's own context: its message travels to the group
#define G_WS(g, rk, call)                                                                                       \
  do {                                                                                                          \
    const int rc_ = (call);                                                                                     \
    if (rc_ != WS_OK) return gfail((g), rc_, std::string("rank ") + std::to_string((rk).rank) + ": " + #call + ": " + ws_last_error((rk).ctx)); \
  } while (0)

// the status of a ws_* call on a rank's own context, its message carried to the group (WS_ERR_CAPACITY included: the caller reads n_lakes)
int gfail_if(ws_group *g, const Rank &rk, int rc) {
  return rc == WS_OK ? WS_OK : gfail(g, rc, std::string("rank ") + std::to_string(rk.rank) + ": " + ws_last_error(rk.ctx));
}

int grow(ws_group *g, Grow &b, size_t bytes) {
  if (bytes <= b.cap) return WS_OK;
  b = Grow();
  const size_t want = bytes + (bytes >> 4) + 256;
  hipError_t e = hipMalloc(&b.p, want);
  if (e != hipSuccess) { b.p = nullptr; return gfail(g, WS_ERR_OOM, std::string("hipMalloc: ") + hipGetErrorString(e)); }
  b.cap = want;
  return WS_OK;
}

// ---- the three exchange steps ------------------------------------------------------------------------------------------
struct Exchange {
  ws_group *g;
  Rank &me;
  hipStream_t stream() const { return me.ctx->stream; }

  Rank *local(int rank) const { return &g->ranks[(size_t)(rank - g->first_local)]; }

  // A held plane (t.h x t.w) of a field cut into tiles: sends my first / last OWNED row and column, receives the neighbours'
  // into me.recv: [0, w) from above, [w, 2w) from below, [2w, 2w + h) from the left, [2w + h, 2w + 2h) from the right.  (Rows
  // are contiguous; columns are packed into me.cols first.  The four corner cells of the halo ring are nobody's neighbours in
  // a 4-connected stencil.)  Row blocks have no left or right neighbour: nothing is packed, and nothing waits for the packing.
  int swap(const uint32_t *plane, const TilePlace &t) {
    const size_t h = t.h, w = t.w;
    const bool up = t.nb[0] >= 0, down = t.nb[1] >= 0, left = t.nb[2] >= 0, right = t.nb[3] >= 0;
    const uint32_t *first = plane + (up ? w : 0), *last = plane + (h - 1 - (down ? 1 : 0)) * w;
    uint32_t *recv = (uint32_t *)me.recv.p, *cols = (uint32_t *)me.cols.p;
    if (left || right) G_HIP(g, block_pack_cols(stream(), plane, h, w, left ? 1 : 0, w - 1 - (right ? 1 : 0), cols));
    if (g->is_rccl) {
      RcclApi *n = rccl();
      G_NCCL(g, n->GroupStart());
      if (up) { G_NCCL(g, n->Send(first, w, ncclUint32, t.nb[0], g->comm, stream())); G_NCCL(g, n->Recv(recv, w, ncclUint32, t.nb[0], g->comm, stream())); }
      if (down) { G_NCCL(g, n->Send(last, w, ncclUint32, t.nb[1], g->comm, stream())); G_NCCL(g, n->Recv(recv + w, w, ncclUint32, t.nb[1], g->comm, stream())); }
      if (left) { G_NCCL(g, n->Send(cols, h, ncclUint32, t.nb[2], g->comm, stream())); G_NCCL(g, n->Recv(recv + 2 * w, h, ncclUint32, t.nb[2], g->comm, stream())); }
      if (right) { G_NCCL(g, n->Send(cols + h, h, ncclUint32, t.nb[3], g->comm, stream())); G_NCCL(g, n->Recv(recv + 2 * w + h, h, ncclUint32, t.nb[3], g->comm, stream())); }
      G_NCCL(g, n->GroupEnd());
      return WS_OK;
    }
    // (every rank's plane is complete in memory: the block steps end with a wait for their stream)
    if (left || right) G_HIP(g, hipStreamSynchronize(stream()));      // my packed columns are complete before anyone copies them
    me.pub_first = first; me.pub_last = last; me.pub_cols = cols;
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    if (up) G_HIP(g, hipMemcpyAsync(recv, local(t.nb[0])->pub_last, w * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
    if (down) G_HIP(g, hipMemcpyAsync(recv + w, local(t.nb[1])->pub_first, w * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
    // (tiles of one tile row have the same rows: the neighbour's packed runs are h words long, its LAST column first comes second)
    if (left) G_HIP(g, hipMemcpyAsync(recv + 2 * w, local(t.nb[2])->pub_cols + h, h * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
    if (right) G_HIP(g, hipMemcpyAsync(recv + 2 * w + h, local(t.nb[3])->pub_cols, h * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
    G_HIP(g, hipStreamSynchronize(stream()));
    // nobody goes on to rewrite its plane while a neighbour still reads it
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    return WS_OK;
  }

  // what swap received, into the halo ring of the plane
  int copy_ring_in(uint32_t *plane, const TilePlace &t) {
    const size_t h = t.h, w = t.w;
    const uint32_t *recv = (const uint32_t *)me.recv.p;
    if (t.nb[0] >= 0) G_HIP(g, hipMemcpyAsync(plane, recv, w * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
    if (t.nb[1] >= 0) G_HIP(g, hipMemcpyAsync(plane + (h - 1) * w, recv + w, w * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
    // (columns after rows: a halo column's first / last cell is a corner of the ring, read by nobody)
    if (t.nb[2] >= 0 || t.nb[3] >= 0)
      G_HIP(g, block_unpack_cols(stream(), plane, h, w, t.nb[2] >= 0 ? recv + 2 * w : nullptr, t.nb[3] >= 0 ? recv + 2 * w + h : nullptr));
    return WS_OK;
  }

  // every rank's OWNED rows of a field in row blocks (`own`: its first owned row) -> rank 0's whole plane (`full`, rank 0 only):
  // one message per rank and plane, unpacked.  Returns with rank 0's copies complete.
  int gather_rows(const uint32_t *own, const GatherLayout &l, uint32_t *full) {
    const size_t w = l.place[0].w;
    const TilePlace &t = l.place[(size_t)me.rank];
    if (g->is_rccl) {
      RcclApi *n = rccl();
      G_NCCL(g, n->GroupStart());
      if (me.rank != 0) {
        if (t.own_h() && w) G_NCCL(g, n->Send(own, t.own_h() * w, ncclUint32, 0, g->comm, stream()));
      } else {
        for (int r = 1; r < g->world; ++r) {
          const TilePlace &p = l.place[(size_t)r];
          if (p.own_h() && w) G_NCCL(g, n->Recv(full + p.r0 * w, p.own_h() * w, ncclUint32, r, g->comm, stream()));
        }
      }
      G_NCCL(g, n->GroupEnd());
      if (me.rank == 0 && t.own_h() && w) G_HIP(g, hipMemcpyAsync(full + t.r0 * w, own, t.own_h() * w * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
      G_HIP(g, hipStreamSynchronize(stream()));
      return WS_OK;
    }
    me.pub_send = own;      // (every rank's plane is complete in memory: the steps before end with a wait for their stream)
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    if (me.rank == 0) {
      for (int r = 0; r < g->world; ++r) {
        const TilePlace &p = l.place[(size_t)r];
        if (p.own_h() && w) G_HIP(g, hipMemcpyAsync(full + p.r0 * w, local(r)->pub_send, p.own_h() * w * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
      }
      G_HIP(g, hipStreamSynchronize(stream()));
    }
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    return WS_OK;
  }

  // ... of a field cut in both directions: every rank's OWNED rectangle of its held plane -> rank 0's whole plane.  A rectangle
  // travels packed (me.rows); rank 0 parks what it receives in me.table and places every rectangle with a 2-D copy.  Returns
  // with rank 0's copies complete.
  int gather_rect(const uint32_t *plane, const GatherLayout &l, size_t field_w, uint32_t *full) {
    const TilePlace &t = l.place[(size_t)me.rank];
    const size_t oh = t.own_h(), ow = t.own_w();
    int rc;
    if ((rc = grow(g, me.rows, std::max<size_t>(oh * ow, 1) * sizeof(uint32_t)))) return rc;
    if (oh * ow)
      G_HIP(g, hipMemcpy2DAsync(me.rows.p, ow * sizeof(uint32_t), plane + t.own_at(), t.w * sizeof(uint32_t), ow * sizeof(uint32_t), oh,
                                hipMemcpyDeviceToDevice, stream()));
    auto place = [&](int r, const uint32_t *packed) -> int {      // rank r's packed rectangle into the whole plane
      const TilePlace &p = l.place[(size_t)r];
      if (p.own_h() * p.own_w())
        G_HIP(g, hipMemcpy2DAsync(full + p.r0 * field_w + p.c0, field_w * sizeof(uint32_t), packed, p.own_w() * sizeof(uint32_t),
                                  p.own_w() * sizeof(uint32_t), p.own_h(), hipMemcpyDeviceToDevice, stream()));
      return WS_OK;
    };
    if (g->is_rccl) {
      RcclApi *n = rccl();
      const std::vector<size_t> &at = l.at;
      if (me.rank == 0 && (rc = grow(g, me.table, std::max<size_t>(at[(size_t)g->world], 1) * sizeof(uint32_t)))) return rc;
      G_NCCL(g, n->GroupStart());
      if (me.rank != 0) {
        if (oh * ow) G_NCCL(g, n->Send(me.rows.p, oh * ow, ncclUint32, 0, g->comm, stream()));
      } else {
        for (int r = 1; r < g->world; ++r)
          if (at[(size_t)r + 1] > at[(size_t)r])
            G_NCCL(g, n->Recv((uint32_t *)me.table.p + at[(size_t)r], at[(size_t)r + 1] - at[(size_t)r], ncclUint32, r, g->comm, stream()));
      }
      G_NCCL(g, n->GroupEnd());
      if (me.rank == 0) {
        if ((rc = place(0, (const uint32_t *)me.rows.p))) return rc;
        for (int r = 1; r < g->world; ++r)
          if ((rc = place(r, (const uint32_t *)me.table.p + at[(size_t)r]))) return rc;
      }
      G_HIP(g, hipStreamSynchronize(stream()));
      return WS_OK;
    }
    G_HIP(g, hipStreamSynchronize(stream()));      // my packed rectangle is complete before rank 0 copies it
    me.pub_send = (const uint32_t *)me.rows.p;
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    if (me.rank == 0) {
      for (int r = 0; r < g->world; ++r)
        if ((rc = place(r, local(r)->pub_send))) return rc;
      G_HIP(g, hipStreamSynchronize(stream()));
    }
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    return WS_OK;
  }

  // every rank's OWNED part of a held plane -> rank 0's whole plane.  Row blocks send their rows as they lie, in one message:
  // packing them would add a copy.
  int gather_owned(const TileCut &cut, const uint32_t *plane, uint32_t *full) {
    GatherLayout l;
    if (!gather_layout(cut, &l)) return gfail(g, WS_ERR_BAD_ARG, "bad tile grid");
    if (cut.px == 1) return gather_rows(plane + l.place[(size_t)me.rank].own_at(), l, full);
    return gather_rect(plane, l, cut.field_w, full);
  }


  // max (or min) over the ranks of the word at me.flag[0]; stream ordered behind whatever wrote it; ONE host read
  int reduce(bool take_max, uint32_t *result) {
    if (g->is_rccl) {
      G_NCCL(g, rccl()->AllReduce(me.flag, me.flag + 1, 1, ncclUint32, take_max ? ncclMax : ncclMin, g->comm, stream()));
      G_HIP(g, hipMemcpyAsync(me.flag_host, me.flag + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
      G_HIP(g, hipStreamSynchronize(stream()));
      *result = me.flag_host[0];
      return WS_OK;
    }
    G_HIP(g, hipMemcpyAsync(me.flag_host, me.flag, sizeof(uint32_t), hipMemcpyDeviceToHost, stream()));
    G_HIP(g, hipStreamSynchronize(stream()));
    me.pub_word = me.flag_host[0];
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    uint32_t v = me.pub_word;
    for (const Rank &r : g->ranks) v = take_max ? std::max(v, r.pub_word) : std::min(v, r.pub_word);
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");      // (pub_word may be rewritten after this)
    *result = v;
    return WS_OK;
  }
  int reduce_host(uint32_t value, bool take_max, uint32_t *result) {
    me.flag_host[2] = value;
    G_HIP(g, hipMemcpyAsync(me.flag, me.flag_host + 2, sizeof(uint32_t), hipMemcpyHostToDevice, stream()));
    return reduce(take_max, result);
  }

  // `words` u32 at `send` of every rank -> table[rank * words ...] on every rank (table: world * words, on my device)
  int gather(const uint32_t *send, size_t words, uint32_t *table) {
    if (g->is_rccl) {
      G_NCCL(g, rccl()->AllGather(send, table, words, ncclUint32, g->comm, stream()));
      return WS_OK;
    }
    G_HIP(g, hipStreamSynchronize(stream()));      // my part is complete before anyone copies it
    me.pub_send = send;
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    for (const Rank &r : g->ranks)
      G_HIP(g, hipMemcpyAsync(table + (size_t)r.rank * words, r.pub_send, words * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream()));
    G_HIP(g, hipStreamSynchronize(stream()));
    if (!g->barrier.wait()) return gfail(g, WS_ERR_HIP, "another rank of the group failed");
    return WS_OK;
  }
};

// ---- the rank programs: distributed.py's segment_tiled / merge_tiled ------------------------------------------------------

// a rank's block as the programs read it: either descriptor of ws_hip.h (rows: a ws_tile_block, whose image has the plane's pitch)
struct TiledBlock {
  const uint8_t *d_img;
  size_t img_stride;
  const uint32_t *d_seeds_rc, *d_colours;
  size_t n_seeds;
  uint32_t first_colour;
  uint32_t *d_labels;
  bool rows;
};
TiledBlock as_block(const ws_tile_block &b, const TilePlace &t) { return {b.d_img, t.w, b.d_seeds_rc, b.d_colours, b.n_seeds, b.first_colour, b.d_labels, true}; }
TiledBlock as_block(const ws_tile_block2d &b, const TilePlace &) { return {b.d_img, b.img_stride, b.d_seeds_rc, b.d_colours, b.n_seeds, 1, b.d_labels, false}; }

// Rounds of { step; swap the ring of `plane`; copy it in; "did any rank change anything" -- max-reduced, read once } until none did.
template <class Step>
int until_quiet(Exchange &x, uint32_t *plane, const TilePlace &t, uint32_t *rounds, Step step) {
  for (;;) {
    int changed = 0, rc;
    if ((rc = step(&changed))) return rc;
    if ((rc = x.swap(plane, t))) return rc;
    if ((rc = x.copy_ring_in(plane, t))) return rc;
    uint32_t any = 0;
    if ((rc = x.reduce_host(changed ? 1u : 0u, true, &any))) return rc;
    ++*rounds;
    if (!any) return WS_OK;
  }
}

// Row blocks.
// Stamps: ws_block_begin relaxes the block to LOCAL convergence from its seed tables; then rounds of { swap halo rows;
// "did any rank receive a row that differs from the one it holds" -- compared on the device, max-reduced there (RCCL) and
// read once; copy the received rows in; ws_block_relax_halo (only the tile rows next to the halo rows start) }.
// Labels: local two-launch resolve, export the two boundary rows, ONE gather of 2 w words per rank, import.
// Merging: a union-find over all seed colours per rank, local unions, ONE gather of 4 w (colour, root) pairs, relabel.
// Lists that are not strictly increasing / widths that are not multiples of 4: the general form, decided by all ranks
// together (min-reduce of "my block can take the fast form").
int tiled_rank(ws_group *g, Rank &me, const TileCut &cut, const TilePlace &t, size_t n_seeds_total, const TiledBlock &b, const ws_options *opt,
               int merging, uint32_t *rounds_out) {
  G_HIP(g, hipSetDevice(me.device));
  const int world = g->world;
  const size_t h = t.h, w = t.w, n = h * w;
  const int up = t.nb[0] >= 0, down = t.nb[1] >= 0;
  uint32_t rounds = 0;
  Exchange x{g, me};
  int rc;
  if ((rc = grow(g, me.keys, (n ? n : 1) * sizeof(uint32_t)))) return rc;
  if ((rc = grow(g, me.recv, (w ? 2 * w : 1) * sizeof(uint32_t)))) return rc;
  uint32_t *keys = (uint32_t *)me.keys.p, *recv = (uint32_t *)me.recv.p;
  hipStream_t s = me.ctx->stream;

  // can this block take the fast form?  (the order of the list is checked by ws_block_begin, on the device)
  uint32_t fast = b.d_colours == nullptr && (w & 3) == 0 && h >= 2 && n < 0x80000000ull && w > 0 ? 1u : 0u;
  if (fast) {
    rc = ws_block_begin(me.ctx, b.d_img, h, w, w, opt->max_water_level, b.d_seeds_rc, b.n_seeds, b.first_colour, keys);
    if (rc == WS_ERR_UNSUPPORTED) fast = 0;
    else if (rc != WS_OK) return gfail(g, rc, std::string("rank ") + std::to_string(me.rank) + ": ws_block_begin: " + ws_last_error(me.ctx));
  }
  uint32_t all_fast = 0;
  if ((rc = x.reduce_host(fast, false, &all_fast))) return rc;
  ++rounds;
  if (all_fast) {
    for (;;) {
      if ((rc = x.swap(keys, t))) return rc;
      ++rounds;
      G_HIP(g, hipMemsetAsync(me.flag, 0, sizeof(uint32_t), s));
      if (up) G_HIP(g, block_rows_differ(s, recv, keys, w, me.flag));
      if (down) G_HIP(g, block_rows_differ(s, recv + w, keys + (h - 1) * w, w, me.flag));
      uint32_t any = 0;
      if ((rc = x.reduce(true, &any))) return rc;
      if (!any) break;      // every halo row already equals its neighbour's boundary row
      if ((rc = x.copy_ring_in(keys, t))) return rc;
      G_WS(g, me, ws_block_relax_halo(me.ctx, b.d_img, h, w, w, opt->max_water_level, up, down, keys));
    }
    G_WS(g, me, ws_block_resolve_local(me.ctx, keys, b.d_labels, h, w, up, down));
    if ((rc = grow(g, me.rows, 2 * w * sizeof(uint32_t)))) return rc;
    if ((rc = grow(g, me.table, (size_t)world * 2 * w * sizeof(uint32_t)))) return rc;
    G_WS(g, me, ws_block_export_boundary(me.ctx, b.d_labels, h, w, up, down, (size_t)me.rank, (uint32_t *)me.rows.p));
    if ((rc = x.gather((const uint32_t *)me.rows.p, 2 * w, (uint32_t *)me.table.p))) return rc;
    ++rounds;
    G_WS(g, me, ws_block_import_boundary(me.ctx, (const uint32_t *)me.table.p, (size_t)world, (size_t)me.rank, b.d_labels, h, w, up, down));
  } else {
    // general form: painted seeds, relaxation rounds and label rounds, one halo swap and one flag each
    const uint32_t *colours = b.d_colours;
    if (!colours && b.n_seeds) {
      if ((rc = grow(g, me.colours, b.n_seeds * sizeof(uint32_t)))) return rc;
      G_HIP(g, block_iota(s, (uint32_t *)me.colours.p, b.n_seeds, b.first_colour));
      colours = (const uint32_t *)me.colours.p;
    }
    G_WS(g, me, ws_block_init(me.ctx, h, w, b.d_seeds_rc, colours, b.n_seeds, keys, b.d_labels));
    rc = until_quiet(x, keys, t, &rounds, [&](int *changed) { return gfail_if(g, me, ws_block_relax(me.ctx, b.d_img, h, w, w, opt->max_water_level, keys, changed)); });
    if (rc == WS_OK) rc = until_quiet(x, b.d_labels, t, &rounds, [&](int *changed) { return gfail_if(g, me, ws_block_resolve(me.ctx, keys, b.d_labels, h, w, changed)); });
    if (rc) return rc;
  }
  if (merging) {
    const size_t n_pairs = 4 * w;
    if ((rc = grow(g, me.parent, (n_seeds_total + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = grow(g, me.rows, n_pairs * 2 * sizeof(uint32_t)))) return rc;
    if ((rc = grow(g, me.table, (size_t)world * n_pairs * 2 * sizeof(uint32_t)))) return rc;
    uint32_t *parent = (uint32_t *)me.parent.p;
    G_WS(g, me, ws_block_merge_local(me.ctx, b.d_labels, h, w, t.lo, cut.field_h, n_seeds_total, parent));
    G_WS(g, me, ws_block_merge_export(me.ctx, b.d_labels, h, w, parent, (uint32_t *)me.rows.p));
    if ((rc = x.gather((const uint32_t *)me.rows.p, n_pairs * 2, (uint32_t *)me.table.p))) return rc;
    ++rounds;
    G_WS(g, me, ws_block_merge_import(me.ctx, (const uint32_t *)me.table.p, (size_t)world * n_pairs, parent));
    G_WS(g, me, ws_block_merge_relabel(me.ctx, b.d_labels, n, parent, n_seeds_total, b.d_labels));      // elementwise: in place
  }
  G_HIP(g, hipStreamSynchronize(s));
  *rounds_out = rounds;
  return WS_OK;
}

// A field cut into py x px tiles (BASELINE config 5's "2-D tiles"; rank = ty * px + tx): every tile is a plane with a halo
// ring of one pixel wherever it has a neighbour -- exactly the pixels the flood never writes, rows AND columns
// (lib.rs:220-222), so the block steps of the general form run on it unchanged: painted seeds with their global colours,
// rounds of { relax to local convergence; swap halo rows and columns; "did any rank change anything" }, then the same
// rounds for the labels (one hop per sweep).  Halo traffic per round: 2 (w + h) words a tile.
int tiled2d_rank(ws_group *g, Rank &me, const TileCut &cut, const TilePlace &t, size_t n_seeds_total, const TiledBlock &b, const ws_options *opt,
                 int merging, uint32_t *rounds_out) {
  G_HIP(g, hipSetDevice(me.device));
  const size_t h = t.h, w = t.w, n = h * w;
  const int *nb = t.nb;
  uint32_t rounds = 0;
  Exchange x{g, me};
  int rc;
  if ((rc = grow(g, me.keys, (n ? n : 1) * sizeof(uint32_t)))) return rc;
  if ((rc = grow(g, me.recv, (2 * w + 2 * h + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = grow(g, me.cols, (2 * h + 1) * sizeof(uint32_t)))) return rc;
  uint32_t *keys = (uint32_t *)me.keys.p, *recv = (uint32_t *)me.recv.p;
  hipStream_t s = me.ctx->stream;
  G_WS(g, me, ws_block_init(me.ctx, h, w, b.d_seeds_rc, b.d_colours, b.n_seeds, keys, b.d_labels));
  // stamps: relax to local convergence, swap the ring, until no rank changed anything
  rc = until_quiet(x, keys, t, &rounds, [&](int *changed) { return gfail_if(g, me, ws_block_relax(me.ctx, b.d_img, h, w, b.img_stride, opt->max_water_level, keys, changed)); });
  if (rc) return rc;
  // labels: the whole tile in two launches from its seeds and from what the ring says so far (ws_block_resolve_ring), swap
  // the ring, until no rank receives a ring that differs from the one it holds: a round carries labels across one tile
  // boundary.  (The iterative resolve -- one hop per launch -- took 32 launches per rank where this takes 3 rounds of 2.)
  if (n >= 0x80000000ull) {      // planes of 2^31 pixels and more: the iterative form
    rc = until_quiet(x, b.d_labels, t, &rounds, [&](int *changed) { return gfail_if(g, me, ws_block_resolve(me.ctx, keys, b.d_labels, h, w, changed)); });
    if (rc) return rc;
  } else {
    if ((rc = grow(g, me.rows, (2 * h + 1) * sizeof(uint32_t)))) return rc;
    uint32_t *held = (uint32_t *)me.rows.p;      // the halo columns I hold, packed like the received ones
    for (;;) {
      G_WS(g, me, ws_block_resolve_ring(me.ctx, keys, b.d_labels, h, w));
      if ((rc = x.swap(b.d_labels, t))) return rc;
      G_HIP(g, hipMemsetAsync(me.flag, 0, sizeof(uint32_t), s));
      // (the four corner cells of the ring are left out: the row copy and the column copy both write them, with different
      // ranks' values, and nobody's stencil reads them)
      if (nb[0] >= 0 && w > 2) G_HIP(g, block_rows_differ(s, recv + 1, b.d_labels + 1, w - 2, me.flag));
      if (nb[1] >= 0 && w > 2) G_HIP(g, block_rows_differ(s, recv + w + 1, b.d_labels + (h - 1) * w + 1, w - 2, me.flag));
      if (nb[2] >= 0 || nb[3] >= 0) {
        G_HIP(g, block_pack_cols(s, b.d_labels, h, w, 0, w - 1, held));
        if (nb[2] >= 0 && h > 2) G_HIP(g, block_rows_differ(s, recv + 2 * w + 1, held + 1, h - 2, me.flag));
        if (nb[3] >= 0 && h > 2) G_HIP(g, block_rows_differ(s, recv + 2 * w + h + 1, held + h + 1, h - 2, me.flag));
      }
      uint32_t any = 0;
      if ((rc = x.reduce(true, &any))) return rc;
      ++rounds;
      if (!any) break;
      if ((rc = x.copy_ring_in(b.d_labels, t))) return rc;
    }
  }
  if (merging) {
    // as the row blocks' (ws_block_merge_*): a union-find over all seed colours per rank, the touching colours of the tile
    // joined under find_merge's rule (one pixel of a pair interior IN THE WHOLE FIELD), then ONE gather of (colour, local
    // root) pairs of the tile's two outermost rows and columns on every side, every pair joined, the relabel
    const size_t max_h = (cut.field_h + (size_t)cut.py - 1) / (size_t)cut.py + 2, max_w = (cut.field_w + (size_t)cut.px - 1) / (size_t)cut.px + 2;
    const size_t n_pairs = 4 * max_w + 4 * max_h;      // the same for every rank: a tile's own 4 w + 4 h, then (0, 0)
    const int world = g->world;
    if ((rc = grow(g, me.parent, (n_seeds_total + 1) * sizeof(uint32_t)))) return rc;
    if ((rc = grow(g, me.rows, n_pairs * 2 * sizeof(uint32_t)))) return rc;
    if ((rc = grow(g, me.table, (size_t)world * n_pairs * 2 * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(me.ctx, me.ctx->uf_size, (n_seeds_total + 1) * sizeof(uint32_t)))) return gfail(g, rc, "out of memory");
    uint32_t *parent = (uint32_t *)me.parent.p;
    G_HIP(g, uf_init(s, parent, (uint32_t *)me.ctx->uf_size.p, n_seeds_total + 1));
    G_HIP(g, block_union_pixels(s, b.d_labels, (int)h, (int)w, (int)t.lo, (int)cut.field_h, parent, (int)t.clo, (int)cut.field_w));
    G_HIP(g, block_colour_roots2d(s, b.d_labels, (int)h, (int)w, parent, (uint2 *)me.rows.p, n_pairs));
    if ((rc = x.gather((const uint32_t *)me.rows.p, n_pairs * 2, (uint32_t *)me.table.p))) return rc;
    ++rounds;
    G_HIP(g, union_edges(s, (const uint2 *)me.table.p, (size_t)world * n_pairs, parent, nullptr, nullptr));
    G_HIP(g, relabel_final_u32(s, b.d_labels, parent, n_seeds_total + 1, b.d_labels, n));      // elementwise: in place
  }
  G_HIP(g, hipStreamSynchronize(s));
  *rounds_out = rounds;
  return WS_OK;
}

// The flood of one rank's block: a group of one rank runs the ordinary single-device transform on a row block (the block is the
// whole field), everything else its rank program.
int flood(ws_group *g, Rank &me, const TileCut &cut, const TilePlace &t, size_t n_seeds_total, const TiledBlock &b, const ws_options *opt, int merging,
          uint32_t *rounds) {
  if (!b.rows) return tiled2d_rank(g, me, cut, t, n_seeds_total, b, opt, merging, rounds);
  if (g->world > 1) return tiled_rank(g, me, cut, t, n_seeds_total, b, opt, merging, rounds);
  if (b.d_colours) return gfail(g, WS_ERR_UNSUPPORTED, "a group of one rank takes the caller's list as it is: d_colours must be NULL");
  if (merging) G_WS(g, me, ws_merge_device(me.ctx, b.d_img, t.h, t.w, t.w, b.d_seeds_rc, b.n_seeds, opt, b.d_labels));
  else G_WS(g, me, ws_segment_device(me.ctx, b.d_img, t.h, t.w, t.w, b.d_seeds_rc, b.n_seeds, opt, b.d_labels));
  return WS_OK;
}

// ---- the flood, and its two planes on rank 0 -----------------------------------------------------------------------------------
// transform_to_list (lib.rs:1551-1561 merging, 1837-1847 segmenting) and merge_tree of a tiled field: the SEGMENTING flood -- the
// part that scales with the pixels and needs the halo exchange -- runs on all ranks, then every rank sends the arrival stamps
// and segment labels of what it owns to rank 0, whose context makes the records of all levels from the whole planes (the arrival
// forms: 8 B per pixel gathered, 20 B per pixel of workspace -- a 32768^2 field is 28 GiB of one device's 288).  Lists and tree
// are global objects (a lake spans blocks, its area is a sum over them); cutting the union-find itself across ranks would trade
// this one gather for an exchange per level.  
struct FloodedField {
  const uint32_t *keys = nullptr, *labels = nullptr;      // h x w of the cut, on rank 0's device; null elsewhere
};

// reserve(gathers): what rank 0 allocates beyond the two planes, BEFORE the first gather -- no allocation may fail between two
// collectives, where the peers would wait for a rank that has left.  (gathers false: a group of one has run the single-device
// transform and nobody waits.)
template <class Reserve>
int flood_to_root(ws_group *g, Rank &me, const TileCut &cut, const TilePlace &t, size_t n_seeds_total, const TiledBlock &b, const ws_options *opt,
                  uint32_t *rounds, Reserve reserve, FloodedField *out) {
  int rc;
  if ((rc = flood(g, me, cut, t, n_seeds_total, b, opt, 0, rounds))) return rc;
  const bool alone = b.rows && g->world == 1;      // the single-device transform ran: its planes are the field's
  const size_t n = cut.field_h * cut.field_w;
  if (me.rank == 0) {
    if (!alone && (rc = grow(g, me.full_keys, (n ? n : 1) * sizeof(uint32_t)))) return rc;
    if (!alone && (rc = grow(g, me.full_labels, (n ? n : 1) * sizeof(uint32_t)))) return rc;
    if ((rc = reserve(!alone))) return rc;
  }
  if (alone) {
    size_t kh = 0, kw = 0;
    G_WS(g, me, ws_last_arrival_device(me.ctx, &out->keys, &kh, &kw));
    out->labels = b.d_labels;
    return WS_OK;
  }
  Exchange x{g, me};
  G_HIP(g, hipStreamSynchronize(me.ctx->stream));
  if ((rc = x.gather_owned(cut, (const uint32_t *)me.keys.p, (uint32_t *)me.full_keys.p))) return rc;
  if ((rc = x.gather_owned(cut, b.d_labels, (uint32_t *)me.full_labels.p))) return rc;
  if (me.rank == 0) *out = {(const uint32_t *)me.full_keys.p, (const uint32_t *)me.full_labels.p};
  return WS_OK;
}

// runs f(rank) for every local rank: side by side on host threads for a local group of several ranks
template <class F>
int for_local_ranks(ws_group *g, F f) {
  const size_t nl = g->ranks.size();
  g->barrier.reset((int)nl);
  { std::lock_guard<std::mutex> l(g->err_m); g->err.clear(); }
  if (nl == 1) return f(g->ranks[0]);
  std::vector<int> rcs(nl, WS_OK);
  std::vector<std::thread> th;
  for (size_t i = 0; i < nl; ++i)
    th.emplace_back([&, i] {
      rcs[i] = f(g->ranks[i]);
      if (rcs[i] != WS_OK) g->barrier.abort();      // nobody waits for a rank that has left
    });
  for (std::thread &t : th) t.join();
  // the rank that failed first in its own right, not the ones that were told "another rank failed"
  int first = WS_OK;
  for (int rc : rcs) if (rc != WS_OK && (first == WS_OK || first == WS_ERR_HIP)) first = rc;
  return first;
}

int check_group_call(ws_group *g, const ws_options *opt) {
  if (!g) return WS_ERR_BAD_ARG;
  if (!opt) return gfail(g, WS_ERR_BAD_ARG, "options pointer is null");
  const int v = ws_options_validate(opt);
  if (v != WS_OK) return gfail(g, v, ws_strerror(v));
  if (pick_engine(opt) == WS_ENGINE_SWEEP && g->world > 1) return gfail(g, WS_ERR_UNSUPPORTED, "the sweep engine has no tiled form");
  return WS_OK;
}

// f(rank, its index among the local ones, its place, &rounds) on every local rank; *exchange_rounds: the collective steps the
// first local rank took part in
template <class F>
int run_tiled(ws_group *g, const TileCut &cut, uint32_t *exchange_rounds, F f) {
  if (exchange_rounds) *exchange_rounds = 0;
  std::vector<uint32_t> rounds(g->ranks.size(), 0);
  const int rc = for_local_ranks(g, [&](Rank &me) -> int {
    TilePlace t;
    if (!tile_place(cut, me.rank, &t)) return gfail(g, WS_ERR_BAD_ARG, "bad tile grid");
    const size_t i = (size_t)(me.rank - g->first_local);
    return f(me, i, t, &rounds[i]);
  });
  if (exchange_rounds) *exchange_rounds = rounds[0];
  return rc;
}

// ---- the argument check of the tiled device forms (the order of its tests: include/ws_hip.h, above the tiled section) ----------

// the catalogue request of the tiled tree forms: the whole field's weight plane, on rank 0's device (host forms: in host memory)
struct TreeWeights {
  const void *weight;
  int dtype;
  size_t stride;
};

// the weight arguments, checked on every rank before anything runs, as ws_merge_tree_from_arrival_device checks them on rank 0
// afterwards (check_lake_weights): a call that rank 0 would refuse after the flood has left its peers' work for nothing
int check_tree_weights(ws_group *g, const TreeWeights &wt, bool image_stands_in, size_t w, size_t ph, size_t pw) {
  uint64_t wmax = 0xFFull;
  if (wt.weight) {
    if (wt.dtype != WS_U8 && wt.dtype != WS_U16) return gfail(g, WS_ERR_UNSUPPORTED, "weights are u8 or u16");
    if (wt.stride < w) return gfail(g, WS_ERR_BAD_ARG, "weight_row_stride < w");
    if (wt.dtype == WS_U16) wmax = 0xFFFFull;
  } else if (!image_stands_in) {
    return gfail(g, WS_ERR_BAD_ARG, "no rank holds the whole image: the catalogue needs d_weight");
  }
  const uint64_t pixels = (uint64_t)ph * pw, longest = std::max(ph, pw);
  if (longest && pixels > UINT64_MAX / wmax / longest) return gfail(g, WS_ERR_TOO_LARGE, "the weighted moments do not fit in 64 bits");
  return WS_OK;
}

// what a device form writes beyond the blocks, as the check reads it
struct TiledOutputs {
  bool counts = true;                          // the host words every rank writes are all there
  bool on_root = true;                         // ... and the device buffers of rank 0
  const TreeWeights *catalogue = nullptr;      // a catalogue is wanted: its weights
};

TileCut row_cut(const ws_group *g, size_t h, size_t w) { return TileCut{h, w, g ? g->world : 1, 1}; }

// The rules of the two descriptors.  Row blocks take a field of no columns (and then no pointers); tiles do not.
const char *field_too_small(const TileCut &c, bool tiles) {
  if (!tiles) return c.field_h < (size_t)c.py ? "a field needs at least one row per rank" : nullptr;
  return c.field_h < (size_t)c.py || c.field_w < (size_t)c.px ? "a field needs at least one row and one column per tile" : nullptr;
}
bool block_ok(const ws_tile_block &b, const TileCut &c, const TilePlace &) {
  return b.reserved == 0 && (c.field_h * c.field_w == 0 || (b.d_img && b.d_labels)) && (!b.n_seeds || b.d_seeds_rc);
}
bool block_ok(const ws_tile_block2d &b, const TileCut &, const TilePlace &t) {
  return b.d_img && b.d_labels && b.img_stride >= t.w && (!b.n_seeds || (b.d_seeds_rc && b.d_colours));
}

template <class B>
int check_tiled_call(ws_group *g, const ws_options *opt, const TileCut &cut, size_t n_seeds_total, const B *blocks, const TiledOutputs &out) {
  int rc = check_group_call(g, opt);
  if (rc) return rc;
  if (!blocks || !out.counts) return gfail(g, WS_ERR_BAD_ARG, "null pointer");
  if (cut.py < 1 || cut.px < 1 || cut.py * cut.px != g->world) return gfail(g, WS_ERR_BAD_ARG, "py * px must be the group's number of ranks");
  if (opt->edge_correction) return gfail(g, WS_ERR_UNSUPPORTED, "the tiled device forms take the field as it is: pad it first (the host forms do)");
  if (const char *why = field_too_small(cut, std::is_same<B, ws_tile_block2d>::value)) return gfail(g, WS_ERR_BAD_ARG, why);
  if (n_seeds_total >= 0x7FFFFFFFull) return gfail(g, WS_ERR_TOO_LARGE, "colours must stay below 2^31");
  if (g->first_local == 0 && !out.on_root) return gfail(g, WS_ERR_BAD_ARG, "an output buffer of rank 0 is null");
  if (out.catalogue && (rc = check_tree_weights(g, *out.catalogue, false, cut.field_w, cut.field_h, cut.field_w))) return rc;
  for (size_t i = 0; i < g->ranks.size(); ++i) {
    TilePlace t;
    if (!tile_place(cut, g->first_local + (int)i, &t)) return gfail(g, WS_ERR_BAD_ARG, "bad tile grid");
    if (!block_ok(blocks[i], cut, t)) return gfail(g, WS_ERR_BAD_ARG, "bad block descriptor");
  }
  return WS_OK;
}

// ---- the device forms: one body per product, over either descriptor -------------------------------------------------------------

template <class B>
int segment_tiled_device(ws_group *g, const TileCut &cut, size_t n_seeds_total, const B *blocks, const ws_options *opt, int merging,
                         uint32_t *exchange_rounds) {
  if (int rc = check_tiled_call(g, opt, cut, n_seeds_total, blocks, TiledOutputs{})) return rc;
  return run_tiled(g, cut, exchange_rounds, [&](Rank &me, size_t i, const TilePlace &t, uint32_t *rounds) {
    return flood(g, me, cut, t, n_seeds_total, as_block(blocks[i], t), opt, merging, rounds);
  });
}

template <class B>
int lists_tiled_device(ws_group *g, const TileCut &cut, size_t n_seeds_total, const B *blocks, const ws_options *opt, int merging, ws_lake *d_lakes,
                       size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured, uint32_t *exchange_rounds) {
  TiledOutputs out;
  out.counts = n_lakes && offsets && uncoloured;
  out.on_root = d_lakes || !cap;
  if (int rc = check_tiled_call(g, opt, cut, n_seeds_total, blocks, out)) return rc;
  *n_lakes = 0;
  return run_tiled(g, cut, exchange_rounds, [&](Rank &me, size_t i, const TilePlace &t, uint32_t *rounds) -> int {
    FloodedField f;
    const int rc = flood_to_root(g, me, cut, t, n_seeds_total, as_block(blocks[i], t), opt, rounds, [](bool) { return WS_OK; }, &f);
    if (rc || me.rank != 0) return rc;
    return gfail_if(g, me, ws_lists_from_arrival_device(me.ctx, merging, f.keys, f.labels, cut.field_h, cut.field_w, n_seeds_total, opt, d_lakes, cap, n_lakes,
                                                        offsets, uncoloured));
  });
}

// rank 0 of a tree form, before the first gather: everything the arrival form will ensure for the colours
int reserve_tree_root(ws_group *g, Rank &me, bool gathers, size_t n_seeds, bool stats) {
  if (gathers) G_WS(g, me, merge_tree_arrival_reserve(me.ctx, n_seeds, stats));
  return WS_OK;
}

template <class B>
int tree_tiled_device(ws_group *g, const TileCut &cut, size_t n_seeds_total, const B *blocks, const ws_options *opt, const TreeWeights &wt,
                      ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *exchange_rounds) {
  TiledOutputs out;
  out.on_root = d_tree != nullptr;
  out.catalogue = d_stats ? &wt : nullptr;
  if (int rc = check_tiled_call(g, opt, cut, n_seeds_total, blocks, out)) return rc;
  return run_tiled(g, cut, exchange_rounds, [&](Rank &me, size_t i, const TilePlace &t, uint32_t *rounds) -> int {
    FloodedField f;
    const int rc = flood_to_root(g, me, cut, t, n_seeds_total, as_block(blocks[i], t), opt, rounds,
                                 [&](bool gathers) { return reserve_tree_root(g, me, gathers, n_seeds_total, d_stats != nullptr); }, &f);
    if (rc || me.rank != 0) return rc;
    return gfail_if(g, me, ws_merge_tree_from_arrival_device(me.ctx, f.keys, f.labels, cut.field_h, cut.field_w, n_seeds_total, opt, wt.weight, wt.dtype,
                                                             wt.stride, d_tree, d_stats));
  });
}

// ---- host buffers in and out: a job and its stages --------------------------------------------------------------------------------
// Every local rank uploads its block of the (padded) image and the seeds that fall on it, floods, and delivers.  Seeds: a list
// whose rows never decrease (every row-major sorted list; find_local_minima's) gives every row block ONE contiguous range; any
// other list, and every list on tiles, is dealt out seed by seed with explicit colours (ws_tile_plan.hpp).  With edge correction
// the rank's part of the PADDED plane is built on the device: a zeroed block and a 2-D copy of the image window that falls
// into it.

// the lake records of transform_to_list, wanted from a host-buffer tiled call (ws_transform_to_list_tiled)
struct HostLists {
  ws_lake *lakes;
  size_t cap;
  size_t *n_lakes;
  uint64_t *offsets, *uncoloured;
};

// the tree and (stats: nullable) the catalogue, wanted from a host-buffer tiled call (ws_merge_tree_tiled); weight null: the image
struct HostTree {
  ws_tree_node *tree;
  ws_lake_stats *stats;
  TreeWeights wt;
};

struct TiledHostJob {
  const uint8_t *img;      // the caller's arguments, in this order: an entry point writes J{img, h, w, stride, seeds_rc, n_seeds, opt}
  size_t h, w, stride;
  const uint64_t *seeds_rc;
  size_t n_seeds;
  const ws_options *opt;
  bool tiles = false;      // a py x px cut run by tiled2d_rank; else row blocks, one per rank of the group
  int py = 0, px = 0;
  // exactly one product: the labels (of the merging transform with `merging`), the lists, or the tree
  enum { LABELS, LISTS, TREE } want = LABELS;
  int merging = 0;         // LABELS, LISTS
  uint64_t *out_labels = nullptr;
  HostLists lists{};
  HostTree tree{};
  // what host_check derives: the cut of the (padded) plane, the options of a block of it
  TileCut cut;
  bool edge = false, rows_sorted = true;
  size_t shift = 0;
  ws_options plain{};
  bool stats() const { return tree.stats != nullptr; }
  size_t weight_bytes() const { return stats() && tree.wt.weight && tree.wt.dtype == WS_U16 ? 2 : 1; }
  size_t tree_bytes() const { return (n_seeds + 1) * sizeof(ws_tree_node); }
};

int host_check(ws_group *g, TiledHostJob &J) {
  int rc = check_group_call(g, J.opt);
  if (rc) return rc;
  if ((!J.img && J.h * J.w) || (!J.seeds_rc && J.n_seeds) || J.stride < J.w) return gfail(g, WS_ERR_BAD_ARG, "bad argument");
  if (!J.tiles) { J.py = g->world; J.px = 1; }
  if (J.py < 1 || J.px < 1 || J.py * J.px != g->world) return gfail(g, WS_ERR_BAD_ARG, "py * px must be the group's number of ranks");
  if (J.tiles && J.want != TiledHostJob::LABELS) return gfail(g, WS_ERR_UNSUPPORTED, "the host form in tiles delivers labels only");
  J.edge = J.opt->edge_correction != 0;
  J.shift = J.edge && J.opt->seed_shift ? 1 : 0;
  const size_t ph = J.h + (J.edge ? 2 : 0), pw = J.w + (J.edge ? 2 : 0);
  J.cut = TileCut{ph, pw, J.py, J.px};
  if (J.want == TiledHostJob::LABELS && !J.out_labels && ph * pw) return gfail(g, WS_ERR_BAD_ARG, "out_labels is null");
  if (J.want == TiledHostJob::TREE && J.stats() && (rc = check_tree_weights(g, J.tree.wt, true, J.w, ph, pw))) return rc;
  if (J.n_seeds >= 0x7FFFFFFFull) return gfail(g, WS_ERR_TOO_LARGE, "too many seeds");
  if (ph > TILE_MAX_SIDE || pw > TILE_MAX_SIDE) return gfail(g, WS_ERR_TOO_LARGE, "plane too large");
  if (const char *why = field_too_small(J.cut, J.tiles)) return gfail(g, WS_ERR_BAD_ARG, why);
  // the reference indexes the (padded) plane with the caller's coordinates and panics outside it (lib.rs:1675-1677)
  if (first_seed_outside(J.seeds_rc, J.n_seeds, ph, pw, J.shift, &J.rows_sorted) != J.n_seeds)
    return gfail(g, WS_ERR_SEED_OOB, "seed outside the label plane (the reference panics: lib.rs:1676)");
  J.plain = *J.opt;
  J.plain.edge_correction = 0;      // the blocks hold the padded plane's own pixels
  J.plain.seed_shift = 0;
  return WS_OK;
}

// the rank's block of the (padded) image and its seeds in local coordinates, on its device
int upload_block(ws_group *g, Rank &me, const TiledHostJob &J, const TilePlace &t, TiledBlock *b) {
  G_HIP(g, hipSetDevice(me.device));
  hipStream_t s = me.ctx->stream;
  const size_t bn = t.h * t.w;
  int rc;
  if ((rc = grow(g, me.img, bn ? bn : 1))) return rc;
  if ((rc = grow(g, me.labels, (bn ? bn : 1) * sizeof(uint32_t)))) return rc;
  // the ring of an edge-corrected plane is zero.  (Row blocks without edge correction are all image and are not zeroed; tiles always are.)
  if (J.edge || J.tiles) G_HIP(g, hipMemsetAsync(me.img.p, 0, bn ? bn : 1, s));
  const ImageWindow v = image_window(t, J.h, J.w, J.edge);
  if (v.rows * v.cols)
    G_HIP(g, hipMemcpy2DAsync((uint8_t *)me.img.p + v.dst_r * t.w + v.dst_c, t.w, J.img + v.src_r * J.stride + v.src_c, J.stride, v.cols, v.rows,
                              hipMemcpyHostToDevice, s));
  const SeedDeal d = deal_seeds(J.seeds_rc, J.n_seeds, J.shift, t, !J.tiles && J.rows_sorted);
  const size_t ns = d.n();
  if ((rc = grow(g, me.seeds, (ns ? ns : 1) * 2 * sizeof(uint32_t)))) return rc;
  if (d.explicit_colours && (rc = grow(g, me.colours, (ns ? ns : 1) * sizeof(uint32_t)))) return rc;
  if (ns) G_HIP(g, hipMemcpyAsync(me.seeds.p, d.loc.data(), ns * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  if (ns && d.explicit_colours) G_HIP(g, hipMemcpyAsync(me.colours.p, d.col.data(), ns * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  G_HIP(g, hipStreamSynchronize(s));      // the deal leaves scope; the block steps run on this stream anyway
  // (a group of one rank on a row block runs the single-device transform, which takes the list as it is: colour = index + 1)
  const bool colours = d.explicit_colours && (J.tiles || g->world > 1);
  *b = TiledBlock{(const uint8_t *)me.img.p, t.w, (const uint32_t *)me.seeds.p, colours ? (const uint32_t *)me.colours.p : nullptr, ns, d.first_colour,
                  (uint32_t *)me.labels.p, !J.tiles};
  return WS_OK;
}

// LABELS: what the rank owns, widened, into the caller's plane
int deliver_labels(ws_group *g, Rank &me, const TiledHostJob &J, const TilePlace &t) {
  const size_t oh = t.own_h(), ow = t.own_w(), pw = J.cut.field_w, bn = t.h * t.w;
  const uint32_t *own = (const uint32_t *)me.labels.p + t.own_at();
  uint64_t *out = J.out_labels + t.r0 * pw + t.c0;
  hipStream_t s = me.ctx->stream;
  int rc;
  if (!(oh * ow)) return WS_OK;
  if (J.cut.px == 1) {
    // whole rows: as u32 chunks over the rank's own link, widened by host threads of the rank's context (ws_hostcopy.hip)
    G_WS(g, me, labels_to_host_u64(me.ctx, own, out, oh * ow));
  } else if (host_copy_in_chunks(me.ctx, oh * ow)) {
    // a rectangle: packed on the device, over the bus as u32 chunks, widened into its rows of the caller's plane
    if ((rc = grow(g, me.rows, oh * ow * sizeof(uint32_t)))) return rc;
    G_HIP(g, hipMemcpy2DAsync(me.rows.p, ow * sizeof(uint32_t), own, t.w * sizeof(uint32_t), ow * sizeof(uint32_t), oh, hipMemcpyDeviceToDevice, s));
    G_WS(g, me, labels_to_host_u64(me.ctx, (const uint32_t *)me.rows.p, out, oh * ow, nullptr, ow, pw));
  } else {
    if ((rc = grow(g, me.out64, bn * sizeof(uint64_t)))) return rc;
    G_HIP(g, widen_labels(s, (const uint32_t *)me.labels.p, (uint64_t *)me.out64.p, bn));
    G_HIP(g, hipMemcpy2DAsync(out, pw * sizeof(uint64_t), (const uint64_t *)me.out64.p + t.own_at(), t.w * sizeof(uint64_t), ow * sizeof(uint64_t), oh,
                              hipMemcpyDeviceToHost, s));
    G_HIP(g, hipStreamSynchronize(s));
  }
  return WS_OK;
}

// LISTS, on rank 0: the records of all levels from the whole planes, to the caller's buffer
int deliver_lists(ws_group *g, Rank &me, const TiledHostJob &J, const FloodedField &f) {
  const HostLists &l = J.lists;
  const size_t ph = J.cut.field_h, pw = J.cut.field_w;
  hipStream_t s = me.ctx->stream;
  int rc;
  if ((rc = grow(g, me.out64, std::max<size_t>(l.cap, 1) * sizeof(ws_lake)))) return rc;
  const int made = ws_lists_from_arrival_device(me.ctx, J.merging, f.keys, f.labels, ph, pw, J.n_seeds, &J.plain, (ws_lake *)me.out64.p, l.cap, l.n_lakes,
                                                l.offsets, l.uncoloured);
  if (made != WS_OK && made != WS_ERR_CAPACITY) return gfail_if(g, me, made);
  const size_t got = std::min(*l.n_lakes, l.cap);
  // (many records: narrowed to u32 on the device -- a colour and an area of a plane below 2^31 pixels fit -- and widened into
  // the caller's ws_lake records by the host threads of rank 0's context, 8 M records a piece: half the bytes over the bus)
  const size_t piece_max = (size_t)1 << 23;
  if (got >= ((size_t)1 << 21) && ph * pw < 0x80000000ull) {
    if ((rc = grow(g, me.rows, std::min(got, piece_max) * 2 * sizeof(uint32_t)))) return rc;
    for (size_t off = 0; off < got; off += piece_max) {
      const size_t piece = std::min(piece_max, got - off);
      G_HIP(g, narrow_words(s, (const uint64_t *)((const ws_lake *)me.out64.p + off), (uint32_t *)me.rows.p, 2 * piece));
      G_WS(g, me, labels_to_host_u64(me.ctx, (const uint32_t *)me.rows.p, (uint64_t *)(l.lakes + off), 2 * piece));
    }
  } else if (got) {
    G_HIP(g, hipMemcpyAsync(l.lakes, me.out64.p, got * sizeof(ws_lake), hipMemcpyDeviceToHost, s));
  }
  G_HIP(g, hipStreamSynchronize(s));
  return gfail_if(g, me, made);
}

// TREE, on rank 0 before the first gather: what the arrival form will ensure, the records' device buffer, the weights plane
int reserve_host_tree(ws_group *g, Rank &me, const TiledHostJob &J, bool gathers) {
  const size_t n = J.cut.field_h * J.cut.field_w;
  int rc;
  if ((rc = reserve_tree_root(g, me, gathers, J.n_seeds, J.stats()))) return rc;
  if ((rc = grow(g, me.out64, J.tree_bytes() + (J.stats() ? (J.n_seeds + 1) * sizeof(ws_lake_stats) : 0)))) return rc;
  if (J.stats() && (rc = grow(g, me.weight, (n ? n : 1) * J.weight_bytes()))) return rc;
  return WS_OK;
}

// TREE, on rank 0: the weights of the (padded) plane built here, the tree and the catalogue from the whole planes, to the caller
int deliver_tree(ws_group *g, Rank &me, const TiledHostJob &J, const FloodedField &f) {
  const size_t ph = J.cut.field_h, pw = J.cut.field_w, n = ph * pw, elem = J.weight_bytes();
  const bool stats = J.stats();
  hipStream_t s = me.ctx->stream;
  if (stats) {      // the caller's plane, or the image, one pixel in under edge correction; the ring weighs 0
    const TreeWeights &wt = J.tree.wt;
    const uint8_t *src = wt.weight ? (const uint8_t *)wt.weight : J.img;
    const size_t src_stride = wt.weight ? wt.stride : J.stride, off = J.edge ? 1 : 0;
    if (J.edge) G_HIP(g, hipMemsetAsync(me.weight.p, 0, (n ? n : 1) * elem, s));
    if (J.h * J.w)
      G_HIP(g, hipMemcpy2DAsync((uint8_t *)me.weight.p + (off * pw + off) * elem, pw * elem, src, src_stride * elem, J.w * elem, J.h, hipMemcpyHostToDevice, s));
  }
  ws_tree_node *d_tree = (ws_tree_node *)me.out64.p;
  ws_lake_stats *d_stats = stats ? (ws_lake_stats *)((uint8_t *)me.out64.p + J.tree_bytes()) : nullptr;
  G_WS(g, me, ws_merge_tree_from_arrival_device(me.ctx, f.keys, f.labels, ph, pw, J.n_seeds, &J.plain, me.weight.p, elem == 2 ? WS_U16 : WS_U8, pw, d_tree, d_stats));
  G_HIP(g, hipMemcpyAsync(J.tree.tree, d_tree, J.tree_bytes(), hipMemcpyDeviceToHost, s));
  if (stats) G_HIP(g, hipMemcpyAsync(J.tree.stats, d_stats, (J.n_seeds + 1) * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, s));
  G_HIP(g, hipStreamSynchronize(s));
  return WS_OK;
}

int run_host_job(ws_group *g, TiledHostJob &J, uint32_t *exchange_rounds) {
  if (int rc = host_check(g, J)) return rc;
  return run_tiled(g, J.cut, exchange_rounds, [&](Rank &me, size_t, const TilePlace &t, uint32_t *rounds) -> int {
    TiledBlock b;
    int rc;
    if ((rc = upload_block(g, me, J, t, &b))) return rc;
    if (J.want == TiledHostJob::LABELS) {
      if ((rc = flood(g, me, J.cut, t, J.n_seeds, b, &J.plain, J.merging, rounds))) return rc;
      return deliver_labels(g, me, J, t);
    }
    FloodedField f;
    auto reserve = [&](bool gathers) { return J.want == TiledHostJob::TREE ? reserve_host_tree(g, me, J, gathers) : WS_OK; };
    if ((rc = flood_to_root(g, me, J.cut, t, J.n_seeds, b, &J.plain, rounds, reserve, &f)) || me.rank != 0) return rc;
    return J.want == TiledHostJob::TREE ? deliver_tree(g, me, J, f) : deliver_lists(g, me, J, f);
  });
}

}  // namespace

// ============================================================================ C ABI ====

extern "C" {

int ws_tile_rows(size_t h, int rank, int world, size_t *r0, size_t *r1, size_t *lo, size_t *hi) {
  if (!r0 || !r1 || !lo || !hi) return WS_ERR_BAD_ARG;
  return tile_split(h, rank, world, r0, r1, lo, hi) ? WS_OK : WS_ERR_BAD_ARG;
}

int ws_tile_grid(size_t h, size_t w, int rank, int py, int px, size_t *rows, size_t *cols) {
  if (py < 1 || px < 1 || rank < 0 || rank >= py * px || !rows || !cols) return WS_ERR_BAD_ARG;
  int rc = ws_tile_rows(h, rank / px, py, rows, rows + 1, rows + 2, rows + 3);
  if (rc == WS_OK) rc = ws_tile_rows(w, rank % px, px, cols, cols + 1, cols + 2, cols + 3);
  return rc;
}

static int group_alloc_rank(ws_group *g, Rank &r) {
  G_HIP(g, hipSetDevice(r.device));
  const int rc = ws_ctx_create(r.device, &r.ctx);
  if (rc != WS_OK) return gfail(g, rc, "ws_ctx_create failed");
  G_HIP(g, hipMalloc((void **)&r.flag, 4 * sizeof(uint32_t)));
  G_HIP(g, hipMemset(r.flag, 0, 4 * sizeof(uint32_t)));
  G_HIP(g, hipHostMalloc((void **)&r.flag_host, 4 * sizeof(uint32_t), hipHostMallocDefault));
  return WS_OK;
}

int ws_group_create_local(int n_ranks, const int *devices, ws_group **out) {
  if (!out || n_ranks < 1 || n_ranks > 1024) return WS_ERR_BAD_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return WS_ERR_NO_DEVICE;
  for (int r = 0; r < n_ranks; ++r)
    if (devices && (devices[r] < 0 || devices[r] >= count)) return WS_ERR_BAD_ARG;
  ws_group *g = new (std::nothrow) ws_group();
  if (!g) return WS_ERR_OOM;
  g->world = n_ranks;
  g->ranks.resize((size_t)n_ranks);
  int rc = WS_OK;
  for (int r = 0; r < n_ranks && rc == WS_OK; ++r) {
    g->ranks[(size_t)r].rank = r;
    g->ranks[(size_t)r].device = devices ? devices[r] : 0;
    rc = group_alloc_rank(g, g->ranks[(size_t)r]);
  }
  // neighbours on different devices copy each other's rows directly
  for (int r = 0; r + 1 < n_ranks && rc == WS_OK; ++r) {
    const int a = g->ranks[(size_t)r].device, b = g->ranks[(size_t)r + 1].device;
    if (a == b) continue;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) { (void)hipSetDevice(a); (void)hipDeviceEnablePeerAccess(b, 0); }
    if (hipDeviceCanAccessPeer(&can, b, a) == hipSuccess && can) { (void)hipSetDevice(b); (void)hipDeviceEnablePeerAccess(a, 0); }
    (void)hipGetLastError();      // (already enabled: fine; not possible: the copies are staged by the runtime)
  }
  if (rc != WS_OK) { ws_group_destroy(g); return rc; }
  *out = g;
  return WS_OK;
}

int ws_group_rccl_unique_id(void *id) {
  if (!id) return WS_ERR_BAD_ARG;
  static_assert(sizeof(ncclUniqueId) == WS_RCCL_ID_BYTES, "the id travels as WS_RCCL_ID_BYTES opaque bytes");
  RcclApi *n = rccl();
  if (!n->lib) return WS_ERR_RCCL;
  ncclUniqueId uid;
  if (n->GetUniqueId(&uid) != ncclSuccess) return WS_ERR_RCCL;
  std::memcpy(id, &uid, sizeof uid);
  return WS_OK;
}

int ws_group_create_rccl(int device, int rank, int world, const void *id, ws_group **out) {
  if (!out || !id || world < 1 || rank < 0 || rank >= world) return WS_ERR_BAD_ARG;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return WS_ERR_NO_DEVICE;
  if (device < 0 || device >= count) return WS_ERR_BAD_ARG;
  RcclApi *n = rccl();
  if (!n->lib) return WS_ERR_RCCL;
  ws_group *g = new (std::nothrow) ws_group();
  if (!g) return WS_ERR_OOM;
  g->is_rccl = true;
  g->world = world;
  g->first_local = rank;
  g->ranks.resize(1);
  g->ranks[0].rank = rank;
  g->ranks[0].device = device;
  int rc = group_alloc_rank(g, g->ranks[0]);
  if (rc == WS_OK) {
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof uid);
    if (hipSetDevice(device) != hipSuccess || n->CommInitRank(&g->comm, world, uid, rank) != ncclSuccess) { g->comm = nullptr; rc = WS_ERR_RCCL; }
  }
  if (rc != WS_OK) { ws_group_destroy(g); return rc; }
  *out = g;
  return WS_OK;
}

void ws_group_destroy(ws_group *g) {
  if (!g) return;
  if (g->comm) (void)rccl()->CommDestroy(g->comm);
  for (Rank &r : g->ranks) {
    (void)hipSetDevice(r.device);
    if (r.ctx) { (void)ws_ctx_synchronize(r.ctx); }
    static_cast<RankBuffers &>(r) = RankBuffers();      // frees every buffer, here: on the rank's device, before its context goes
    if (r.flag) (void)hipFree(r.flag);
    if (r.flag_host) (void)hipHostFree(r.flag_host);
    if (r.ctx) ws_ctx_destroy(r.ctx);
  }
  delete g;
}

int ws_group_info(const ws_group *g, int *world, int *n_local, int *first_local) {
  if (!g) return WS_ERR_BAD_ARG;
  if (world) *world = g->world;
  if (n_local) *n_local = (int)g->ranks.size();
  if (first_local) *first_local = g->first_local;
  return WS_OK;
}

const char *ws_group_last_error(const ws_group *g) {
  if (!g) return rccl()->lib ? "null group" : rccl()->why.c_str();
  return g->err.c_str();
}

// every rank's held plane of the cut: rank * 100000 + the word's index in the field where it owns, 0xDEAD in its halo
static int selftest_gather_owned(ws_group *g, Rank &me, const TileCut &cut) {
  GatherLayout l;
  if (!gather_layout(cut, &l)) return gfail(g, WS_ERR_BAD_ARG, "selftest: tile grid");
  const TilePlace &t = l.place[(size_t)me.rank];
  const size_t fw = cut.field_w, n = cut.field_h * fw;
  std::vector<uint32_t> plane(t.h * t.w, 0xDEADu), full(n);
  for (size_t r = t.r0; r < t.r1; ++r)
    for (size_t q = t.c0; q < t.c1; ++q) plane[(r - t.lo) * t.w + (q - t.clo)] = (uint32_t)me.rank * 100000u + (uint32_t)(r * fw + q);
  int rc;
  if ((rc = grow(g, me.labels, plane.size() * sizeof(uint32_t)))) return rc;
  if (me.rank == 0 && (rc = grow(g, me.full_keys, n * sizeof(uint32_t)))) return rc;
  hipStream_t s = me.ctx->stream;
  G_HIP(g, hipMemcpyAsync(me.labels.p, plane.data(), plane.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
  G_HIP(g, hipStreamSynchronize(s));
  Exchange x{g, me};
  if ((rc = x.gather_owned(cut, (const uint32_t *)me.labels.p, (uint32_t *)me.full_keys.p)) || me.rank != 0) return rc;
  G_HIP(g, hipMemcpyAsync(full.data(), me.full_keys.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
  G_HIP(g, hipStreamSynchronize(s));
  for (const TilePlace &p : l.place)
    for (size_t r = p.r0; r < p.r1; ++r)
      for (size_t q = p.c0; q < p.c1; ++q)
        if (full[r * fw + q] != (uint32_t)(&p - l.place.data()) * 100000u + (uint32_t)(r * fw + q))
          return gfail(g, g->is_rccl ? WS_ERR_RCCL : WS_ERR_HIP, "selftest: the gather of owned rows or rectangles on rank 0 delivered wrong words");
  return WS_OK;
}

int ws_group_selftest(ws_group *g) {
  if (!g) return WS_ERR_BAD_ARG;
  const size_t w = 1024, h = 4;
  return for_local_ranks(g, [&](Rank &me) -> int {
    G_HIP(g, hipSetDevice(me.device));
    int rc;
    const int world = g->world, up = me.rank > 0, down = me.rank < world - 1;
    if ((rc = grow(g, me.keys, h * w * sizeof(uint32_t)))) return rc;
    if ((rc = grow(g, me.recv, 2 * w * sizeof(uint32_t)))) return rc;
    if ((rc = grow(g, me.table, (size_t)world * w * sizeof(uint32_t)))) return rc;
    std::vector<uint32_t> host(h * w), got(std::max<size_t>(2 * w, (size_t)world * w));
    for (size_t i = 0; i < h * w; ++i) host[i] = (uint32_t)me.rank * 100000u + (uint32_t)i;      // row r of rank k: k * 100000 + r * w ...
    hipStream_t s = me.ctx->stream;
    G_HIP(g, hipMemcpyAsync(me.keys.p, host.data(), h * w * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    G_HIP(g, hipStreamSynchronize(s));
    Exchange x{g, me};
    TilePlace block;      // a block of h rows with a halo row on every side that has a neighbour
    block.h = h; block.w = w;
    block.nb[0] = up ? me.rank - 1 : -1; block.nb[1] = down ? me.rank + 1 : -1;
    if ((rc = x.swap((const uint32_t *)me.keys.p, block))) return rc;
    G_HIP(g, hipMemcpyAsync(got.data(), me.recv.p, 2 * w * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    G_HIP(g, hipStreamSynchronize(s));
    // the upper neighbour's last OWNED row (its row h - 2 if it has a lower neighbour -- it has: me), the lower one's first owned row
    for (size_t i = 0; i < w; ++i) {
      if (up && got[i] != (uint32_t)(me.rank - 1) * 100000u + (uint32_t)((h - 2) * w + i)) return gfail(g, g->is_rccl ? WS_ERR_RCCL : WS_ERR_HIP, "selftest: halo swap (from above) delivered wrong words");
      if (down && got[w + i] != (uint32_t)(me.rank + 1) * 100000u + (uint32_t)(w + i)) return gfail(g, g->is_rccl ? WS_ERR_RCCL : WS_ERR_HIP, "selftest: halo swap (from below) delivered wrong words");
    }
    uint32_t v = 0;
    if ((rc = x.reduce_host((uint32_t)me.rank + 7u, true, &v))) return rc;
    if (v != (uint32_t)world + 6u) return gfail(g, g->is_rccl ? WS_ERR_RCCL : WS_ERR_HIP, "selftest: max-reduce returned a wrong word");
    if ((rc = x.reduce_host((uint32_t)me.rank + 7u, false, &v))) return rc;
    if (v != 7u) return gfail(g, g->is_rccl ? WS_ERR_RCCL : WS_ERR_HIP, "selftest: min-reduce returned a wrong word");
    if ((rc = x.gather((const uint32_t *)me.keys.p + w, w, (uint32_t *)me.table.p))) return rc;
    G_HIP(g, hipMemcpyAsync(got.data(), me.table.p, (size_t)world * w * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    G_HIP(g, hipStreamSynchronize(s));
    for (int k = 0; k < world; ++k)
      for (size_t i = 0; i < w; ++i)
        if (got[(size_t)k * w + i] != (uint32_t)k * 100000u + (uint32_t)(w + i)) return gfail(g, g->is_rccl ? WS_ERR_RCCL : WS_ERR_HIP, "selftest: all-gather delivered wrong words");
    // the gather of what every rank owns on rank 0 (transform_to_list of a tiled field): row blocks of 2 * world + 1 rows, and
    // 1 x world tiles of a field of 3 x (2 * world + 1) words
    if ((rc = selftest_gather_owned(g, me, TileCut{2 * (size_t)world + 1, w, world, 1}))) return rc;
    if ((rc = selftest_gather_owned(g, me, TileCut{3, 2 * (size_t)world + 1, 1, world}))) return rc;
    return WS_OK;
  });
}

// ---- a field in row blocks, and in py x px tiles: device-resident blocks -------------------------------------------------------
int ws_segment_tiled_device(ws_group *g, size_t field_h, size_t w, size_t n_seeds_total, const ws_tile_block *blocks, const ws_options *opt,
                            int merging, uint32_t *exchange_rounds) {
  return segment_tiled_device(g, row_cut(g, field_h, w), n_seeds_total, blocks, opt, merging, exchange_rounds);
}

int ws_segment_tiled2d_device(ws_group *g, size_t field_h, size_t field_w, int py, int px, size_t n_seeds_total, const ws_tile_block2d *blocks,
                              const ws_options *opt, int merging, uint32_t *exchange_rounds) {
  return segment_tiled_device(g, TileCut{field_h, field_w, py, px}, n_seeds_total, blocks, opt, merging, exchange_rounds);
}

int ws_transform_to_list_tiled_device(ws_group *g, size_t field_h, size_t w, size_t n_seeds_total, const ws_tile_block *blocks,
                                      const ws_options *opt, int merging, ws_lake *d_lakes, size_t cap, size_t *n_lakes,
                                      uint64_t *offsets, uint64_t *uncoloured, uint32_t *exchange_rounds) {
  return lists_tiled_device(g, row_cut(g, field_h, w), n_seeds_total, blocks, opt, merging, d_lakes, cap, n_lakes, offsets, uncoloured, exchange_rounds);
}

int ws_transform_to_list_tiled2d_device(ws_group *g, size_t field_h, size_t field_w, int py, int px, size_t n_seeds_total,
                                        const ws_tile_block2d *blocks, const ws_options *opt, int merging, ws_lake *d_lakes, size_t cap,
                                        size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured, uint32_t *exchange_rounds) {
  return lists_tiled_device(g, TileCut{field_h, field_w, py, px}, n_seeds_total, blocks, opt, merging, d_lakes, cap, n_lakes, offsets, uncoloured,
                            exchange_rounds);
}

int ws_merge_tree_tiled_device(ws_group *g, size_t field_h, size_t w, size_t n_seeds_total, const ws_tile_block *blocks, const ws_options *opt,
                               const void *d_weight, int weight_dtype, size_t weight_row_stride, ws_tree_node *d_tree, ws_lake_stats *d_stats,
                               uint32_t *exchange_rounds) {
  return tree_tiled_device(g, row_cut(g, field_h, w), n_seeds_total, blocks, opt, TreeWeights{d_weight, weight_dtype, weight_row_stride}, d_tree, d_stats,
                           exchange_rounds);
}

int ws_merge_tree_tiled2d_device(ws_group *g, size_t field_h, size_t field_w, int py, int px, size_t n_seeds_total, const ws_tile_block2d *blocks,
                                 const ws_options *opt, const void *d_weight, int weight_dtype, size_t weight_row_stride, ws_tree_node *d_tree,
                                 ws_lake_stats *d_stats, uint32_t *exchange_rounds) {
  return tree_tiled_device(g, TileCut{field_h, field_w, py, px}, n_seeds_total, blocks, opt, TreeWeights{d_weight, weight_dtype, weight_row_stride}, d_tree,
                           d_stats, exchange_rounds);
}

// ---- ... host buffers in and out: a job and a call ------------------------------------------------------------------------------
int ws_segment_tiled(ws_group *g, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                     const ws_options *opt, int merging, uint64_t *out_labels, uint32_t *exchange_rounds) {
  TiledHostJob J{img, h, w, stride, seeds_rc, n_seeds, opt};
  J.merging = merging;
  J.out_labels = out_labels;
  return run_host_job(g, J, exchange_rounds);
}

// ... in py x px tiles: every seed with its colour (index + 1), tiled2d_rank, the owned rectangle of out_labels
int ws_segment_tiled2d(ws_group *g, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                       const ws_options *opt, int py, int px, int merging, uint64_t *out_labels, uint32_t *exchange_rounds) {
  TiledHostJob J{img, h, w, stride, seeds_rc, n_seeds, opt};
  J.tiles = true; J.py = py; J.px = px;
  J.merging = merging;
  J.out_labels = out_labels;
  return run_host_job(g, J, exchange_rounds);
}

// transform_to_list of a host field over the ranks of the group; the records go to the caller's host buffer from rank 0's device
int ws_transform_to_list_tiled(ws_group *g, int merging, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc,
                               size_t n_seeds, const ws_options *opt, ws_lake *lakes, size_t cap, size_t *n_lakes, uint64_t *offsets,
                               uint64_t *uncoloured, uint32_t *exchange_rounds) {
  if (!g) return WS_ERR_BAD_ARG;
  if (!n_lakes || !offsets || !uncoloured || (!lakes && cap)) return gfail(g, WS_ERR_BAD_ARG, "null pointer");
  *n_lakes = 0;
  TiledHostJob J{img, h, w, stride, seeds_rc, n_seeds, opt};
  J.want = TiledHostJob::LISTS;
  J.merging = merging;
  J.lists = HostLists{lakes, cap, n_lakes, offsets, uncoloured};
  return run_host_job(g, J, exchange_rounds);
}

// merge_tree (and the catalogue) of a host field over the ranks of the group; the records go to the caller's host buffers
int ws_merge_tree_tiled(ws_group *g, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                        const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride, ws_tree_node *tree,
                        ws_lake_stats *stats, uint32_t *exchange_rounds) {
  if (!g) return WS_ERR_BAD_ARG;
  if (!tree && g->first_local == 0) return gfail(g, WS_ERR_BAD_ARG, "null pointer");
  TiledHostJob J{img, h, w, stride, seeds_rc, n_seeds, opt};
  J.want = TiledHostJob::TREE;
  J.tree = HostTree{tree, stats, TreeWeights{weight, weight_dtype, weight_row_stride}};
  return run_host_job(g, J, exchange_rounds);
}

// ---- a batch of independent slices ----------------------------------------------------------------------------------------------

int ws_segment_batch_group(ws_group *g, size_t h, size_t w, const ws_batch_part *parts, const ws_options *opt, size_t *failed_rank,
                           size_t *failed_slice) {
  if (failed_rank) *failed_rank = 0;
  if (failed_slice) *failed_slice = 0;
  int rc = check_group_call(g, opt);
  if (rc) return rc;
  if (!parts) return gfail(g, WS_ERR_BAD_ARG, "parts pointer is null");
  std::vector<size_t> bad(g->ranks.size(), 0);
  std::vector<int> rcs(g->ranks.size(), WS_OK);
  rc = for_local_ranks(g, [&](Rank &me) -> int {
    const size_t i = (size_t)(me.rank - g->first_local);
    const ws_batch_part &p = parts[i];
    if (p.n_slices == 0) return WS_OK;
    rcs[i] = ws_segment_batch_device(me.ctx, p.d_cube, p.n_slices, h, w, w, h * w, p.d_seeds_rc, p.seed_offsets, opt, p.d_labels, &bad[i]);
    if (rcs[i] != WS_OK) return gfail(g, rcs[i], std::string("rank ") + std::to_string(me.rank) + ": ws_segment_batch_device: " + ws_last_error(me.ctx));
    return WS_OK;
  });
  for (size_t i = 0; i < rcs.size(); ++i)
    if (rcs[i] != WS_OK) { if (failed_rank) *failed_rank = (size_t)g->first_local + i; if (failed_slice) *failed_slice = bad[i]; break; }
  return rc;
}

// A cube of independent slices in HOST memory over the ranks of a group: rank r takes the slices [n r / world, n (r + 1) / world)
// and runs them as ws_segment_batch on its own context -- four lanes per device, every device on its own link to the host.
// A process drives its local ranks only (an RCCL group: its one rank's block of slices; the cube pointer is that process's).
int ws_segment_batch_host(ws_group *g, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                          const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, uint64_t *out_labels,
                          size_t *n_seeds, size_t *failed_slice) {
  if (failed_slice) *failed_slice = 0;
  int rc = check_group_call(g, opt);
  if (rc) return rc;
  if (n_slices == 0) return WS_OK;
  if (!out_labels || (!cube && h * w) || (seeds_rc && !seed_offsets)) return gfail(g, WS_ERR_BAD_ARG, "null pointer");
  const size_t e = opt->edge_correction ? 2 : 0, plane = (h + e) * (w + e);
  const size_t world = (size_t)g->world;
  std::vector<size_t> bad(g->ranks.size(), 0);
  std::vector<int> rcs(g->ranks.size(), WS_OK);
  rc = for_local_ranks(g, [&](Rank &me) -> int {
    const size_t i = (size_t)(me.rank - g->first_local);
    const size_t k0 = n_slices * (size_t)me.rank / world, k1 = n_slices * ((size_t)me.rank + 1) / world;
    if (k1 == k0) return WS_OK;
    // (the rank's seed offsets as they are: ws_segment_batch only looks at differences and at seeds_rc + 2 * offset)
    rcs[i] = ws_segment_batch(me.ctx, cube + k0 * slice_stride, k1 - k0, h, w, row_stride, slice_stride, seeds_rc, seeds_rc ? seed_offsets + k0 : nullptr,
                              opt, out_labels + k0 * plane, n_seeds ? n_seeds + k0 : nullptr, &bad[i]);
    bad[i] += k0;
    if (rcs[i] != WS_OK) return gfail(g, rcs[i], std::string("rank ") + std::to_string(me.rank) + ": ws_segment_batch: " + ws_last_error(me.ctx));
    return WS_OK;
  });
  for (size_t i = 0; i < rcs.size(); ++i)      // ranks hold increasing blocks of slices: the first failing rank has the lowest failing slice
    if (rcs[i] != WS_OK) { if (failed_slice) *failed_slice = bad[i]; break; }
  return rc;
}

}  // extern "C"
