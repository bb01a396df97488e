// ws_lists.hip -- the merging drivers (lib.rs:1328-1522) and transform_to_list (lib.rs:1551-1561, 1837-1847): per-level
// unions over seed colours, lake areas and sparse lake records (kernels: ws_merge.hip the level loop, ws_merge_final.hip the
// final labels alone, ws_merge_tree.hip history planes, merge tree and lake statistics; wrappers: ws_merge.hpp).
#include "ws_ctx.hpp"
#include "ws_level_plan.hpp"

using namespace wsapi;

namespace {

// mflags layout (u64 words): per-level histograms / cursors, lake cursor, per-level lake offsets
constexpr int MF_HIST_PX = 0;
constexpr int MF_HIST_ED = NLEVELS;
constexpr int MF_CUR_PX = 2 * NLEVELS;
constexpr int MF_CUR_ED = 3 * NLEVELS;
constexpr int MF_HOOKED = 5 * NLEVELS + 16;               // NLEVELS u32 counters (one per level: no memset between levels)
constexpr int MF_LAKE_COUNT = 6 * NLEVELS + 16;           // NLEVELS u64 per-level record counters
constexpr int MF_OFF_PX = 8 * NLEVELS + 24;               // NLEVELS + 1 bucket bounds of the arriving pixels (k_level_offsets)
constexpr int MF_OFF_ED = MF_OFF_PX + NLEVELS + 1;        // ... and of the crossing edges
constexpr int MF_WORDS = MF_OFF_ED + NLEVELS + 1;
constexpr uint32_t LIST_GROUP = 16;                       // levels per host copy of lake records (16 groups: kern_ev has 64)

// Segmenting result (stamps + colours) -> per-level buckets of arriving pixels and crossing edges, all on the device:
// histograms, their prefix sums (the bucket bounds, which only kernels ever read), scatter.  Workspace: 4 B per arriving
// pixel + 8 B per crossing edge, at most 20 B per pixel of the plane (one arrival per pixel, two crossing edges -- right,
// down -- per pixel; a random field is close to that).  A context whose buffers already hold the worst case reads
// nothing back; otherwise the two totals (16 bytes) are read once and the buffers sized by them, so that a sparse or
// partly flooded plane near the 2^32-pixel limit does not ask for 80 GB it will not use.
// slice_base (nullable): the plane is a stack of slices of slice_h rows (level_hist)
int build_buckets(ws_ctx *c, const uint32_t *keys, const uint32_t *seg_labels, int ph, int pw, int slice_h = 0, const uint32_t *slice_base = nullptr) {
  int rc;
  const size_t n = (size_t)ph * pw;
  if ((rc = ensure(c, c->mflags, MF_WORDS * sizeof(uint64_t)))) return rc;
  u64c *mf = (u64c *)c->mflags.p;
  HIP_TRY(c, hipMemsetAsync(mf, 0, MF_WORDS * sizeof(uint64_t), c->stream));
  HIP_TRY(c, level_hist(c->stream, keys, seg_labels, ph, pw, mf + MF_HIST_PX, mf + MF_HIST_ED, slice_h, slice_base));
  HIP_TRY(c, level_offsets(c->stream, mf + MF_HIST_PX, mf + MF_HIST_ED, mf + MF_OFF_PX, mf + MF_OFF_ED, mf + MF_CUR_PX, mf + MF_CUR_ED));
  size_t need_px = (n ? n : 1) * sizeof(uint32_t), need_ed = (n ? 2 * n : 1) * sizeof(uint2);
  if (c->px_items.cap < need_px || c->edge_items.cap < need_ed) {
    unsigned long long totals[2] = {0, 0};
    HIP_TRY(c, hipMemcpyAsync(&totals[0], mf + MF_OFF_PX + NLEVELS, sizeof(u64c), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipMemcpyAsync(&totals[1], mf + MF_OFF_ED + NLEVELS, sizeof(u64c), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    need_px = std::min<size_t>(need_px, std::max<size_t>(totals[0], 1) * sizeof(uint32_t));
    need_ed = std::min<size_t>(need_ed, std::max<size_t>(totals[1], 1) * sizeof(uint2));
  }
  if ((rc = ensure(c, c->px_items, need_px))) return rc;
  if ((rc = ensure(c, c->edge_items, need_ed))) return rc;
  HIP_TRY(c, level_scatter(c->stream, keys, seg_labels, ph, pw, mf + MF_CUR_PX, mf + MF_CUR_ED,
                           (uint32_t *)c->px_items.p, (uint2 *)c->edge_items.p, slice_h, slice_base));
  return WS_OK;
}

int ensure_uf(ws_ctx *c, size_t n_colours) {
  int rc;
  if ((rc = ensure(c, c->uf_parent, n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->uf_size, n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->uf_hooked, n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->uf_death, n_colours * sizeof(uint32_t)))) return rc;
  return WS_OK;
}

// workgroups of the per-level kernels: their buckets' sizes are only known on the device, so the grid follows the plane
// (an even spread would be pixels / 255 per level) and the kernels stride
unsigned level_grid(size_t n_px) { return (unsigned)std::min<size_t>(std::max<size_t>(n_px / (256 * 64), 8), 2048); }

// A job that no entry point builds is refused before anything runs (level_job_refusal, ws_level_plan.hpp)
int check_job(ws_ctx *c, const LevelJob &job) {
  if (const char *why = level_job_refusal(job)) return fail(c, WS_ERR_BAD_ARG, why);
  return WS_OK;
}

// What the stages of merge_host hand on to each other (one per call, never copied: opt may point into it)
struct LevelRun {
  ws_options plain{};                  // the arrival form's options: the plane as it stands
  const ws_options *opt = nullptr;
  size_t ph = 0, pw = 0, n = 0;        // the (padded) plane
  const uint32_t *keys = nullptr, *seg = nullptr;      // the flood's arrival stamps and segmenting labels
  LevelPlan plan;
  uint32_t levels = 0;
  unsigned grid = 0;                   // workgroups of the per-level kernels
  unsigned emit_grid = 0;              // ... and of the live-list walk
  uint64_t *records = nullptr;         // (colour, area) pairs on the device: the context's buffer, or the caller's
  const uint8_t *himg = nullptr;       // the image the hook is shown
  std::vector<uint64_t> bounds;        // bucket bounds of the arriving pixels and of the crossing edges
};

// The hook of level l: the level's plane to the host (device state current on c->stream), then the caller's function
int level_hook(ws_ctx *c, const LevelJob &job, const LevelRun &r, uint32_t l) {
  uint32_t *parent = (uint32_t *)c->uf_parent.p;
  uint64_t *d_out64 = (uint64_t *)c->out64.p;
  const size_t n = r.n;
  if (host_copy_in_chunks(c, n)) {      // the level's plane as u32 (in the u64 buffer, which that path leaves alone), widened by host threads
    if (job.merging) HIP_TRY(c, relabel_u32(c->stream, r.keys, r.seg, parent, (uint32_t *)d_out64, n, l));
    else HIP_TRY(c, snapshot_level_u32(c->stream, r.keys, r.seg, (uint32_t *)d_out64, n, l));
    if (int rc_copy = labels_to_host_u64(c, (const uint32_t *)d_out64, c->host64.data(), n)) return rc_copy;
  } else {
    if (job.merging) HIP_TRY(c, relabel_u64(c->stream, r.keys, r.seg, parent, d_out64, n, l));
    else HIP_TRY(c, snapshot_level(c->stream, r.keys, r.seg, d_out64, n, l));
    HIP_TRY(c, hipMemcpyAsync(c->host64.data(), d_out64, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
  }
  job.cb(job.user, (uint8_t)l, r.opt->max_water_level, r.himg, c->host64.data(), r.ph, r.pw);        // lib.rs:1510-1518
  return WS_OK;
}

// Levels [l0, l1) of the per-level driver shared by the merging hook, both transform_to_list flavours and transform_history:
// the plan's steps, level by level; launches only, unless a hook is called.
int level_range(ws_ctx *c, const LevelJob &job, const LevelRun &r, uint32_t l0, uint32_t l1) {
  uint32_t *parent = (uint32_t *)c->uf_parent.p, *size = (uint32_t *)c->uf_size.p, *death = (uint32_t *)c->uf_death.p;
  uint32_t *hooked = r.plan.hooked_list ? (uint32_t *)c->uf_hooked.p : nullptr;
  uint2 *sd = (uint2 *)c->uf_sd.p;
  uint32_t *alive = (uint32_t *)c->alive.p;
  u64c *mf = (u64c *)c->mflags.p;
  uint32_t *hooked_count = (uint32_t *)(mf + MF_HOOKED);
  const uint32_t *px_items = (const uint32_t *)c->px_items.p;
  const uint2 *edge_items = (const uint2 *)c->edge_items.p;
  const size_t n_colours = job.n_seeds + 1, cap = job.cap;
  const unsigned grid = r.grid;
  for (uint32_t l = l0; l < l1; ++l)
    for (int i = 0; i < r.plan.n_steps; ++i)
      switch (r.plan.steps[i]) {
        case LevelStep::UNION_STAMPED:
          HIP_TRY(c, union_stamped_ranged(c->stream, edge_items, mf + MF_OFF_ED + l, grid, parent, death, (uint32_t *)c->uf_hook.p, l));
          break;
        case LevelStep::UNION_EMIT:
          HIP_TRY(c, union_emit(c->stream, edge_items, mf + MF_OFF_ED + l, grid, parent, hooked, hooked_count + l, death, l, size, n_colours, r.records, cap,
                                mf + MF_LAKE_COUNT));
          break;
        case LevelStep::UNION_EMIT_ALIVE:
          HIP_TRY(c, union_emit_alive(c->stream, edge_items, mf + MF_OFF_ED + l, grid, parent, hooked, hooked_count + l, sd, l, n_colours, alive,
                                      r.plan.split_emit ? 0u : r.emit_grid, r.records, cap, mf + MF_LAKE_COUNT));
          break;
        case LevelStep::EMIT_ALIVE_PREV:
          if (l > 0) HIP_TRY(c, emit_alive(c->stream, sd, n_colours, alive, r.emit_grid, r.records, cap, mf + MF_LAKE_COUNT, l - 1));
          break;
        case LevelStep::UNION_EDGES:
          HIP_TRY(c, union_edges_ranged(c->stream, edge_items, mf + MF_OFF_ED + l, grid, parent, hooked, hooked_count + l));
          break;
        case LevelStep::FOLD_ADD:
          HIP_TRY(c, fold_and_add_ranged(c->stream, hooked, hooked_count + l, px_items, mf + MF_OFF_PX + l, grid, parent, size));
          break;
        case LevelStep::FOLD_ADD_SD:
          HIP_TRY(c, fold_and_add_sd(c->stream, hooked, hooked_count + l, px_items, mf + MF_OFF_PX + l, grid, parent, sd));
          break;
        case LevelStep::EMIT_LAKES:      // offsets are prefix sums of the record counts, taken on the host
          HIP_TRY(c, emit_lakes(c->stream, parent, size, n_colours, r.records, cap, mf + MF_LAKE_COUNT, l));
          break;
        case LevelStep::HOOK:
          if (int rc = level_hook(c, job, r, l)) return rc;
          break;
      }
  return WS_OK;
}

// Records [from, end) of the device array d_rec into the host's `lakes`, on stream `on` (returns with the copy complete when the
// chunked road is taken; otherwise queued).  A piece of two million records and more (2048^2 planes on) crosses the bus as u32 --
// a colour and an area of a plane below 2^31 pixels fit -- and is widened into the caller's records by the host's threads
// (ws_hostcopy.hip; pieces of at most n records: the narrowed words borrow the u64 label buffer, n x 8 bytes).
// A piece that is too short for the chunked road must NOT go down it: labels_to_host_u64's other path widens into the very
// buffer the narrowed words sit in (and may reallocate it).  Such pieces are copied as they are.
int records_to_host(ws_ctx *c, const ws_lake *d_rec, ws_lake *lakes, size_t from, size_t end, size_t n, hipStream_t on) {
  const bool may_narrow = n < 0x80000000ull && c->out64.p && c->out64.cap >= n * sizeof(uint64_t);
  while (from < end) {
    const size_t piece = std::min<size_t>(end - from, n);
    if (may_narrow && 2 * piece >= ((size_t)1 << 22) && host_copy_in_chunks(c, 2 * piece)) {      // (from 2 M records a piece: below, starting the threads costs what they save -- 1024^2: 4.5 against 4.1 ms)
      HIP_TRY(c, narrow_words(on, (const uint64_t *)(d_rec + from), (uint32_t *)c->out64.p, 2 * piece));
      if (int rc = labels_to_host_u64(c, (const uint32_t *)c->out64.p, (uint64_t *)(lakes + from), 2 * piece, on)) return rc;
    } else {
      HIP_TRY(c, hipMemcpyAsync(lakes + from, d_rec + from, piece * sizeof(ws_lake), hipMemcpyDeviceToHost, on));
    }
    from += piece;
  }
  return WS_OK;
}

// ---- merge_host: the per-level driver, stage by stage (the job and its plan: ws_level_plan.hpp) --------------------------------------

// Source: the plane checked, the inputs on the device, the flood.  Yields r.keys and r.seg.
int level_source(ws_ctx *c, const LevelJob &job, LevelRun &r) {
  const bool from_arrival = job.source == LevelSource::ARRIVAL;
  r.opt = job.opt;
  if (from_arrival) { r.plain = *job.opt; r.plain.edge_correction = 0; r.opt = &r.plain; }      // the plane as it stands
  const ws_options *opt = r.opt;
  int rc = check_plane(c, job.h, job.w, job.stride, opt, &r.ph, &r.pw);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t ph = r.ph, pw = r.pw, n = ph * pw, n_seeds = job.n_seeds;
  r.n = n;
  const uint8_t *d_img = nullptr;
  size_t d_stride = 0;
  const uint32_t *d_seeds = nullptr;
  if (!from_arrival && (rc = ensure(c, c->labels, (n ? n : 1) * sizeof(uint32_t)))) return rc;
  if (job.source == LevelSource::HOST && (rc = ensure(c, c->out64, (n ? n : 1) * sizeof(uint64_t)))) return rc;
  stats_begin(c);
  switch (job.source) {
    case LevelSource::ARRIVAL:
      if (n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
      break;
    case LevelSource::DEVICE:
      if (n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
      d_img = job.d_img;
      d_stride = job.stride;
      if (opt->edge_correction && job.h * job.w == 0 && (rc = empty_image_block(c, &d_img, &d_stride, job.h, job.w))) return rc;
      if ((rc = shifted_seeds(c, job.d_seeds_rc, n_seeds, opt, &d_seeds))) return rc;
      break;
    case LevelSource::HOST:
      if ((rc = stage_inputs(c, job.img, job.h, job.w, job.stride, job.seeds_rc, n_seeds, opt, ph, pw, &d_img, &d_stride, &d_seeds))) return rc;
      break;
  }
  r.seg = from_arrival ? job.d_seg : (const uint32_t *)c->labels.p;
  // the flood itself is the segmenting one (same coloured set, same arrival stamps: lib.rs:1394-1438 == 1704-1748)
  if (!from_arrival && (rc = run_fused(c, d_img, d_stride, (int)ph, (int)pw, opt->max_water_level, d_seeds, n_seeds, (uint32_t *)c->labels.p, opt->edge_correction != 0))) return rc;
  r.keys = from_arrival ? job.d_keys : (const uint32_t *)c->keys.p;
  return WS_OK;
}

// Prepare: every buffer first, so that nothing moves once launches (or captured graphs) hold its address; then the buckets, the
// union-find and the mode's start state.
int level_prepare(ws_ctx *c, const LevelJob &job, LevelRun &r) {
  int rc;
  const size_t n = r.n, n_seeds = job.n_seeds;
  if ((rc = ensure_uf(c, n_seeds + 1))) return rc;
  if (r.plan.ensure_hook && (rc = ensure(c, c->uf_hook, (n_seeds + 1) * sizeof(uint32_t)))) return rc;
  if (r.plan.ensure_live) {
    if ((rc = ensure(c, c->uf_sd, (n_seeds + 1) * sizeof(uint2)))) return rc;
    if ((rc = ensure(c, c->alive, 2 * alive_list_words(n_seeds + 1) * sizeof(uint32_t)))) return rc;
  }
  if (job.lists() && !job.device_records() && (rc = ensure(c, c->lakes, (job.cap ? job.cap : 1) * 2 * sizeof(uint64_t)))) return rc;
  r.records = job.device_records() ? (uint64_t *)job.d_lakes : (uint64_t *)c->lakes.p;
  if ((rc = build_buckets(c, r.keys, r.seg, (int)r.ph, (int)r.pw, job.slice_h, job.d_slice_base))) return rc;
  HIP_TRY(c, uf_init(c->stream, (uint32_t *)c->uf_parent.p, (uint32_t *)c->uf_size.p, n_seeds + 1));
  r.himg = job.cb ? hook_image(c, job.img, job.h, job.w, job.stride, r.opt->edge_correction) : nullptr;
  if (job.cb) c->host64.resize(n ? n : 1);
  r.levels = (uint32_t)r.opt->max_water_level + 1;
  r.grid = level_grid(n);
  if (r.plan.sd_init) {
    r.emit_grid = (unsigned)std::min<size_t>(std::max<size_t>((n_seeds + 4095) / 4096, 1), 1024);
    HIP_TRY(c, sd_init(c->stream, (uint2 *)c->uf_sd.p, n_seeds + 1));
  } else if (r.plan.death_all_ones) {
    HIP_TRY(c, hipMemsetAsync(c->uf_death.p, 0xFF, (n_seeds + 1) * sizeof(uint32_t), c->stream));
  }
  return WS_OK;
}

// Run: all levels queued, in groups of LIST_GROUP.
// The level loop is ~3 launches of a few microseconds per level and has no host decision in it: a call that repeats
// the previous one's shape and buffers replays it as hipGraphs, one per group of LIST_GROUP levels (the groups' record
// copies still overlap the later groups).  The second such call captures, later ones replay.
int level_run(ws_ctx *c, const LevelJob &job, const LevelRun &r) {
  int rc;
  const size_t n = r.n, n_seeds = job.n_seeds;
  const uint32_t levels = r.levels;
  const bool want_list = job.lists();
  ws_ctx::ListKey key;
  // (the mode follows from merging, want_list, history, cb == null -- which capture needs anyway -- and n_colours against the
  // context's threshold, whose setter starts a new generation)
  key.merging = job.merging; key.want_list = want_list; key.levels = levels; key.n_colours = n_seeds + 1; key.n = n; key.cap = job.cap;
  key.records = r.records;
  key.keys = r.keys; key.seg = r.seg;
  key.slice_h = job.d_slice_base ? (size_t)job.slice_h : 0;
  key.history = job.history;      // (its unions are other kernels: never replay a history graph for lists or final labels, nor the reverse)
  key.generation = c->buffer_generation;
  const bool graph_able = level_capturable(job, c->stream != nullptr, c->graph_unusable, c->profiling, n);
  bool use_graphs = graph_able && key == c->list_seen_key;
  c->list_seen_key = graph_able ? key : ws_ctx::ListKey();
  if (!(use_graphs && key == c->list_graph_key)) {      // another shape: yesterday's graphs are of no use
    for (hipGraphExec_t &g : c->list_graphs) if (g) { (void)hipGraphExecDestroy(g); g = nullptr; }
    c->list_graph_key = use_graphs ? key : ws_ctx::ListKey();
  }
  if (tuning_env("WS_DEBUG_LIST"))
    std::fprintf(stderr, "[ws] merge_host: merging %d list %d cb %d levels %u colours %zu n %zu cap %zu gen %llu graph_able %d use_graphs %d fused %d\n",
                 (int)job.merging, (int)want_list, job.cb != nullptr, levels, n_seeds + 1, n, job.cap, (unsigned long long)key.generation, (int)graph_able,
                 (int)use_graphs, (int)(r.plan.tail != LevelTail::NONE));
  for (uint32_t g0 = 0; g0 < levels; g0 += LIST_GROUP) {
    const uint32_t g1 = std::min(g0 + LIST_GROUP, levels), gi = g0 / LIST_GROUP;
    bool done = false;
    if (use_graphs) {
      if (!c->list_graphs[gi]) {
        hipGraph_t graph = nullptr;
        if (hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal) == hipSuccess) {
          const int lrc = level_range(c, job, r, g0, g1);
          const hipError_t e2 = hipStreamEndCapture(c->stream, &graph);
          if (lrc == WS_OK && e2 == hipSuccess && hipGraphInstantiate(&c->list_graphs[gi], graph, nullptr, nullptr, 0) != hipSuccess) c->list_graphs[gi] = nullptr;
          if (graph) (void)hipGraphDestroy(graph);
        }
        if (!c->list_graphs[gi]) {      // nothing ran: plain launches from here on, for good
          (void)hipGetLastError();
          c->graph_unusable = true;
          use_graphs = false;
        }
      }
      if (c->list_graphs[gi]) {
        HIP_TRY(c, hipGraphLaunch(c->list_graphs[gi], c->stream));
        c->stats.graph_launches++;
        done = true;
      }
    }
    if (!done && (rc = level_range(c, job, r, g0, g1))) return rc;
    // a marker per group, so that the records of finished levels can travel to the host while later levels are computed
    if (want_list) HIP_TRY(c, hipEventRecord(c->kern_ev[gi], c->stream));
  }
  if (r.plan.tail == LevelTail::NONE) return WS_OK;
  // the fused modes' last level; and a marker behind it: there a group's last level is complete one launch later
  u64c *mf = (u64c *)c->mflags.p;
  if (r.plan.tail == LevelTail::EMIT_ALIVE)
    HIP_TRY(c, emit_alive(c->stream, (const uint2 *)c->uf_sd.p, n_seeds + 1, (uint32_t *)c->alive.p, r.emit_grid, r.records, job.cap, mf + MF_LAKE_COUNT,
                          levels - 1));
  else
    HIP_TRY(c, emit_lakes(c->stream, (uint32_t *)c->uf_parent.p, (const uint32_t *)c->uf_size.p, n_seeds + 1, r.records, job.cap, mf + MF_LAKE_COUNT, levels - 1,
                          (const uint32_t *)c->uf_death.p));
  HIP_TRY(c, hipEventRecord(c->kern_ev[(levels + LIST_GROUP - 1) / LIST_GROUP], c->stream));
  return WS_OK;
}

// Collect: the bucket bounds; and, for lists, group by group: wait for the group's marker, read its offsets, copy its records
// (155 MB at 1024^2: as long over PCIe as the levels take to compute, so the two are overlapped).
int level_collect(ws_ctx *c, const LevelJob &job, LevelRun &r) {
  int rc;
  u64c *mf = (u64c *)c->mflags.p;
  const uint32_t levels = r.levels;
  r.bounds.assign(2 * (NLEVELS + 1), 0);
  if (!job.lists()) {
    HIP_TRY(c, hipMemcpyAsync(r.bounds.data(), mf + MF_OFF_PX, 2 * (NLEVELS + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    return WS_OK;
  }
  uint64_t *offsets = job.offsets;
  offsets[0] = 0;
  size_t copied = 0;
  for (uint32_t g0 = 0; g0 < levels; g0 += LIST_GROUP) {
    const uint32_t g1 = std::min(g0 + LIST_GROUP, levels);
    HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->kern_ev[g0 / LIST_GROUP + r.plan.marker_shift], 0));
    HIP_TRY(c, hipMemcpyAsync(offsets + g0 + 1, mf + MF_LAKE_COUNT + g0, (g1 - g0) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->copy_stream));
    if (g0 == 0)      // the bucket bounds were final before the first level: they ride along with the first group
      HIP_TRY(c, hipMemcpyAsync(r.bounds.data(), mf + MF_OFF_PX, 2 * (NLEVELS + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, c->copy_stream));
    HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
    for (uint32_t l = g0; l < g1; ++l) offsets[l + 1] += offsets[l];      // counts -> offsets
    const size_t end = std::min<size_t>(offsets[g1], job.cap);
    if (!job.device_records() && end > copied) {      // (the records of this group travel while later levels are computed)
      if ((rc = records_to_host(c, (const ws_lake *)c->lakes.p, job.lakes, copied, end, r.n, c->copy_stream))) return rc;
      copied = end;
    }
  }
  HIP_TRY(c, hipStreamSynchronize(c->copy_stream));
  *job.n_lakes = offsets[levels];
  for (uint32_t l = 0; l < levels; ++l) job.uncoloured[l] = r.n - r.bounds[l + 1];                   // index 0 of lib.rs:630's vector
  return WS_OK;
}

// Final labels: the plane at max_water_level to the host
int level_labels(ws_ctx *c, const LevelJob &job, const LevelRun &r) {
  const size_t n = r.n;
  if (!job.out_labels || !n) return WS_OK;
  uint32_t *parent = (uint32_t *)c->uf_parent.p;
  uint64_t *d_out64 = (uint64_t *)c->out64.p;
  if (job.merging && !host_copy_in_chunks(c, n)) {
    HIP_TRY(c, relabel_u64(c->stream, r.keys, r.seg, parent, d_out64, n, r.opt->max_water_level));
    HIP_TRY(c, hipMemcpyAsync(job.out_labels, d_out64, n * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    return WS_OK;
  }
  // a large plane crosses the bus as u32 and is widened by host threads (ws_hostcopy.hip); the relabelled u32 plane of
  // the merging transform borrows the u64 buffer, which that path does not use
  if (job.merging) HIP_TRY(c, relabel_u32(c->stream, r.keys, r.seg, parent, (uint32_t *)d_out64, n, r.opt->max_water_level));
  return labels_to_host_u64(c, job.merging ? (const uint32_t *)d_out64 : r.seg, job.out_labels, n);
}

int level_epilogue(ws_ctx *c, const LevelJob &job, const LevelRun &r) {
  if (int rc = stats_end(c)) return rc;
  if (job.merging)
    for (uint32_t l = 0; l < r.levels; ++l) c->stats.merge_levels += r.bounds[NLEVELS + 1 + l + 1] > r.bounds[NLEVELS + 1 + l] ? 1u : 0u;
  if (job.lists() && *job.n_lakes > job.cap) return fail(c, WS_ERR_CAPACITY, "lake buffer too small");
  return WS_OK;
}

int merge_host(ws_ctx *c, const LevelJob &job) {
  if (!c) return WS_ERR_BAD_ARG;
  int rc = check_job(c, job);
  if (rc) return rc;
  static const bool split_emit = tuning_env("WS_TOLIST_SPLIT") != nullptr;      // A/B knob for tools/
  LevelRun r;
  r.plan = level_plan(job, c->live_list_min, split_emit);
  if ((rc = level_source(c, job, r))) return rc;
  if (r.plan.mode == LevelMode::NONE) return stats_end(c);      // the segmenting history is the flood's stamps and labels
  if ((rc = level_prepare(c, job, r))) return rc;
  if ((rc = level_run(c, job, r))) return rc;
  if ((rc = level_collect(c, job, r))) return rc;
  if ((rc = level_labels(c, job, r))) return rc;
  return level_epilogue(c, job, r);
}

void stats_add(ws_stats &a, const ws_stats &b) {
  a.relax_passes += b.relax_passes; a.resolve_passes += b.resolve_passes; a.sweep_steps += b.sweep_steps;
  a.merge_levels = std::max(a.merge_levels, b.merge_levels);
  a.tiles_run_relax += b.tiles_run_relax; a.tiles_run_resolve += b.tiles_run_resolve;
  a.ms_relax += b.ms_relax; a.ms_resolve += b.ms_resolve; a.ms_sweep += b.ms_sweep; a.ms_other += b.ms_other; a.ms_total += b.ms_total;
  a.launches_relax += b.launches_relax; a.launches_resolve += b.launches_resolve; a.launches_sweep += b.launches_sweep;
  a.relax_tile_iterations += b.relax_tile_iterations; a.graph_launches += b.graph_launches;
}

// The stack of ws_segment_batch_device (same conditions: see the header) for a batch whose every group of slices has a seed;
// groups of batch_max_px / plane slices.  false: the slice-by-slice loop takes the batch.
bool stackable(ws_ctx *c, size_t n_slices, size_t h, size_t w, size_t stride, size_t ph, size_t pw, const size_t *seed_offsets,
               const ws_options *opt, size_t *per_group) {
  static const bool off = tuning_env("WS_NO_BATCH_STACK") != nullptr || tuning_env("WS_NO_SEED_TABLES") != nullptr;      // A/B knobs for tools/
  const size_t plane = ph * pw;
  if (off || n_slices < 2 || pick_engine(opt) != WS_ENGINE_FUSED || !c->expect_sorted || (pw & 3) != 0 || plane == 0 ||
      plane % 128 != 0 || plane >= 0x40000000ull || stride != w || h * w == 0)
    return false;
  if (seed_offsets[n_slices] - seed_offsets[0] >= 0xFFFFFFFFull) return false;
  *per_group = std::max<size_t>(1, c->batch_max_px / plane);
  for (size_t k0 = 0; k0 < n_slices; k0 += *per_group)      // (a flood needs a seed)
    if (seed_offsets[std::min(k0 + *per_group, n_slices)] == seed_offsets[k0]) return false;
  return true;
}

// A batch that stacks, as its drivers hand it to flood_group
struct StackBatch {
  const uint8_t *d_cube = nullptr;
  size_t h = 0, stride = 0, ph = 0, pw = 0;
  const uint32_t *d_seeds_rc = nullptr;
  const size_t *seed_offsets = nullptr;
  const ws_options *opt = nullptr;
};

// The flood of slices [k0, k0 + g) as one stack (flood_stack) into `labels`; first (g + 1): every slice's first seed within the
// group.  true: flooded, and the statistics span is still OPEN -- the drivers differ in where they close it.  false: the flood
// failed or mispredicted; the span is closed, the error cleared, and the slice-by-slice loop repeats the work and names the slice.
bool flood_group(ws_ctx *c, const StackBatch &b, size_t k0, size_t g, uint32_t *labels, std::vector<uint32_t> &first) {
  const size_t s0 = b.seed_offsets[k0];
  first.resize(g + 1);
  for (size_t k = 0; k <= g; ++k) first[k] = (uint32_t)(b.seed_offsets[k0 + k] - s0);
  stats_begin(c);
  bool mispredicted = false;
  const int rc = flood_stack(c, b.d_cube + k0 * b.h * b.stride, b.stride, g, b.ph, b.pw, b.d_seeds_rc + 2 * s0, first.data(), b.opt, labels, &mispredicted);
  c->have_keys = false;      // the stamps are those of a stack, not of an image
  if (rc == WS_OK && !mispredicted) return true;
  (void)stats_end(c);
  c->err.clear();
  return false;
}

// The arrival-form job of a flooded stack of slices of ph rows: the per-level driver over the stack's numbering of colours
LevelJob stack_job(ws_ctx *c, bool merging, size_t g, size_t ph, size_t pw, size_t n_seeds, const ws_options *opt, const uint32_t *labels,
                   const uint32_t *d_base) {
  LevelJob job;
  job.merging = merging; job.h = g * ph; job.w = pw; job.stride = pw; job.n_seeds = n_seeds; job.opt = opt;
  job.source = LevelSource::ARRIVAL; job.d_keys = (const uint32_t *)c->keys.p; job.d_seg = labels;
  job.slice_h = (int)ph; job.d_slice_base = d_base;
  return job;
}

// The history job of a device-resident image: the flood and, merging, the stamped level loop; nothing leaves the context
LevelJob history_job_device(bool merging, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc, size_t n_seeds,
                            const ws_options *opt) {
  LevelJob job;
  job.merging = merging; job.h = h; job.w = w; job.stride = stride; job.n_seeds = n_seeds; job.opt = opt;
  job.source = LevelSource::DEVICE; job.d_img = d_img; job.d_seeds_rc = d_seeds_rc; job.history = true;
  return job;
}

// ... and of a host image
LevelJob history_job_host(bool merging, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                          const ws_options *opt) {
  LevelJob job;
  job.merging = merging; job.h = h; job.w = w; job.stride = stride; job.n_seeds = n_seeds; job.opt = opt;
  job.img = img; job.seeds_rc = seeds_rc; job.history = true;
  return job;
}

// ... and of a finished transform's planes (ws_merge_tree_from_arrival_device): no flood, the stamped level loop alone
LevelJob history_job_arrival(const uint32_t *d_keys, const uint32_t *d_seg, size_t h, size_t w, size_t n_seeds, const ws_options *opt) {
  LevelJob job;
  job.merging = true; job.h = h; job.w = w; job.stride = w; job.n_seeds = n_seeds; job.opt = opt;
  job.source = LevelSource::ARRIVAL; job.d_keys = d_keys; job.d_seg = d_seg; job.history = true;
  return job;
}

// ws_transform_to_list_batch_device on a stack: per group of slices, the flood of the stack (flood_stack), the per-level driver
// over the stack's numbering of colours (merge_host, arrival form: the bucketing adds the slice's base to every colour and pairs
// no pixels across a slice border), then the split of the group's records (level-major, stack colours) into the caller's
// slice-major layout in the slices' own colours.  *done = false: nothing was decided, the loop takes the batch.
int lists_batch_stacked(ws_ctx *c, bool merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t stride,
                        const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_lake *d_lakes, size_t cap,
                        size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured, bool *done) {
  *done = false;
  size_t ph, pw, per_group = 0;
  int rc = check_plane(c, h, w, stride, opt, &ph, &pw);
  if (rc) return rc;
  if (!stackable(c, n_slices, h, w, stride, ph, pw, seed_offsets, opt, &per_group)) return WS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t plane = ph * pw;
  const uint32_t levels = (uint32_t)opt->max_water_level + 1;
  ws_stats acc{};
  size_t need = 0;      // records of the groups so far; while need <= cap they are in d_lakes[0 .. need)
  std::vector<uint32_t> first;
  std::vector<uint64_t> goff(levels + 1), gunc(levels);
  std::vector<u64c> bins;
  StackBatch batch;
  batch.d_cube = d_cube; batch.h = h; batch.stride = stride; batch.ph = ph; batch.pw = pw; batch.d_seeds_rc = d_seeds_rc; batch.seed_offsets = seed_offsets; batch.opt = opt;
  for (size_t k0 = 0; k0 < n_slices; k0 += per_group) {
    const size_t g = std::min(per_group, n_slices - k0);
    const size_t s0 = seed_offsets[k0], ns = seed_offsets[k0 + g] - s0;
    const size_t gcap = need <= cap ? cap - need : 0, n_bins = g * levels;
    if ((rc = ensure(c, c->stack_labels, g * plane * sizeof(uint32_t)))) return rc;
    if ((rc = ensure(c, c->stack_records, std::max<size_t>(gcap, 1) * sizeof(ws_lake)))) return rc;
    if ((rc = ensure(c, c->stack_bins, (levels + 1 + n_bins + g * NLEVELS) * sizeof(u64c)))) return rc;
    uint32_t *labels = (uint32_t *)c->stack_labels.p;
    if (!flood_group(c, batch, k0, g, labels, first)) return WS_OK;      // the loop takes the batch
    if ((rc = stats_end(c))) return rc;
    stats_add(acc, c->stats);
    const uint32_t *d_base = stacked_first(c, ns);
    u64c *d_off = (u64c *)c->stack_bins.p, *d_bins = d_off + levels + 1, *d_hist = d_bins + n_bins;
    HIP_TRY(c, hipMemsetAsync(d_bins, 0, (n_bins + g * NLEVELS) * sizeof(u64c), c->stream));
    HIP_TRY(c, slice_arrivals(c->stream, (const uint32_t *)c->keys.p, plane, g, d_hist));
    size_t got = 0;
    LevelJob job = stack_job(c, merging, g, ph, pw, ns, opt, labels, d_base);
    job.d_lakes = (ws_lake *)c->stack_records.p; job.cap = gcap; job.n_lakes = &got; job.offsets = goff.data(); job.uncoloured = gunc.data();
    rc = merge_host(c, job);
    if (rc != WS_OK && rc != WS_ERR_CAPACITY) return rc;
    stats_add(acc, c->stats);
    need += got;
    if (rc == WS_ERR_CAPACITY || need > cap) {      // counted, not written: the caller learns how many records to make room for
      c->err.clear();
      continue;
    }
    // counts per (slice, level) -> the bins' first records in the caller's layout, which the scatter takes as its cursors.
    // A bin holds at most one record per colour of its slice; segmenting lists that have ALL of them (every seed owns its pixel
    // from level 0 on: the usual case) are known without a pass over the records.
    HIP_TRY(c, hipMemcpyAsync(d_off, goff.data(), (levels + 1) * sizeof(u64c), hipMemcpyHostToDevice, c->stream));
    const bool full = !merging && got == (size_t)levels * ns;
    if (!full)
      HIP_TRY(c, split_records(c->stream, false, (const uint64_t *)c->stack_records.p, got, d_off, levels, d_base, (uint32_t)g, d_bins, nullptr));
    bins.resize(n_bins + g * NLEVELS);
    HIP_TRY(c, hipMemcpyAsync(bins.data(), d_bins, bins.size() * sizeof(u64c), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (full)
      for (size_t k = 0; k < g; ++k)
        for (uint32_t l = 0; l < levels; ++l) bins[k * levels + l] = first[k + 1] - first[k];
    u64c at = need - got;
    for (size_t b = 0; b < n_bins; ++b) {
      const u64c count = bins[b];
      offsets[k0 * levels + b] = at;
      bins[b] = at;
      at += count;
    }
    if (at != need) return fail(c, WS_ERR_HIP, "internal: the split of the stack's records lost some");
    for (size_t k = 0; k < g; ++k) {      // index 0 of lib.rs:630's vector: the slice's pixels not yet coloured
      u64c arrived = 0;
      for (uint32_t l = 0; l < levels; ++l) {
        arrived += bins[n_bins + k * NLEVELS + l];
        uncoloured[(k0 + k) * levels + l] = plane - arrived;
      }
    }
    HIP_TRY(c, hipMemcpyAsync(d_bins, bins.data(), n_bins * sizeof(u64c), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, split_records(c->stream, true, (const uint64_t *)c->stack_records.p, got, d_off, levels, d_base, (uint32_t)g, d_bins,
                             (uint64_t *)d_lakes));
    HIP_TRY(c, hipStreamSynchronize(c->stream));      // `bins` and `goff` are the next group's
  }
  offsets[n_slices * levels] = need;
  *n_lakes = need;
  c->stats = acc;
  *done = true;
  if (need > cap) return fail(c, WS_ERR_CAPACITY, "lake buffer too small");
  return WS_OK;
}

// ws_merge_batch_device on a stack: the flood of each group of slices into the caller's labels, then the unions of the final
// level over the stack's numbering of colours and a relabel back to every slice's own (merge_stack).
int merge_batch_stacked(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc,
                        const size_t *seed_offsets, const ws_options *opt, uint32_t *d_labels, bool *done) {
  *done = false;
  size_t ph, pw, per_group = 0;
  int rc = check_plane(c, h, w, stride, opt, &ph, &pw);
  if (rc) return rc;
  if (!stackable(c, n_slices, h, w, stride, ph, pw, seed_offsets, opt, &per_group)) return WS_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t plane = ph * pw;
  ws_stats acc{};
  std::vector<uint32_t> first;
  StackBatch batch;
  batch.d_cube = d_cube; batch.h = h; batch.stride = stride; batch.ph = ph; batch.pw = pw; batch.d_seeds_rc = d_seeds_rc; batch.seed_offsets = seed_offsets; batch.opt = opt;
  for (size_t k0 = 0; k0 < n_slices; k0 += per_group) {
    const size_t g = std::min(per_group, n_slices - k0);
    const size_t ns = seed_offsets[k0 + g] - seed_offsets[k0];
    if ((rc = ensure_uf(c, ns + 1))) return rc;
    uint32_t *labels = d_labels + k0 * plane;
    if (!flood_group(c, batch, k0, g, labels, first)) return WS_OK;      // the loop takes the batch
    HIP_TRY(c, uf_init(c->stream, (uint32_t *)c->uf_parent.p, (uint32_t *)c->uf_size.p, ns + 1));
    {
      Span sp(c, KC_OTHER);
      HIP_TRY(c, merge_stack(c->stream, labels, (int)ph, (int)pw, g, stacked_first(c, ns), (uint32_t *)c->uf_parent.p, ns + 1));
    }
    if ((rc = stats_end(c))) return rc;
    stats_add(acc, c->stats);
  }
  c->stats = acc;
  c->stats.merge_levels = 1;
  *done = true;
  return WS_OK;
}

// the checks the batch entry points share (as ws_segment_batch_device's)
int check_batch(ws_ctx *c, size_t n_slices, size_t h, size_t row_stride, size_t slice_stride, const size_t *seed_offsets,
                const ws_options *opt) {
  if (n_slices && !seed_offsets) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (!opt) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int v = ws_options_validate(opt)) return fail(c, v, ws_strerror(v));
  if (n_slices > 1 && slice_stride < h * row_stride) return fail(c, WS_ERR_BAD_ARG, "slice_stride < h * row_stride");
  for (size_t k = 0; k < n_slices; ++k)
    if (seed_offsets[k + 1] < seed_offsets[k]) return fail(c, WS_ERR_BAD_ARG, "seed_offsets must not decrease");
  return WS_OK;
}

// ---- transform_history (lib.rs:1233-1237, 1538-1549, 1824-1835) for a list of levels ------------------------------------------------

constexpr size_t HISTORY_SCRATCH_BYTES = (size_t)256 << 20;      // the host form's u32 planes on the device, at most, per chunk of levels

// n_planes planes of n u32 words, contiguous on the device, into the host's u64 planes: in ONE labels_to_host_u64 where the host
// threads widen (host_copy_in_chunks), else plane by plane, widened on the device in the u64 buffer the context holds for one plane
int planes_to_host(ws_ctx *c, const uint32_t *src, uint64_t *dst, size_t n_planes, size_t n) {
  if (host_copy_in_chunks(c, n_planes * n)) return labels_to_host_u64(c, src, dst, n_planes * n);
  for (size_t i = 0; i < n_planes; ++i)
    if (int rc = labels_to_host_u64(c, src + i * n, dst + i * n, n)) return rc;
  return WS_OK;
}

// what both forms check before anything runs; *n_px: pixels of the (padded) plane
int check_history(ws_ctx *c, size_t h, size_t w, size_t stride, const ws_options *opt, const uint8_t *levels, size_t n_levels, size_t *n_px) {
  size_t ph, pw;
  if (int rc = check_plane(c, h, w, stride, opt, &ph, &pw)) return rc;
  if (n_levels > (size_t)HISTORY_MAX_LEVELS) return fail(c, WS_ERR_BAD_ARG, "more than 256 levels");
  if (n_levels && !levels) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  for (size_t k = 0; k < n_levels; ++k)
    if (levels[k] > opt->max_water_level) return fail(c, WS_ERR_BAD_ARG, "a level above max_water_level");
  *n_px = ph * pw;
  return WS_OK;
}

// levels[k0 .. k1) in ascending order (stable: repeats keep their order), each with its plane k - k0
HistoryTable history_table(const uint8_t *levels, size_t k0, size_t k1) {
  HistoryTable t{};
  t.n = (uint32_t)(k1 - k0);
  for (size_t k = k0; k < k1; ++k) t.e[k - k0] = (uint32_t)levels[k] | (uint32_t)(k - k0) << 8;
  std::stable_sort(t.e, t.e + t.n, [](uint32_t a, uint32_t b) { return (a & 0xFFu) < (b & 0xFFu); });
  return t;
}

// the planes of tab's levels from the transform merge_host(history) has just run on this context
int render_levels(ws_ctx *c, bool merging, const HistoryTable &tab, uint32_t *d_out, size_t plane_stride, size_t n) {
  HIP_TRY(c, render_history(c->stream, merging, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, (const uint32_t *)c->uf_death.p,
                            (const uint32_t *)c->uf_hook.p, tab, d_out, plane_stride, n));
  return WS_OK;
}

// ---- merge_tree: the hierarchy of the merging transform -----------------------------------------------------

static_assert(sizeof(ws_tree_node) == sizeof(TreeRec) && WS_TREE_ALIVE == TREE_ALIVE, "ws_tree_node is the kernels' TreeRec");

// what both forms check before anything runs
int check_tree(ws_ctx *c, size_t h, size_t w, size_t stride, const ws_options *opt, size_t n_seeds, size_t *ph, size_t *pw) {
  if (int rc = check_plane(c, h, w, stride, opt, ph, pw)) return rc;
  if (n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  return WS_OK;
}

// every buffer the tree needs, BEFORE the transform: a buffer that moves bumps the context's generation, and the level loop's
// captured graphs are keyed by it
int ensure_tree(ws_ctx *c, size_t n_seeds, bool host_records) {
  int rc;
  if ((rc = ensure(c, c->tree_order, (n_seeds + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->tree_ws, TREE_WS_WORDS * sizeof(u64c)))) return rc;
  if (host_records && (rc = ensure(c, c->tree_out, (n_seeds + 1) * sizeof(ws_tree_node)))) return rc;
  return WS_OK;
}

// the records from the transform merge_host(merging, history) has just run on this context over the planes keys and seg (the
// context's own, or the arrival form's); d_seeds: the seed pairs in those planes' coordinates
int build_tree(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph, size_t pw,
               ws_tree_node *d_tree) {
  const uint32_t levels = (uint32_t)opt->max_water_level + 1;
  const uint32_t *death = (const uint32_t *)c->uf_death.p, *hook = (const uint32_t *)c->uf_hook.p;
  u64c *ws = (u64c *)c->tree_ws.p;
  TreeRec *tree = reinterpret_cast<TreeRec *>(d_tree);
  Span sp(c, KC_OTHER);
  HIP_TRY(c, hipMemsetAsync(ws, 0, TREE_WS_WORDS * sizeof(u64c), c->stream));
  // (MF_OFF_PX + levels: the pixels that arrived at levels 0 .. max_water_level)
  HIP_TRY(c, tree_init(c->stream, death, hook, d_seeds, seg, (int)ph, (int)pw, (const u64c *)c->mflags.p + MF_OFF_PX + levels, tree, n_seeds + 1, ws));
  HIP_TRY(c, tree_own_counts(c->stream, keys, seg, death, hook, tree, ph * pw));
  HIP_TRY(c, tree_fold(c->stream, tree, n_seeds + 1, levels, ws, (uint32_t *)c->tree_order.p));
  return WS_OK;
}

// ---- merge_tree_stats: the lakes of the hierarchy measured ---------------------------------------------------

static_assert(sizeof(ws_lake_stats) == 72 && sizeof(ws_lake_stats) == sizeof(LakeRec), "ws_lake_stats is the kernels' LakeRec");

// what both forms check, after check_tree and before anything runs: the weights' type and stride, and that no sum can pass 64 bits
int check_lake_weights(ws_ctx *c, size_t w, size_t ph, size_t pw, const void *weight, int dtype, size_t weight_stride) {
  uint64_t wmax = 0xFFull;
  if (weight) {
    if (dtype != WS_U8 && dtype != WS_U16) return fail(c, WS_ERR_UNSUPPORTED, "weights are u8 or u16");
    if (weight_stride < w) return fail(c, WS_ERR_BAD_ARG, "weight_row_stride < w");
    if (dtype == WS_U16) wmax = 0xFFFFull;
  }
  const uint64_t pixels = (uint64_t)ph * pw, longest = std::max(ph, pw);
  if (longest && pixels > UINT64_MAX / wmax / longest) return fail(c, WS_ERR_TOO_LARGE, "the weighted moments do not fit in 64 bits");
  return WS_OK;
}

int ensure_lake(ws_ctx *c, size_t n_seeds, bool host_records) {
  int rc;
  if ((rc = ensure(c, c->lake_acc, (n_seeds + 1) * LAKE_ACC_BYTES))) return rc;
  if (host_records && (rc = ensure(c, c->lake_out, (n_seeds + 1) * sizeof(ws_lake_stats)))) return rc;
  return WS_OK;
}

// the statistics of the tree build_tree has just finished at d_tree, from the same transform and planes
int build_lake_stats(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph,
                     size_t pw, const ws_tree_node *d_tree, const LakeWeights &wt, ws_lake_stats *d_stats) {
  Span sp(c, KC_OTHER);
  HIP_TRY(c, lake_stats(c->stream, keys, seg, (const uint32_t *)c->uf_death.p,
                        (const uint32_t *)c->uf_hook.p, reinterpret_cast<const TreeRec *>(d_tree), d_seeds, n_seeds + 1,
                        (uint32_t)opt->max_water_level + 1, (const u64c *)c->tree_ws.p, (const uint32_t *)c->tree_order.p, wt, (int)ph, (int)pw,
                        c->lake_acc.p, reinterpret_cast<LakeRec *>(d_stats)));
  return WS_OK;
}

// ---- the tree entry points' bodies: ws_merge_tree(_device), and with ls, ws_merge_tree_stats(_device) ---------------------------------

// the statistics request of ws_merge_tree_stats(_device): the weights (null: the image itself) and where the records go --
// device pointers in the device form, host pointers in the host form
struct LakeStatsWanted {
  const void *weight = nullptr;
  int dtype = 0;
  size_t stride = 0;
  ws_lake_stats *stats = nullptr;
};

// All argument checks come before device work, and every buffer is ensured BEFORE the transform (ensure_tree).
int merge_tree_device_body(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc, size_t n_seeds,
                           const ws_options *opt, ws_tree_node *d_tree, uint32_t *d_labels, const LakeStatsWanted *ls) {
  size_t ph = 0, pw = 0;
  if (int rc = check_tree(c, h, w, stride, opt, n_seeds, &ph, &pw)) return rc;
  if (ls)
    if (int rc = check_lake_weights(c, w, ph, pw, ls->weight, ls->dtype, ls->stride)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure_tree(c, n_seeds, false)) return rc;
  if (ls)
    if (int rc = ensure_lake(c, n_seeds, false)) return rc;
  if (int rc = merge_host(c, history_job_device(true, d_img, h, w, stride, d_seeds_rc, n_seeds, opt))) return rc;
  // the seed pairs as the flood took them: the caller's, or (shifted_seeds) moved into the padded plane in the context's buffer
  const uint32_t *seeds = seed_shift_of(opt) && n_seeds ? (const uint32_t *)c->seeds.p : d_seeds_rc;
  if (int rc = build_tree(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree)) return rc;
  if (ls) {
    const uint32_t off = opt->edge_correction ? 1u : 0u;
    const LakeWeights wt = ls->weight ? LakeWeights{ls->weight, ls->stride, (uint32_t)h, (uint32_t)w, off, ls->dtype == WS_U16}
                                      : LakeWeights{d_img, stride, (uint32_t)h, (uint32_t)w, off, 0};
    if (int rc = build_lake_stats(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree, wt, ls->stats)) return rc;
  }
  if (d_labels && ph * pw) HIP_TRY(c, hipMemcpyAsync(d_labels, c->labels.p, ph * pw * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int merge_tree_host_body(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                         const ws_options *opt, ws_tree_node *tree, uint64_t *labels, const LakeStatsWanted *ls) {
  size_t ph = 0, pw = 0;
  if (int rc = check_tree(c, h, w, stride, opt, n_seeds, &ph, &pw)) return rc;
  if (ls)
    if (int rc = check_lake_weights(c, w, ph, pw, ls->weight, ls->dtype, ls->stride)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure_tree(c, n_seeds, true)) return rc;
  if (ls)
    if (int rc = ensure_lake(c, n_seeds, true)) return rc;
  const size_t elem = ls && ls->weight && ls->dtype == WS_U16 ? 2 : 1;
  const bool own_plane = ls && ls->weight && h * w;
  if (own_plane) {      // contiguous on the context, before the transform: nothing moves under the level loop's graphs
    if (int rc = ensure(c, c->lake_weight, h * w * elem)) return rc;
    HIP_TRY(c, hipMemcpy2DAsync(c->lake_weight.p, w * elem, ls->weight, ls->stride * elem, w * elem, h, hipMemcpyHostToDevice, c->stream));
  }
  if (int rc = merge_host(c, history_job_host(true, img, h, w, stride, seeds_rc, n_seeds, opt))) return rc;
  const uint32_t *seeds = (const uint32_t *)c->seeds.p;      // stage_inputs: narrowed, shifted where the options say so
  ws_tree_node *d_tree = (ws_tree_node *)c->tree_out.p;
  if (int rc = build_tree(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree)) return rc;
  if (ls) {
    // (no weights: the image as stage_inputs left it on the device, w bytes a row)
    const LakeWeights wt{own_plane ? c->lake_weight.p : c->img.p, w, (uint32_t)h, (uint32_t)w, opt->edge_correction ? 1u : 0u, elem == 2};
    if (int rc = build_lake_stats(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree, wt, (ws_lake_stats *)c->lake_out.p))
      return rc;
  }
  HIP_TRY(c, hipMemcpyAsync(tree, d_tree, (n_seeds + 1) * sizeof(ws_tree_node), hipMemcpyDeviceToHost, c->stream));
  if (ls) HIP_TRY(c, hipMemcpyAsync(ls->stats, c->lake_out.p, (n_seeds + 1) * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  if (labels && ph * pw)
    if (int rc = labels_to_host_u64(c, (const uint32_t *)c->labels.p, labels, ph * pw)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

// every buffer the arrival form needs that is sized by the colours alone: the tree's and the catalogue's workspace, the recovered
// seed pairs and the union-find of the stamped level loop (the tiled forms call this on rank 0 before their gathers)
int reserve_tree_arrival(ws_ctx *c, size_t n_seeds, bool stats) {
  int rc;
  if ((rc = ensure_tree(c, n_seeds, false))) return rc;
  if (stats && (rc = ensure_lake(c, n_seeds, false))) return rc;
  if ((rc = ensure(c, c->tree_seed_px, std::max<size_t>(n_seeds, 1) * 2 * sizeof(uint32_t)))) return rc;
  if ((rc = ensure_uf(c, n_seeds + 1))) return rc;
  return ensure(c, c->uf_hook, (n_seeds + 1) * sizeof(uint32_t));
}

// ws_merge_tree_from_arrival_device: the planes of a finished segmenting transform instead of an image and a seed list.  The stamped
// level loop reads nothing else (merge_host, arrival form), and the seed pixels tree_init and lake_stats want are in the planes:
// stamp 0 marks them (seed_pixels_from_planes).  The plane is taken as it stands -- a padded plane comes in padded -- so the
// weights have no offset.  No pixel (or no seed): the plane's record 0 alone.
int merge_tree_arrival_body(ws_ctx *c, const uint32_t *d_keys, const uint32_t *d_seg, size_t h, size_t w, size_t n_seeds, const ws_options *opt,
                            ws_tree_node *d_tree, const LakeStatsWanted *ls) {
  ws_options plain = *opt;
  plain.edge_correction = 0;
  size_t ph = 0, pw = 0;
  if (int rc = check_tree(c, h, w, w, &plain, n_seeds, &ph, &pw)) return rc;
  if (pick_engine(opt) == WS_ENGINE_SWEEP) return fail(c, WS_ERR_UNSUPPORTED, "the sweep engine keeps no arrival stamps");
  if (ls) {
    if (!ls->weight) return fail(c, WS_ERR_BAD_ARG, "this form has no image: d_weight is null");
    if (int rc = check_lake_weights(c, w, ph, pw, ls->weight, ls->dtype, ls->stride)) return rc;
  }
  HIP_TRY(c, hipSetDevice(c->device));
  if (ph * pw == 0) {      // no pixel: nothing is uncoloured, no colour exists -- record 0 is the fold's identity
    const ws_tree_node none{0u, WS_TREE_ALIVE, 0u, 0u};
    const ws_lake_stats nothing{0, 0, 0, 0, 0, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 0u};
    HIP_TRY(c, hipMemcpyAsync(d_tree, &none, sizeof none, hipMemcpyHostToDevice, c->stream));
    if (ls) HIP_TRY(c, hipMemcpyAsync(ls->stats, &nothing, sizeof nothing, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WS_OK;
  }
  if (int rc = reserve_tree_arrival(c, n_seeds, ls != nullptr)) return rc;
  if (int rc = merge_host(c, history_job_arrival(d_keys, d_seg, h, w, n_seeds, &plain))) return rc;
  const uint32_t *seeds = (const uint32_t *)c->tree_seed_px.p;
  {
    Span sp(c, KC_OTHER);
    HIP_TRY(c, seed_pixels_from_planes(c->stream, d_keys, d_seg, (int)ph, (int)pw, n_seeds + 1, (uint32_t *)c->tree_seed_px.p));
  }
  if (int rc = build_tree(c, d_keys, d_seg, seeds, n_seeds, &plain, ph, pw, d_tree)) return rc;
  if (ls) {
    const LakeWeights wt{ls->weight, ls->stride, (uint32_t)h, (uint32_t)w, 0u, ls->dtype == WS_U16};
    if (int rc = build_lake_stats(c, d_keys, d_seg, seeds, n_seeds, &plain, ph, pw, d_tree, wt, ls->stats)) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

// ---- transform_history of a cube of slices (ws_transform_history_batch(_device)) ---------------------------------------------------

// The transform of slices [k_first, k_first + g) of a batch, left on the context for rendering: a stack (labels restart at 1 in every
// slice; colour c of slice k_first + k is c + base[k] in the merge forest) or one slice of the loop (g == 1, base null)
struct HistoryGroup {
  size_t k_first, g;
  const uint32_t *keys, *labels, *base;
};

// slices [ka, kb) of the group (plane pixels each), tab's levels, into out: slice ka + r's plane of slot j at out + (r * per_slice + j) * plane_stride
int render_group(ws_ctx *c, bool merging, const HistoryGroup &grp, size_t plane, size_t ka, size_t kb, const HistoryTable &tab, uint32_t *out,
                 size_t per_slice, size_t plane_stride) {
  if (!grp.base) return render_levels(c, merging, tab, out, plane_stride, plane);
  const HistoryStack st{grp.base + ka, (uint32_t)plane, (uint32_t)per_slice};
  HIP_TRY(c, render_history_stack(c->stream, merging, grp.keys + ka * plane, grp.labels + ka * plane, (const uint32_t *)c->uf_death.p,
                                  (const uint32_t *)c->uf_hook.p, tab, out, plane_stride, (kb - ka) * plane, st));
  return WS_OK;
}

// The transforms of a batch for transform_history, each handed to emit(HistoryGroup) while its planes can be rendered.  Slices
// that stack run per group of slices as one flood (flood_stack) and, merging, ONE run of the stamping per-level driver over the
// stack's numbering of colours (merge_host, arrival form, history: no pair crosses a slice border, so no lake either); anything
// else -- and a stack that fails or mispredicts, which the loop repeats and whose failing slice it names -- as the single-field
// transform of ws_transform_history_device slice by slice.  Statistics are summed.
template <class F>
int history_batch_run(ws_ctx *c, bool merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t stride, size_t slice_stride,
                      const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, size_t *failed_slice, F emit) {
  size_t ph, pw, per_group = 0;
  int rc = check_plane(c, h, w, stride, opt, &ph, &pw);
  if (rc) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t plane = ph * pw;
  ws_stats acc{};
  if (n_slices > 1 && slice_stride == h * stride && d_cube && d_seeds_rc && stackable(c, n_slices, h, w, stride, ph, pw, seed_offsets, opt, &per_group)) {
    bool stacked = true;
    std::vector<uint32_t> first;
    StackBatch batch;
    batch.d_cube = d_cube; batch.h = h; batch.stride = stride; batch.ph = ph; batch.pw = pw; batch.d_seeds_rc = d_seeds_rc; batch.seed_offsets = seed_offsets; batch.opt = opt;
    for (size_t k0 = 0; k0 < n_slices && stacked; k0 += per_group) {
      const size_t g = std::min(per_group, n_slices - k0);
      const size_t ns = seed_offsets[k0 + g] - seed_offsets[k0];
      if ((rc = ensure(c, c->stack_labels, g * plane * sizeof(uint32_t)))) return rc;
      uint32_t *labels = (uint32_t *)c->stack_labels.p;
      if (!flood_group(c, batch, k0, g, labels, first)) {
        stacked = false;
        break;
      }
      if ((rc = stats_end(c))) return rc;
      stats_add(acc, c->stats);
      const uint32_t *d_base = stacked_first(c, ns);
      if (merging) {
        LevelJob job = stack_job(c, true, g, ph, pw, ns, opt, labels, d_base);
        job.history = true;
        if ((rc = merge_host(c, job))) return rc;
        stats_add(acc, c->stats);
      }
      if ((rc = emit(HistoryGroup{k0, g, (const uint32_t *)c->keys.p, labels, d_base}))) return rc;
    }
    if (stacked) {
      c->stats = acc;
      return WS_OK;
    }
    acc = ws_stats{};
  }
  for (size_t k = 0; k < n_slices; ++k) {
    const size_t ns = seed_offsets[k + 1] - seed_offsets[k];
    rc = merge_host(c, history_job_device(merging, d_cube + k * slice_stride, h, w, stride, ns ? d_seeds_rc + 2 * seed_offsets[k] : nullptr, ns, opt));
    if (rc == WS_OK) {
      stats_add(acc, c->stats);
      rc = emit(HistoryGroup{k, 1, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, nullptr});
    }
    if (rc != WS_OK) { if (failed_slice) *failed_slice = k; return rc; }
  }
  c->stats = acc;
  c->have_keys = false;      // as after a stacked batch: the stamps are no single slice's business
  return WS_OK;
}

// what both batch forms check before anything runs: the batch as ws_transform_to_list_batch(_device), the levels as
// ws_transform_history(_device); *n_px: pixels of a (padded) slice
int check_history_batch(ws_ctx *c, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride, const size_t *seed_offsets,
                        const ws_options *opt, const uint8_t *levels, size_t n_levels, size_t *n_px) {
  if (int rc = check_batch(c, n_slices, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  return check_history(c, h, w, row_stride, opt, levels, n_levels, n_px);
}

// The host form's inputs on the device, as the device forms take them: the cube as contiguous slices (c->batch_cube) and the
// seeds as u32 pairs (c->batch_seeds) -- seeds_rc == NULL: every slice's own find_local_minima (lib.rs:1178-1197), its seeds
// behind the previous slices'.  offs (n_slices + 1): the seed offsets into c->batch_seeds; n_seeds (nullable): the counts.
int upload_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                 const uint64_t *seeds_rc, const size_t *seed_offsets, std::vector<size_t> &offs, size_t *n_seeds, size_t *failed_slice) {
  int rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t hw = h * w;
  if ((rc = ensure(c, c->batch_cube, std::max<size_t>(n_slices * hw, 1)))) return rc;
  uint8_t *d_cube = (uint8_t *)c->batch_cube.p;
  if (hw && row_stride == w && (n_slices == 1 || slice_stride == hw)) {      // a contiguous cube: one copy
    HIP_TRY(c, hipMemcpyAsync(d_cube, cube, n_slices * hw, hipMemcpyHostToDevice, c->stream));
  } else if (hw) {
    for (size_t k = 0; k < n_slices; ++k)
      HIP_TRY(c, hipMemcpy2DAsync(d_cube + k * hw, w, cube + k * slice_stride, row_stride, w, h, hipMemcpyHostToDevice, c->stream));
  }
  offs.assign(n_slices + 1, 0);
  if (seeds_rc) {
    // the u64 pairs cross whole and are narrowed on the device, as stage_inputs does (k_narrow_seeds: the host loop it replaced
    // took 5 ms for 7.3 M seeds); a coordinate past u32 is out of bounds either way: its pair becomes ~0 and stays so
    const size_t s0 = seed_offsets[0], total = seed_offsets[n_slices] - s0;
    if ((rc = ensure(c, c->batch_seeds, std::max<size_t>(total, 1) * 2 * sizeof(uint32_t)))) return rc;
    if (total) {
      if ((rc = ensure(c, c->seeds64, total * 2 * sizeof(uint64_t)))) return rc;
      HIP_TRY(c, hipMemcpyAsync(c->seeds64.p, seeds_rc + 2 * s0, total * 2 * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(c, narrow_seeds(c->stream, (const uint64_t *)c->seeds64.p, total, 0xFFFFFFFFull, 0xFFFFFFFFull, (uint32_t *)c->batch_seeds.p));
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    for (size_t k = 0; k <= n_slices; ++k) offs[k] = seed_offsets[k] - s0;
  } else {
    const size_t bound = h >= 3 && w >= 3 ? ((h - 1) / 2 + 1) * ((w - 1) / 2 + 1) : 0;
    if ((rc = ensure(c, c->batch_seeds, std::max<size_t>(n_slices * bound, 1) * 2 * sizeof(uint32_t)))) return rc;
    for (size_t k = 0; k < n_slices; ++k) {
      size_t found = 0;
      if (bound && (rc = ws_find_local_minima_device(c, d_cube + k * hw, h, w, w, (uint32_t *)c->batch_seeds.p + 2 * offs[k], bound, &found))) {
        if (failed_slice) *failed_slice = k;
        return rc;
      }
      offs[k + 1] = offs[k] + found;
    }
  }
  if (n_seeds)
    for (size_t k = 0; k < n_slices; ++k) n_seeds[k] = offs[k + 1] - offs[k];
  return WS_OK;
}

// ---- merge_tree of a cube of slices (ws_merge_tree_batch(_device)) ----------------------------------------

// the records of a stacked group from the transform history_batch_run has just run on this context, into the caller's layout at d_tree
int build_tree_stack(ws_ctx *c, const HistoryGroup &grp, size_t ns, const ws_options *opt, size_t ph, size_t pw, ws_tree_node *d_tree) {
  const uint32_t levels = (uint32_t)opt->max_water_level + 1;
  const size_t plane = ph * pw;
  const uint32_t *death = (const uint32_t *)c->uf_death.p, *hook = (const uint32_t *)c->uf_hook.p;
  u64c *ws = (u64c *)c->tree_ws.p, *hist = ws + TREE_WS_WORDS;      // (behind the fold's counters: arrivals per (slice, level))
  TreeRec *forest = (TreeRec *)c->tree_forest.p;
  const TreeStack st{grp.base, (uint32_t)grp.g, (uint32_t)plane};
  Span sp(c, KC_OTHER);
  HIP_TRY(c, hipMemsetAsync(ws, 0, (TREE_WS_WORDS + grp.g * NLEVELS) * sizeof(u64c), c->stream));
  HIP_TRY(c, slice_arrivals(c->stream, grp.keys, plane, grp.g, hist));
  HIP_TRY(c, tree_init_stack(c->stream, death, hook, (const uint32_t *)c->seed_stack.p, grp.labels, (int)(grp.g * ph), (int)pw, forest, ns + 1, ws, st));
  HIP_TRY(c, tree_own_counts_stack(c->stream, grp.keys, grp.labels, death, hook, forest, grp.g * plane, st));
  HIP_TRY(c, tree_fold(c->stream, forest, ns + 1, levels, ws, (uint32_t *)c->tree_order.p));      // ONE launch per level for the group
  HIP_TRY(c, tree_unstack(c->stream, forest, ns, grp.base, grp.g, hist, levels, plane, reinterpret_cast<TreeRec *>(d_tree)));
  return WS_OK;
}

// ---- merge_tree_stats of a cube of slices (ws_merge_tree_stats_batch(_device)) ------------------------------

// the statistics request of a batch: the weight cube on the device (null: the image cube itself, u8) with its strides in
// elements, and where the records go (device; the layout of d_tree)
struct LakeBatchWanted {
  const void *weight = nullptr;
  int dtype = 0;
  size_t stride = 0, slice_stride = 0;
  ws_lake_stats *d_stats = nullptr;
};

// what both forms check after check_batch and check_plane, before anything runs: the weights as check_lake_weights for one slice's
// plane (the 64-bit bound is a slice's: rows and columns restart in every slice), their slice stride as check_batch treats the cube's
int check_lake_batch(ws_ctx *c, size_t n_slices, size_t h, size_t w, size_t ph, size_t pw, const void *weight, int dtype, size_t weight_stride,
                     size_t weight_slice_stride) {
  if (int rc = check_lake_weights(c, w, ph, pw, weight, dtype, weight_stride)) return rc;
  if (weight && n_slices > 1 && weight_slice_stride < h * weight_stride) return fail(c, WS_ERR_BAD_ARG, "weight_slice_stride < h * weight_row_stride");
  return WS_OK;
}

// the weights of slices k .. of the batch: the request's cube, or the image cube read as u8 with its own strides
LakeWeights lake_weights_from(const LakeBatchWanted &ls, const uint8_t *d_cube, size_t stride, size_t slice_stride, size_t k, size_t h, size_t w,
                              const ws_options *opt) {
  const uint32_t off = opt->edge_correction ? 1u : 0u;
  if (!ls.weight) return LakeWeights{d_cube + k * slice_stride, stride, (uint32_t)h, (uint32_t)w, off, 0, slice_stride};
  const size_t elem = ls.dtype == WS_U16 ? 2 : 1;
  return LakeWeights{(const uint8_t *)ls.weight + k * ls.slice_stride * elem, ls.stride, (uint32_t)h, (uint32_t)w, off, ls.dtype == WS_U16, ls.slice_stride};
}

// the statistics of the forest build_tree_stack has just folded in c->tree_forest (tree_fold's buckets are still in c->tree_ws and
// c->tree_order), into the caller's layout at d_stats
int build_lake_stats_stack(ws_ctx *c, const HistoryGroup &grp, size_t ns, const ws_options *opt, size_t ph, size_t pw, const LakeWeights &wt,
                           ws_lake_stats *d_stats) {
  const TreeStack st{grp.base, (uint32_t)grp.g, (uint32_t)(ph * pw)};
  Span sp(c, KC_OTHER);
  HIP_TRY(c, lake_stats_stack(c->stream, grp.keys, grp.labels, (const uint32_t *)c->uf_death.p, (const uint32_t *)c->uf_hook.p,
                              (const TreeRec *)c->tree_forest.p, (const uint32_t *)c->seed_stack.p, ns + 1, (uint32_t)opt->max_water_level + 1,
                              (const u64c *)c->tree_ws.p, (const uint32_t *)c->tree_order.p, wt, st, (int)pw, c->lake_acc.p,
                              reinterpret_cast<LakeRec *>(d_stats)));
  return WS_OK;
}

// The trees of a batch into d_tree (device; slice k's n_k + 1 records from (seed_offsets[k] - seed_offsets[0]) + k on), every group's
// segmenting labels handed to labels(HistoryGroup) while they are on the context; with ls, every group's statistics into
// ls->d_stats in the same layout -- a stacked group's from the forest (lake_stats_stack: one fold launch per level for the group),
// a looped slice's as ws_merge_tree_stats_device's with that slice's weight plane.  Every buffer the tree and statistics kernels
// need is sized for the largest group BEFORE the first transform (as ensure_tree: nothing moves under the level loop's captured graphs).
template <class F>
int tree_batch_run(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t stride, size_t slice_stride,
                   const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, size_t ph, size_t pw, ws_tree_node *d_tree,
                   size_t *failed_slice, F labels, const LakeBatchWanted *ls = nullptr) {
  HIP_TRY(c, hipSetDevice(c->device));
  size_t per_group = 0, most = 0, most_group = 0;
  for (size_t k = 0; k < n_slices; ++k) most = std::max(most, seed_offsets[k + 1] - seed_offsets[k]);
  const bool stack = n_slices > 1 && slice_stride == h * stride && d_cube && d_seeds_rc &&
                     stackable(c, n_slices, h, w, stride, ph, pw, seed_offsets, opt, &per_group);
  if (!stack) per_group = 0;
  if (stack) {
    per_group = std::min(per_group, n_slices);
    for (size_t k0 = 0; k0 < n_slices; k0 += per_group) most_group = std::max(most_group, seed_offsets[std::min(k0 + per_group, n_slices)] - seed_offsets[k0]);
  }
  int rc;
  if ((rc = ensure(c, c->tree_order, (std::max(most, most_group) + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->tree_ws, (TREE_WS_WORDS + per_group * NLEVELS) * sizeof(u64c)))) return rc;
  if (stack) {
    if ((rc = ensure(c, c->tree_forest, (most_group + 1) * sizeof(TreeRec)))) return rc;
    if ((rc = ensure(c, c->seed_stack, (most_group * 2 + per_group + 1) * sizeof(uint32_t)))) return rc;      // (flood_stack's, for its largest group)
  }
  // (the accumulator planes: a group's colours, the forest's entry 0 and one record 0 per slice of the group)
  if (ls && (rc = ensure(c, c->lake_acc, (std::max(most, most_group) + 1 + per_group) * LAKE_ACC_BYTES))) return rc;
  const size_t s0 = seed_offsets[0];
  return history_batch_run(c, true, d_cube, n_slices, h, w, stride, slice_stride, d_seeds_rc, seed_offsets, opt, failed_slice,
                           [&](const HistoryGroup &grp) -> int {
                             const size_t k = grp.k_first, ns = seed_offsets[k + grp.g] - seed_offsets[k];
                             ws_tree_node *out = d_tree + (seed_offsets[k] - s0) + k;
                             ws_lake_stats *out_stats = ls ? ls->d_stats + (seed_offsets[k] - s0) + k : nullptr;
                             if (grp.base) {
                               if (int rc_t = build_tree_stack(c, grp, ns, opt, ph, pw, out)) return rc_t;
                               if (ls)
                                 if (int rc_t = build_lake_stats_stack(c, grp, ns, opt, ph, pw, lake_weights_from(*ls, d_cube, stride, slice_stride, k, h, w, opt), out_stats))
                                   return rc_t;
                             } else {
                               // the seed pairs as the flood took them: the caller's, or (shifted_seeds) moved into the padded plane
                               const uint32_t *seeds = seed_shift_of(opt) && ns ? (const uint32_t *)c->seeds.p : d_seeds_rc + 2 * seed_offsets[k];
                               if (int rc_t = build_tree(c, grp.keys, grp.labels, seeds, ns, opt, ph, pw, out)) return rc_t;
                               if (ls)
                                 if (int rc_t = build_lake_stats(c, grp.keys, grp.labels, seeds, ns, opt, ph, pw, out, lake_weights_from(*ls, d_cube, stride, slice_stride, k, h, w, opt), out_stats))
                                   return rc_t;
                             }
                             return labels(grp);
                           });
}

}  // namespace

namespace wsapi {
int merge_tree_arrival_reserve(ws_ctx *c, size_t n_seeds, bool stats) {
  HIP_TRY(c, hipSetDevice(c->device));
  return reserve_tree_arrival(c, n_seeds, stats);
}
}  // namespace wsapi

extern "C" {

int ws_transform_history_device(ws_ctx *c, int merging, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc,
                                size_t n_seeds, const ws_options *opt, const uint8_t *levels, size_t n_levels, uint32_t *d_out,
                                size_t plane_stride) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if ((!d_img && h * w) || (!d_seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  size_t n = 0;
  if (int rc = check_history(c, h, w, stride, opt, levels, n_levels, &n)) return rc;
  if (plane_stride < n) return fail(c, WS_ERR_BAD_ARG, "plane_stride is shorter than the plane");
  if (n_levels == 0) return WS_OK;
  if (!d_out && n) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int rc = merge_host(c, history_job_device(merging != 0, d_img, h, w, stride, d_seeds_rc, n_seeds, opt))) return rc;
  return render_levels(c, merging != 0, history_table(levels, 0, n_levels), d_out, plane_stride, n);
}

int ws_transform_history(ws_ctx *c, int merging, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc,
                         size_t n_seeds, const ws_options *opt, const uint8_t *levels, size_t n_levels, uint64_t *out) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if ((!img && h * w) || (!seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  size_t n = 0;
  if (int rc = check_history(c, h, w, stride, opt, levels, n_levels, &n)) return rc;
  if (n_levels == 0) return WS_OK;
  if (!out && n) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int rc = merge_host(c, history_job_host(merging != 0, img, h, w, stride, seeds_rc, n_seeds, opt))) return rc;
  if (n == 0) return WS_OK;
  // chunks of levels rendered into bounded scratch; a chunk's planes are contiguous there and in `out`, so a chunk of 2^21 words
  // and more crosses the bus in ONE labels_to_host_u64 as u32, widened by the host threads while its next pieces are in flight.
  // Smaller chunks, or no host threads (ws_ctx_set_host_threads(0)): plane by plane, widened on the device in the u64 buffer
  // the context already holds for one plane
  const size_t per = std::max<size_t>(1, std::min<size_t>(n_levels, HISTORY_SCRATCH_BYTES / (n * sizeof(uint32_t))));
  if (int rc = ensure(c, c->history_planes, per * n * sizeof(uint32_t))) return rc;
  uint32_t *planes = (uint32_t *)c->history_planes.p;
  for (size_t k0 = 0; k0 < n_levels; k0 += per) {
    const size_t k1 = std::min(k0 + per, n_levels);
    if (int rc = render_levels(c, merging != 0, history_table(levels, k0, k1), planes, n, n)) return rc;
    if (int rc = planes_to_host(c, planes, out + k0 * n, k1 - k0, n)) return rc;
  }
  return WS_OK;
}

int ws_merge_tree_device(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc, size_t n_seeds,
                         const ws_options *opt, ws_tree_node *d_tree, uint32_t *d_labels) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !d_tree || (!d_img && h * w) || (!d_seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  return merge_tree_device_body(c, d_img, h, w, stride, d_seeds_rc, n_seeds, opt, d_tree, d_labels, nullptr);
}

int ws_merge_tree(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                  const ws_options *opt, ws_tree_node *tree, uint64_t *labels) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !tree || (!img && h * w) || (!seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  return merge_tree_host_body(c, img, h, w, stride, seeds_rc, n_seeds, opt, tree, labels, nullptr);
}

int ws_merge_tree_stats_device(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc, size_t n_seeds,
                               const ws_options *opt, const void *d_weight, int weight_dtype, size_t weight_stride, ws_tree_node *d_tree,
                               ws_lake_stats *d_stats, uint32_t *d_labels) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !d_tree || !d_stats || (!d_img && h * w) || (!d_seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  LakeStatsWanted ls;
  ls.weight = d_weight; ls.dtype = weight_dtype; ls.stride = weight_stride; ls.stats = d_stats;
  return merge_tree_device_body(c, d_img, h, w, stride, d_seeds_rc, n_seeds, opt, d_tree, d_labels, &ls);
}

int ws_merge_tree_stats(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                        const ws_options *opt, const void *weight, int weight_dtype, size_t weight_stride, ws_tree_node *tree,
                        ws_lake_stats *stats, uint64_t *labels) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !tree || !stats || (!img && h * w) || (!seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  LakeStatsWanted ls;
  ls.weight = weight; ls.dtype = weight_dtype; ls.stride = weight_stride; ls.stats = stats;
  return merge_tree_host_body(c, img, h, w, stride, seeds_rc, n_seeds, opt, tree, labels, &ls);
}

int ws_merge_tree_from_arrival_device(ws_ctx *c, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w, size_t n_seeds,
                                      const ws_options *opt, const void *d_weight, int weight_dtype, size_t weight_row_stride,
                                      ws_tree_node *d_tree, ws_lake_stats *d_stats) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !d_tree || ((!d_keys || !d_seg_labels) && h * w)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (!d_stats) return merge_tree_arrival_body(c, d_keys, d_seg_labels, h, w, n_seeds, opt, d_tree, nullptr);
  LakeStatsWanted ls;
  ls.weight = d_weight; ls.dtype = weight_dtype; ls.stride = weight_row_stride; ls.stats = d_stats;
  return merge_tree_arrival_body(c, d_keys, d_seg_labels, h, w, n_seeds, opt, d_tree, &ls);
}

// half: 0 the whole call; 1 ws_merge_device_begin (returns WS_INTERNAL_PENDING when the graph and the speculative unions
// have been queued and the host half is still to come); 2 ws_merge_device_end (that host half)
static int merge_device_body(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc,
                             size_t n_seeds, const ws_options *opt, uint32_t *d_labels, int half) {
  size_t ph, pw;
  int rc = check_plane(c, h, w, stride, opt, &ph, &pw);
  if (rc) return rc;
  if ((!d_img && h * w) || (!d_seeds_rc && n_seeds) || (!d_labels && ph * pw)) return fail(c, WS_ERR_BAD_ARG, "null device pointer");
  if (n_seeds >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t n = ph * pw;
  if ((rc = ensure(c, c->labels, (n ? n : 1) * sizeof(uint32_t)))) return rc;
  stats_begin(c);
  const uint8_t *src = d_img;
  size_t src_stride = stride;
  const bool padded = opt->edge_correction != 0;
  if (padded && h * w == 0 && (rc = empty_image_block(c, &src, &src_stride, h, w))) return rc;
  const uint32_t *seeds;
  if ((rc = shifted_seeds(c, d_seeds_rc, n_seeds, opt, &seeds))) return rc;
  uint32_t *seg = (uint32_t *)c->labels.p;
  if ((rc = ensure(c, c->counts, std::max<size_t>(union_image_tiles((int)ph, (int)pw), 1) * sizeof(uint32_t)))) return rc;
  c->tile_min_out = (uint32_t *)c->counts.p;      // the resolve kernel classifies the tiles while it has them in registers
  c->tile_min_filled = false;
  if ((rc = ensure_uf(c, n_seeds + 1))) return rc;
  auto unions_and_relabel = [&](bool preclassified) -> int {
    HIP_TRY(c, uf_init(c->stream, (uint32_t *)c->uf_parent.p, (uint32_t *)c->uf_size.p, n_seeds + 1));
    Span sp(c, KC_OTHER);
    // at the final level a pixel is coloured exactly when its segmenting label is non-zero: no stamps needed
    HIP_TRY(c, union_image(c->stream, seg, seeds, n_seeds, (int)ph, (int)pw, (uint32_t *)c->uf_parent.p, (uint32_t *)c->counts.p,
                           preclassified, (uint32_t *)c->uf_size.p));      // (uf_init has just zeroed uf_size: the tile-root marks)
    HIP_TRY(c, relabel_final_u32(c->stream, seg, (uint32_t *)c->uf_parent.p, n_seeds + 1, d_labels, n, (uint32_t *)c->counts.p, (int)ph, (int)pw));
    return WS_OK;
  };
  // A call that replays the previous call's graph (run_fused_form: same buffers, sizes and seed count) queues its unions
  // and the relabel behind the graph BEFORE the host has looked at the graph's convergence word -- the host's wait and
  // look were ~18 us of idle GPU in the middle of every transform.  If the flood then turns out to need more passes (or
  // the seed tables were not valid), the unions ran on the previous call's labels and tile classes -- the same buffers,
  // valid colours of the same seed count -- and are simply done again after the real resolve.
  if (half != 2) {
    c->async_phase = ws_ctx::ASYNC_BEGIN;
    rc = run_fused(c, src, src_stride, (int)ph, (int)pw, opt->max_water_level, seeds, n_seeds, seg, padded);
  }
  bool speculated = false;
  if (half == 2 || (rc == WS_INTERNAL_PENDING && c->async_phase == ws_ctx::ASYNC_LAUNCHED)) {
    if (half != 2 && (rc = unions_and_relabel(true))) { c->async_phase = ws_ctx::ASYNC_NONE; c->tile_min_out = nullptr; return rc; }
    speculated = true;
    if (half == 1) return WS_INTERNAL_PENDING;      // (the context stays ASYNC_LAUNCHED, tile_min_out set: ws_merge_device_end)
    c->async_phase = ws_ctx::ASYNC_RESUME;      // the host half: waits for the graph's end event, reads its words, goes on if it must
    rc = run_fused(c, src, src_stride, (int)ph, (int)pw, opt->max_water_level, seeds, n_seeds, seg, padded);
  }
  c->async_phase = ws_ctx::ASYNC_NONE;
  c->tile_min_out = nullptr;
  if (rc) return rc == WS_INTERNAL_PENDING ? fail(c, WS_ERR_UNSUPPORTED, "internal: transform left pending") : rc;
  if (!(speculated && c->graph_sufficed) && (rc = unions_and_relabel(c->tile_min_filled))) return rc;
  c->stats.merge_levels = 1;
  return stats_end(c);
}

int ws_merge_device(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc,
                    size_t n_seeds, const ws_options *opt, uint32_t *d_labels) {
  if (!c) return WS_ERR_BAD_ARG;
  if (c->async_phase != ws_ctx::ASYNC_NONE) return fail(c, WS_ERR_BAD_ARG, "a transform begun with ws_*_device_begin has not been ended");
  return merge_device_body(c, d_img, h, w, stride, d_seeds_rc, n_seeds, opt, d_labels, 0);
}

// ws_merge_device in two halves, as ws_segment_device_begin / _end: what is left in flight is the replayed graph of the
// segmenting part AND the unions and the relabel queued behind it (see merge_device_body).
int ws_merge_device_begin(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc,
                          size_t n_seeds, const ws_options *opt, uint32_t *d_labels) {
  if (!c || !opt) return WS_ERR_BAD_ARG;
  if (c->async_phase != ws_ctx::ASYNC_NONE) return fail(c, WS_ERR_BAD_ARG, "ws_merge_device_begin: the previous transform has not been ended");
  c->async_args = {d_img, h, w, stride, d_seeds_rc, n_seeds, *opt, d_labels};
  c->async_merge = true;
  const int rc = merge_device_body(c, d_img, h, w, stride, d_seeds_rc, n_seeds, opt, d_labels, 1);
  if (rc == WS_INTERNAL_PENDING && c->async_phase == ws_ctx::ASYNC_LAUNCHED) return WS_OK;
  c->async_phase = ws_ctx::ASYNC_DONE;      // ran whole (or failed): _end hands the status over
  c->async_rc = rc == WS_INTERNAL_PENDING ? (int)WS_ERR_UNSUPPORTED : rc;
  return WS_OK;
}

int ws_merge_device_end(ws_ctx *c) {
  if (!c) return WS_ERR_BAD_ARG;
  if (!c->async_merge) return fail(c, WS_ERR_BAD_ARG, "ws_merge_device_end without ws_merge_device_begin");
  if (c->async_phase == ws_ctx::ASYNC_DONE) { c->async_phase = ws_ctx::ASYNC_NONE; c->async_merge = false; return c->async_rc; }
  if (c->async_phase != ws_ctx::ASYNC_LAUNCHED) return fail(c, WS_ERR_BAD_ARG, "ws_merge_device_end without ws_merge_device_begin");
  const auto a = c->async_args;
  const int rc = merge_device_body(c, a.d_img, a.h, a.w, a.stride, a.d_seeds, a.n_seeds, &a.opt, a.d_labels, 2);
  c->async_phase = ws_ctx::ASYNC_NONE;
  c->async_merge = false;
  return rc == WS_INTERNAL_PENDING ? (int)WS_ERR_UNSUPPORTED : rc;
}

int ws_merge_with_hook(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc,
                       size_t n_seeds, const ws_options *opt, ws_level_cb cb, void *user, uint64_t *out_labels) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  LevelJob job;
  job.merging = true; job.h = h; job.w = w; job.stride = stride; job.n_seeds = n_seeds; job.opt = opt;
  job.img = img; job.seeds_rc = seeds_rc;
  job.cb = cb; job.user = user; job.out_labels = out_labels;
  return merge_host(c, job);
}

int ws_transform_to_list_device(ws_ctx *c, int merging, const uint8_t *d_img, size_t h, size_t w, size_t stride,
                                const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt, ws_lake *d_lakes, size_t cap,
                                size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!n_lakes || !offsets || !uncoloured || (!d_lakes && cap) || (!d_img && h * w) || (!d_seeds_rc && n_seeds))
    return fail(c, WS_ERR_BAD_ARG, "null pointer");
  LevelJob job;
  job.merging = merging != 0; job.h = h; job.w = w; job.stride = stride; job.n_seeds = n_seeds; job.opt = opt;
  job.source = LevelSource::DEVICE; job.d_img = d_img; job.d_seeds_rc = d_seeds_rc;
  job.d_lakes = d_lakes; job.cap = cap; job.n_lakes = n_lakes; job.offsets = offsets; job.uncoloured = uncoloured;
  return merge_host(c, job);
}

int ws_lists_from_arrival_device(ws_ctx *c, int merging, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w,
                                 size_t n_seeds, const ws_options *opt, ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets,
                                 uint64_t *uncoloured) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !n_lakes || !offsets || !uncoloured || (!d_lakes && cap) || ((!d_keys || !d_seg_labels) && h * w))
    return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (pick_engine(opt) == WS_ENGINE_SWEEP) return fail(c, WS_ERR_UNSUPPORTED, "the sweep engine keeps no arrival stamps");
  if (int v = ws_options_validate(opt)) return fail(c, v, ws_strerror(v));
  if (h * w == 0) {      // no pixel: no lake at any level
    *n_lakes = 0;
    for (uint32_t l = 0; l <= opt->max_water_level; ++l) { offsets[l] = 0; uncoloured[l] = 0; }
    offsets[(size_t)opt->max_water_level + 1] = 0;
    return WS_OK;
  }
  LevelJob job;
  job.merging = merging != 0; job.h = h; job.w = w; job.stride = w; job.n_seeds = n_seeds; job.opt = opt;
  job.source = LevelSource::ARRIVAL; job.d_keys = d_keys; job.d_seg = d_seg_labels;
  job.d_lakes = d_lakes; job.cap = cap; job.n_lakes = n_lakes; job.offsets = offsets; job.uncoloured = uncoloured;
  return merge_host(c, job);
}

int ws_transform_to_list(ws_ctx *c, int merging, const uint8_t *img, size_t h, size_t w, size_t stride,
                         const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt, ws_lake *lakes, size_t cap,
                         size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!n_lakes || !offsets || !uncoloured || (!lakes && cap)) return fail(c, WS_ERR_BAD_ARG, "null output pointer");
  LevelJob job;
  job.merging = merging != 0; job.h = h; job.w = w; job.stride = stride; job.n_seeds = n_seeds; job.opt = opt;
  job.img = img; job.seeds_rc = seeds_rc;
  job.lakes = lakes; job.cap = cap; job.n_lakes = n_lakes; job.offsets = offsets; job.uncoloured = uncoloured;
  return merge_host(c, job);
}

int ws_transform_to_list_batch_device(ws_ctx *c, int merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w,
                                      size_t row_stride, size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets,
                                      const ws_options *opt, ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets,
                                      uint64_t *uncoloured, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  if (!n_lakes || !offsets || !uncoloured || (!d_lakes && cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int rc = check_batch(c, n_slices, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  if (n_slices && ((!d_cube && h * w) || (!d_seeds_rc && seed_offsets[n_slices] > seed_offsets[0]))) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  const size_t levels = (size_t)opt->max_water_level + 1;
  if (n_slices > 1 && slice_stride == h * row_stride && d_cube && d_seeds_rc) {
    bool done = false;
    const int rc = lists_batch_stacked(c, merging != 0, d_cube, n_slices, h, w, row_stride, d_seeds_rc, seed_offsets, opt, d_lakes, cap,
                                       n_lakes, offsets, uncoloured, &done);
    if (done || (rc != WS_OK && rc != WS_ERR_CAPACITY)) return rc;
  }
  // the loop: one ws_transform_to_list_device per slice, its records behind the previous slices'
  std::vector<uint64_t> off(levels + 1);
  ws_stats acc{};
  size_t need = 0;
  for (size_t k = 0; k < n_slices; ++k) {
    const size_t ns = seed_offsets[k + 1] - seed_offsets[k];
    const bool room = need <= cap;
    size_t got = 0;
    const int rc = ws_transform_to_list_device(c, merging, d_cube + k * slice_stride, h, w, row_stride, ns ? d_seeds_rc + 2 * seed_offsets[k] : nullptr,
                                               ns, opt, room ? d_lakes + need : nullptr, room ? cap - need : 0, &got, off.data(),
                                               uncoloured + k * levels);
    if (rc != WS_OK && rc != WS_ERR_CAPACITY) { if (failed_slice) *failed_slice = k; return rc; }
    stats_add(acc, c->stats);
    for (size_t l = 0; l < levels; ++l) offsets[k * levels + l] = need + off[l];
    need += got;
  }
  offsets[n_slices * levels] = need;
  *n_lakes = need;
  c->stats = acc;
  c->have_keys = false;      // as after a stacked batch: the stamps are no single slice's business
  if (need > cap) return fail(c, WS_ERR_CAPACITY, "lake buffer too small");
  c->err.clear();
  return WS_OK;
}

int ws_transform_to_list_batch(ws_ctx *c, int merging, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                               size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                               ws_lake *lakes, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured, size_t *n_seeds,
                               size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  if (!n_lakes || !offsets || !uncoloured || (!lakes && cap) || (!cube && h * w && n_slices)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int rc = check_batch(c, seeds_rc ? n_slices : 0, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  size_t ph, pw;
  int rc = check_plane(c, h, w, row_stride, opt, &ph, &pw);
  if (rc) return rc;
  const size_t hw = h * w, plane = ph * pw;
  // the cube as contiguous slices, the seeds as u32 pairs (the device form's inputs), then the records back as ws_transform_to_list's are
  std::vector<size_t> offs;
  if ((rc = upload_batch(c, cube, n_slices, h, w, row_stride, slice_stride, seeds_rc, seed_offsets, offs, n_seeds, failed_slice))) return rc;
  uint8_t *d_cube = (uint8_t *)c->batch_cube.p;
  if ((rc = ensure(c, c->lakes, std::max<size_t>(cap, 1) * sizeof(ws_lake)))) return rc;
  if ((rc = ensure(c, c->out64, std::max<size_t>(plane, 1) * sizeof(uint64_t)))) return rc;      // (the narrowed records' staging)
  rc = ws_transform_to_list_batch_device(c, merging, d_cube, n_slices, h, w, w, hw, (const uint32_t *)c->batch_seeds.p, offs.data(), opt,
                                         (ws_lake *)c->lakes.p, cap, n_lakes, offsets, uncoloured, failed_slice);
  if (rc) return rc;
  if ((rc = records_to_host(c, (const ws_lake *)c->lakes.p, lakes, 0, *n_lakes, std::max<size_t>(plane, 1), c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int ws_merge_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                          const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, uint32_t *d_labels,
                          size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  if (int rc = check_batch(c, n_slices, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  const size_t e = opt->edge_correction ? 2 : 0, plane = (h + e) * (w + e);
  if (n_slices > 1 && slice_stride == h * row_stride && d_cube && d_seeds_rc && d_labels) {
    bool done = false;
    const int rc = merge_batch_stacked(c, d_cube, n_slices, h, w, row_stride, d_seeds_rc, seed_offsets, opt, d_labels, &done);
    if (rc != WS_OK) return rc;
    if (done) return WS_OK;
  }
  ws_stats acc{};
  for (size_t k = 0; k < n_slices; ++k) {
    const size_t ns = seed_offsets[k + 1] - seed_offsets[k];
    const int rc = ws_merge_device(c, d_cube + k * slice_stride, h, w, row_stride, ns ? d_seeds_rc + 2 * seed_offsets[k] : nullptr, ns, opt,
                                   d_labels + k * plane);
    if (rc != WS_OK) { if (failed_slice) *failed_slice = k; return rc; }
    stats_add(acc, c->stats);
  }
  c->stats = acc;
  c->have_keys = false;
  return WS_OK;
}

int ws_transform_history_batch_device(ws_ctx *c, int merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                      size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                      const uint8_t *levels, size_t n_levels, uint32_t *d_out, size_t plane_stride, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  size_t n = 0;
  if (int rc = check_history_batch(c, n_slices, h, w, row_stride, slice_stride, seed_offsets, opt, levels, n_levels, &n)) return rc;
  if (plane_stride < n) return fail(c, WS_ERR_BAD_ARG, "plane_stride is shorter than the plane");
  if (n_levels == 0 || n_slices == 0) return WS_OK;
  if ((!d_cube && h * w) || (!d_seeds_rc && seed_offsets[n_slices] > seed_offsets[0]) || (!d_out && n)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  // every slice's planes at once, straight into the caller's buffer
  const HistoryTable tab = history_table(levels, 0, n_levels);
  return history_batch_run(c, merging != 0, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, failed_slice,
                           [&](const HistoryGroup &grp) {
                             return render_group(c, merging != 0, grp, n, 0, grp.g, tab, d_out + grp.k_first * n_levels * plane_stride, n_levels,
                                                 plane_stride);
                           });
}

int ws_transform_history_batch(ws_ctx *c, int merging, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                               size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                               const uint8_t *levels, size_t n_levels, uint64_t *out, size_t *n_seeds, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  size_t n = 0;
  if (int rc = check_history_batch(c, seeds_rc ? n_slices : 0, h, w, row_stride, slice_stride, seed_offsets, opt, levels, n_levels, &n)) return rc;
  if (n_levels == 0 || n_slices == 0) return WS_OK;
  if ((!cube && h * w) || (!out && n)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  std::vector<size_t> offs;
  int rc = upload_batch(c, cube, n_slices, h, w, row_stride, slice_stride, seeds_rc, seed_offsets, offs, n_seeds, failed_slice);
  if (rc) return rc;
  if (n == 0)      // (no pixel: the transforms still run, for their errors)
    return history_batch_run(c, merging != 0, (const uint8_t *)c->batch_cube.p, n_slices, h, w, w, h * w, (const uint32_t *)c->batch_seeds.p,
                             offs.data(), opt, failed_slice, [](const HistoryGroup &) { return (int)WS_OK; });
  // The planes are rendered into bounded scratch and cross the bus chunk by chunk.  Where a slice's planes fit, a chunk is a run
  // of whole slices -- contiguous in `out` as in the scratch, so it crosses in ONE labels_to_host_u64 (u32 words widened by the
  // host threads); where they do not, a chunk is a run of one slice's levels, as in ws_transform_history.
  const size_t scratch_words = HISTORY_SCRATCH_BYTES / sizeof(uint32_t), slice_words = n_levels * n;
  const size_t slices_per = slice_words <= scratch_words ? std::min(n_slices, scratch_words / slice_words) : 0;
  const size_t levels_per = std::max<size_t>(1, std::min(n_levels, scratch_words / n));
  if ((rc = ensure(c, c->history_planes, (slices_per ? slices_per * slice_words : levels_per * n) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->out64, n * sizeof(uint64_t)))) return rc;      // (the plane-by-plane copy widens there)
  uint32_t *planes = (uint32_t *)c->history_planes.p;
  const HistoryTable all = history_table(levels, 0, n_levels);
  return history_batch_run(c, merging != 0, (const uint8_t *)c->batch_cube.p, n_slices, h, w, w, h * w, (const uint32_t *)c->batch_seeds.p,
                           offs.data(), opt, failed_slice, [&](const HistoryGroup &grp) -> int {
                             if (slices_per) {
                               for (size_t ka = 0; ka < grp.g; ka += slices_per) {
                                 const size_t kb = std::min(ka + slices_per, grp.g);
                                 if (int rc_r = render_group(c, merging != 0, grp, n, ka, kb, all, planes, n_levels, n)) return rc_r;
                                 if (int rc_c = planes_to_host(c, planes, out + (grp.k_first + ka) * slice_words, (kb - ka) * n_levels, n)) return rc_c;
                               }
                               return (int)WS_OK;
                             }
                             for (size_t k = 0; k < grp.g; ++k)
                               for (size_t j0 = 0; j0 < n_levels; j0 += levels_per) {
                                 const size_t j1 = std::min(j0 + levels_per, n_levels);
                                 if (int rc_r = render_group(c, merging != 0, grp, n, k, k + 1, history_table(levels, j0, j1), planes, 0, n)) return rc_r;
                                 if (int rc_c = planes_to_host(c, planes, out + (grp.k_first + k) * slice_words + j0 * n, j1 - j0, n)) return rc_c;
                               }
                             return (int)WS_OK;
                           });
}

int ws_merge_tree_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                               const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_tree_node *d_tree,
                               uint32_t *d_labels, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  if (int rc = check_batch(c, n_slices, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  size_t ph = 0, pw = 0;
  if (int rc = check_plane(c, h, w, row_stride, opt, &ph, &pw)) return rc;
  if (n_slices == 0) return WS_OK;
  const size_t total = seed_offsets[n_slices] - seed_offsets[0], plane = ph * pw;
  if (total >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (!d_tree || (!d_cube && h * w) || (!d_seeds_rc && total)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int rc = tree_batch_run(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, ph, pw, d_tree, failed_slice,
                              [&](const HistoryGroup &grp) -> int {
                                if (d_labels && plane)
                                  HIP_TRY(c, hipMemcpyAsync(d_labels + grp.k_first * plane, grp.labels, grp.g * plane * sizeof(uint32_t),
                                                            hipMemcpyDeviceToDevice, c->stream));
                                return (int)WS_OK;
                              }))
    return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int ws_merge_tree_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                        const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_tree_node *tree, size_t cap,
                        size_t *n_records, uint64_t *labels, size_t *n_seeds, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  if (int rc = check_batch(c, seeds_rc ? n_slices : 0, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  size_t ph = 0, pw = 0;
  int rc = check_plane(c, h, w, row_stride, opt, &ph, &pw);
  if (rc) return rc;
  if (n_slices == 0) {
    if (n_records) *n_records = 0;
    return WS_OK;
  }
  if ((!cube && h * w) || (!tree && cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (seeds_rc && seed_offsets[n_slices] - seed_offsets[0] >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  std::vector<size_t> offs;
  if ((rc = upload_batch(c, cube, n_slices, h, w, row_stride, slice_stride, seeds_rc, seed_offsets, offs, n_seeds, failed_slice))) return rc;
  const size_t total = offs[n_slices] + n_slices, plane = ph * pw;
  if (n_records) *n_records = total;
  if (offs[n_slices] >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (cap < total) return fail(c, WS_ERR_CAPACITY, "tree buffer too small");      // counted, nothing flooded: the caller learns how many records to make room for
  if ((rc = ensure(c, c->tree_out, total * sizeof(ws_tree_node)))) return rc;
  if (labels && (rc = ensure(c, c->out64, std::max<size_t>(plane, 1) * sizeof(uint64_t)))) return rc;      // (the plane-by-plane copy widens there)
  rc = tree_batch_run(c, (const uint8_t *)c->batch_cube.p, n_slices, h, w, w, h * w, (const uint32_t *)c->batch_seeds.p, offs.data(), opt, ph, pw,
                      (ws_tree_node *)c->tree_out.p, failed_slice, [&](const HistoryGroup &grp) -> int {
                        if (!labels || !plane) return (int)WS_OK;
                        return planes_to_host(c, grp.labels, labels + grp.k_first * plane, grp.g, plane);
                      });
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(tree, c->tree_out.p, total * sizeof(ws_tree_node), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int ws_merge_tree_stats_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                     size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                     const void *d_weight, int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride,
                                     ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *d_labels, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  if (int rc = check_batch(c, n_slices, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  size_t ph = 0, pw = 0;
  if (int rc = check_plane(c, h, w, row_stride, opt, &ph, &pw)) return rc;
  if (int rc = check_lake_batch(c, n_slices, h, w, ph, pw, d_weight, weight_dtype, weight_row_stride, weight_slice_stride)) return rc;
  if (n_slices == 0) return WS_OK;
  const size_t total = seed_offsets[n_slices] - seed_offsets[0], plane = ph * pw;
  if (total >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (!d_tree || !d_stats || (!d_cube && h * w) || (!d_seeds_rc && total)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  LakeBatchWanted ls;
  ls.weight = h * w ? d_weight : nullptr; ls.dtype = weight_dtype; ls.stride = weight_row_stride; ls.slice_stride = weight_slice_stride; ls.d_stats = d_stats;
  if (int rc = tree_batch_run(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, ph, pw, d_tree, failed_slice,
                              [&](const HistoryGroup &grp) -> int {
                                if (d_labels && plane)
                                  HIP_TRY(c, hipMemcpyAsync(d_labels + grp.k_first * plane, grp.labels, grp.g * plane * sizeof(uint32_t),
                                                            hipMemcpyDeviceToDevice, c->stream));
                                return (int)WS_OK;
                              }, &ls))
    return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int ws_merge_tree_stats_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                              const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, const void *weight, int weight_dtype,
                              size_t weight_row_stride, size_t weight_slice_stride, ws_tree_node *tree, ws_lake_stats *stats, size_t cap,
                              size_t *n_records, uint64_t *labels, size_t *n_seeds, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  if (int rc = check_batch(c, seeds_rc ? n_slices : 0, h, row_stride, slice_stride, seed_offsets, opt)) return rc;
  size_t ph = 0, pw = 0;
  int rc = check_plane(c, h, w, row_stride, opt, &ph, &pw);
  if (rc) return rc;
  if ((rc = check_lake_batch(c, n_slices, h, w, ph, pw, weight, weight_dtype, weight_row_stride, weight_slice_stride))) return rc;
  if (n_slices == 0) {
    if (n_records) *n_records = 0;
    return WS_OK;
  }
  if ((!cube && h * w) || ((!tree || !stats) && cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (seeds_rc && seed_offsets[n_slices] - seed_offsets[0] >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  std::vector<size_t> offs;
  if ((rc = upload_batch(c, cube, n_slices, h, w, row_stride, slice_stride, seeds_rc, seed_offsets, offs, n_seeds, failed_slice))) return rc;
  const size_t total = offs[n_slices] + n_slices, plane = ph * pw;
  if (n_records) *n_records = total;
  if (offs[n_slices] >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (cap < total) return fail(c, WS_ERR_CAPACITY, "record buffers too small");      // counted, nothing flooded
  if ((rc = ensure(c, c->tree_out, total * sizeof(ws_tree_node)))) return rc;
  if ((rc = ensure(c, c->lake_out, total * sizeof(ws_lake_stats)))) return rc;
  if (labels && (rc = ensure(c, c->out64, std::max<size_t>(plane, 1) * sizeof(uint64_t)))) return rc;      // (the plane-by-plane copy widens there)
  LakeBatchWanted ls;
  ls.d_stats = (ws_lake_stats *)c->lake_out.p;
  if (weight && h * w) {      // the weight cube contiguous on the context, before the first transform: nothing moves under the level loop's graphs
    const size_t elem = weight_dtype == WS_U16 ? 2 : 1;
    if ((rc = ensure(c, c->lake_weight, n_slices * h * w * elem))) return rc;
    for (size_t k = 0; k < n_slices; ++k)
      HIP_TRY(c, hipMemcpy2DAsync((uint8_t *)c->lake_weight.p + k * h * w * elem, w * elem, (const uint8_t *)weight + k * weight_slice_stride * elem,
                                  weight_row_stride * elem, w * elem, h, hipMemcpyHostToDevice, c->stream));
    ls.weight = c->lake_weight.p; ls.dtype = weight_dtype; ls.stride = w; ls.slice_stride = h * w;
  }
  rc = tree_batch_run(c, (const uint8_t *)c->batch_cube.p, n_slices, h, w, w, h * w, (const uint32_t *)c->batch_seeds.p, offs.data(), opt, ph, pw,
                      (ws_tree_node *)c->tree_out.p, failed_slice, [&](const HistoryGroup &grp) -> int {
                        if (!labels || !plane) return (int)WS_OK;
                        return planes_to_host(c, grp.labels, labels + grp.k_first * plane, grp.g, plane);
                      }, &ls);
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(tree, c->tree_out.p, total * sizeof(ws_tree_node), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(stats, c->lake_out.p, total * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

}  // extern "C"
