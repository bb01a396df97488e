// ws_lists.hip -- the merging drivers (lib.rs:1328-1522) and transform_to_list (lib.rs:1551-1561, 1837-1847): per-level
// unions over seed colours, lake areas and sparse lake records (kernels: ws_merge.hip the level loop, ws_merge_final.hip the
// final labels alone, ws_merge_tree.hip history planes, merge tree, lake statistics and lake shapes; wrappers: ws_merge.hpp).  The per-level
// driver merge_host with the single-field entry points; the same products for cubes of slices: ws_batch.hip, which calls what
// ws_lists.hpp declares.
#include "ws_lists.hpp"

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
}  // namespace

// Records [from, end) of the device array d_rec into the host's `lakes`, on stream `on` (returns with the copy complete when the
// chunked road is taken; otherwise queued).  A piece of two million records and more (2048^2 planes on) crosses the bus as u32 --
// a colour and an area of a plane below 2^31 pixels fit -- and is widened into the caller's records by the host's threads
// (ws_hostcopy.hip; pieces of at most n records: the narrowed words borrow the u64 label buffer, n x 8 bytes).
// A piece that is too short for the chunked road must NOT go down it: labels_to_host_u64's other path widens into the very
// buffer the narrowed words sit in (and may reallocate it).  Such pieces are copied as they are.
int wsapi::records_to_host(ws_ctx *c, const ws_lake *d_rec, ws_lake *lakes, size_t from, size_t end, size_t n, hipStream_t on) {
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

namespace {

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
}  // namespace

int wsapi::merge_host(ws_ctx *c, const LevelJob &job) {
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

void wsapi::stats_add(ws_stats &a, const ws_stats &b) {
  a.relax_passes += b.relax_passes; a.resolve_passes += b.resolve_passes; a.sweep_steps += b.sweep_steps;
  a.merge_levels = std::max(a.merge_levels, b.merge_levels);
  a.tiles_run_relax += b.tiles_run_relax; a.tiles_run_resolve += b.tiles_run_resolve;
  a.ms_relax += b.ms_relax; a.ms_resolve += b.ms_resolve; a.ms_sweep += b.ms_sweep; a.ms_other += b.ms_other; a.ms_total += b.ms_total;
  a.launches_relax += b.launches_relax; a.launches_resolve += b.launches_resolve; a.launches_sweep += b.launches_sweep;
  a.relax_tile_iterations += b.relax_tile_iterations; a.graph_launches += b.graph_launches;
}

int wsapi::ensure_uf(ws_ctx *c, size_t n_colours) {
  int rc;
  if ((rc = ensure(c, c->uf_parent, n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->uf_size, n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->uf_hooked, n_colours * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->uf_death, n_colours * sizeof(uint32_t)))) return rc;
  return WS_OK;
}

// ---- transform_history (lib.rs:1233-1237, 1538-1549, 1824-1835) for a list of levels ------------------------------------------------

// n_planes planes of n u32 words, contiguous on the device, into the host's u64 planes: in ONE labels_to_host_u64 where the host
// threads widen (host_copy_in_chunks), else plane by plane, widened on the device in the u64 buffer the context holds for one plane
int wsapi::planes_to_host(ws_ctx *c, const uint32_t *src, uint64_t *dst, size_t n_planes, size_t n) {
  if (host_copy_in_chunks(c, n_planes * n)) return labels_to_host_u64(c, src, dst, n_planes * n);
  for (size_t i = 0; i < n_planes; ++i)
    if (int rc = labels_to_host_u64(c, src + i * n, dst + i * n, n)) return rc;
  return WS_OK;
}

// what both forms check before anything runs; *n_px: pixels of the (padded) plane
int wsapi::check_history(ws_ctx *c, size_t h, size_t w, size_t stride, const ws_options *opt, const uint8_t *levels, size_t n_levels, size_t *n_px) {
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
HistoryTable wsapi::history_table(const uint8_t *levels, size_t k0, size_t k1) {
  HistoryTable t{};
  t.n = (uint32_t)(k1 - k0);
  for (size_t k = k0; k < k1; ++k) t.e[k - k0] = (uint32_t)levels[k] | (uint32_t)(k - k0) << 8;
  std::stable_sort(t.e, t.e + t.n, [](uint32_t a, uint32_t b) { return (a & 0xFFu) < (b & 0xFFu); });
  return t;
}

// the planes of tab's levels from the transform merge_host(history) has just run on this context
int wsapi::render_levels(ws_ctx *c, bool merging, const HistoryTable &tab, uint32_t *d_out, size_t plane_stride, size_t n) {
  HIP_TRY(c, render_history(c->stream, merging, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, (const uint32_t *)c->uf_death.p,
                            (const uint32_t *)c->uf_hook.p, tab, d_out, plane_stride, n));
  return WS_OK;
}

// ---- merge_tree: the hierarchy of the merging transform -----------------------------------------------------

static_assert(sizeof(ws_tree_node) == sizeof(TreeRec) && WS_TREE_ALIVE == TREE_ALIVE, "ws_tree_node is the kernels' TreeRec");

// the records from the transform merge_host(merging, history) has just run on this context over the planes keys and seg (the
// context's own, or the arrival form's); d_seeds: the seed pairs in those planes' coordinates
int wsapi::build_tree(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph, size_t pw,
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
int wsapi::check_lake_weights(ws_ctx *c, size_t w, size_t ph, size_t pw, const void *weight, int dtype, size_t weight_stride) {
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

// the statistics of the tree build_tree has just finished at d_tree, from the same transform and planes
int wsapi::build_lake_stats(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph,
                     size_t pw, const ws_tree_node *d_tree, const LakeWeights &wt, ws_lake_stats *d_stats) {
  Span sp(c, KC_OTHER);
  HIP_TRY(c, lake_stats(c->stream, keys, seg, (const uint32_t *)c->uf_death.p,
                        (const uint32_t *)c->uf_hook.p, reinterpret_cast<const TreeRec *>(d_tree), d_seeds, n_seeds + 1,
                        (uint32_t)opt->max_water_level + 1, (const u64c *)c->tree_ws.p, (const uint32_t *)c->tree_order.p, wt, (int)ph, (int)pw,
                        c->lake_acc.p, reinterpret_cast<LakeRec *>(d_stats)));
  return WS_OK;
}

// ---- merge_tree_shapes: the lakes' second moments ---------------------------------------------------------

static_assert(sizeof(ws_lake_shape) == 96 && sizeof(ws_lake_shape) == sizeof(ShapeRec) && sizeof(ws_lake_shape) == SHAPE_ACC_BYTES,
              "ws_lake_shape is the kernels' ShapeRec");

// the shapes of the tree build_tree has just finished at d_tree, after build_lake_stats, from the same transform, planes and weights
int wsapi::build_lake_shapes(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph,
                      size_t pw, const ws_tree_node *d_tree, const LakeWeights &wt, ws_lake_shape *d_shapes) {
  Span sp(c, KC_OTHER);
  HIP_TRY(c, lake_shapes(c->stream, keys, seg, (const uint32_t *)c->uf_death.p,
                         (const uint32_t *)c->uf_hook.p, reinterpret_cast<const TreeRec *>(d_tree), d_seeds, n_seeds + 1,
                         (uint32_t)opt->max_water_level + 1, (const u64c *)c->tree_ws.p, (const uint32_t *)c->tree_order.p, wt, (int)ph, (int)pw,
                         c->shape_acc.p, reinterpret_cast<ShapeRec *>(d_shapes)));
  return WS_OK;
}

namespace {

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

int ensure_lake(ws_ctx *c, size_t n_seeds, bool host_records) {
  int rc;
  if ((rc = ensure(c, c->lake_acc, (n_seeds + 1) * LAKE_ACC_BYTES))) return rc;
  if (host_records && (rc = ensure(c, c->lake_out, (n_seeds + 1) * sizeof(ws_lake_stats)))) return rc;
  return WS_OK;
}

int ensure_shape(ws_ctx *c, size_t n_seeds, bool host_records) {
  int rc;
  if ((rc = ensure(c, c->shape_acc, (n_seeds + 1) * SHAPE_ACC_BYTES))) return rc;
  if (host_records && (rc = ensure(c, c->shape_out, (n_seeds + 1) * sizeof(ws_lake_shape)))) return rc;
  return WS_OK;
}

// ---- the tree entry points' bodies: ws_merge_tree(_device); with ls, ws_merge_tree_stats(_device); with ls and sh, ws_merge_tree_shapes(_device)

// the statistics request of ws_merge_tree_stats(_device): the weights (null: the image itself) and where the records go --
// device pointers in the device form, host pointers in the host form
struct LakeStatsWanted {
  const void *weight = nullptr;
  int dtype = 0;
  size_t stride = 0;
  ws_lake_stats *stats = nullptr;
};

// the shapes request of ws_merge_tree_shapes(_device), which comes with a statistics request (its weights are the shapes'): where
// the records go -- a device pointer in the device forms, a host pointer in the host form
struct LakeShapesWanted {
  ws_lake_shape *shapes = nullptr;
};

// All argument checks come before device work, and every buffer is ensured BEFORE the transform (ensure_tree).
int merge_tree_device_body(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc, size_t n_seeds,
                           const ws_options *opt, ws_tree_node *d_tree, uint32_t *d_labels, const LakeStatsWanted *ls,
                           const LakeShapesWanted *sh = nullptr) {
  size_t ph = 0, pw = 0;
  if (int rc = check_tree(c, h, w, stride, opt, n_seeds, &ph, &pw)) return rc;
  if (ls)
    if (int rc = check_lake_weights(c, w, ph, pw, ls->weight, ls->dtype, ls->stride)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure_tree(c, n_seeds, false)) return rc;
  if (ls)
    if (int rc = ensure_lake(c, n_seeds, false)) return rc;
  if (sh)
    if (int rc = ensure_shape(c, n_seeds, false)) return rc;
  if (int rc = merge_host(c, LevelJob::from_device(true, d_img, h, w, stride, d_seeds_rc, n_seeds, opt).with_history())) return rc;
  // the seed pairs as the flood took them: the caller's, or (shifted_seeds) moved into the padded plane in the context's buffer
  const uint32_t *seeds = seed_shift_of(opt) && n_seeds ? (const uint32_t *)c->seeds.p : d_seeds_rc;
  if (int rc = build_tree(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree)) return rc;
  if (ls) {
    const uint32_t off = opt->edge_correction ? 1u : 0u;
    const LakeWeights wt = ls->weight ? LakeWeights{ls->weight, ls->stride, (uint32_t)h, (uint32_t)w, off, ls->dtype == WS_U16}
                                      : LakeWeights{d_img, stride, (uint32_t)h, (uint32_t)w, off, 0};
    if (int rc = build_lake_stats(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree, wt, ls->stats)) return rc;
    if (sh)
      if (int rc = build_lake_shapes(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree, wt, sh->shapes)) return rc;
  }
  if (d_labels && ph * pw) HIP_TRY(c, hipMemcpyAsync(d_labels, c->labels.p, ph * pw * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int merge_tree_host_body(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                         const ws_options *opt, ws_tree_node *tree, uint64_t *labels, const LakeStatsWanted *ls, const LakeShapesWanted *sh = nullptr) {
  size_t ph = 0, pw = 0;
  if (int rc = check_tree(c, h, w, stride, opt, n_seeds, &ph, &pw)) return rc;
  if (ls)
    if (int rc = check_lake_weights(c, w, ph, pw, ls->weight, ls->dtype, ls->stride)) return rc;
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = ensure_tree(c, n_seeds, true)) return rc;
  if (ls)
    if (int rc = ensure_lake(c, n_seeds, true)) return rc;
  if (sh)
    if (int rc = ensure_shape(c, n_seeds, true)) return rc;
  const size_t elem = ls && ls->weight && ls->dtype == WS_U16 ? 2 : 1;
  const bool own_plane = ls && ls->weight && h * w;
  if (own_plane) {      // contiguous on the context, before the transform: nothing moves under the level loop's graphs
    if (int rc = ensure(c, c->lake_weight, h * w * elem)) return rc;
    HIP_TRY(c, hipMemcpy2DAsync(c->lake_weight.p, w * elem, ls->weight, ls->stride * elem, w * elem, h, hipMemcpyHostToDevice, c->stream));
  }
  if (int rc = merge_host(c, LevelJob::from_host(true, img, h, w, stride, seeds_rc, n_seeds, opt).with_history())) return rc;
  const uint32_t *seeds = (const uint32_t *)c->seeds.p;      // stage_inputs: narrowed, shifted where the options say so
  ws_tree_node *d_tree = (ws_tree_node *)c->tree_out.p;
  if (int rc = build_tree(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree)) return rc;
  if (ls) {
    // (no weights: the image as stage_inputs left it on the device, w bytes a row)
    const LakeWeights wt{own_plane ? c->lake_weight.p : c->img.p, w, (uint32_t)h, (uint32_t)w, opt->edge_correction ? 1u : 0u, elem == 2};
    if (int rc = build_lake_stats(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree, wt, (ws_lake_stats *)c->lake_out.p))
      return rc;
    if (sh)
      if (int rc = build_lake_shapes(c, (const uint32_t *)c->keys.p, (const uint32_t *)c->labels.p, seeds, n_seeds, opt, ph, pw, d_tree, wt, (ws_lake_shape *)c->shape_out.p))
        return rc;
  }
  HIP_TRY(c, hipMemcpyAsync(tree, d_tree, (n_seeds + 1) * sizeof(ws_tree_node), hipMemcpyDeviceToHost, c->stream));
  if (ls) HIP_TRY(c, hipMemcpyAsync(ls->stats, c->lake_out.p, (n_seeds + 1) * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  if (sh) HIP_TRY(c, hipMemcpyAsync(sh->shapes, c->shape_out.p, (n_seeds + 1) * sizeof(ws_lake_shape), hipMemcpyDeviceToHost, c->stream));
  if (labels && ph * pw)
    if (int rc = labels_to_host_u64(c, (const uint32_t *)c->labels.p, labels, ph * pw)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

// every buffer the arrival form needs that is sized by the colours alone: the tree's and the catalogue's workspace, the recovered
// seed pairs and the union-find of the stamped level loop (the tiled forms call this on rank 0 before their gathers)
int reserve_tree_arrival(ws_ctx *c, size_t n_seeds, bool stats, bool shapes = false) {
  int rc;
  if ((rc = ensure_tree(c, n_seeds, false))) return rc;
  if (stats && (rc = ensure_lake(c, n_seeds, false))) return rc;
  if (shapes && (rc = ensure_shape(c, n_seeds, false))) return rc;
  if ((rc = ensure(c, c->tree_seed_px, std::max<size_t>(n_seeds, 1) * 2 * sizeof(uint32_t)))) return rc;
  if ((rc = ensure_uf(c, n_seeds + 1))) return rc;
  return ensure(c, c->uf_hook, (n_seeds + 1) * sizeof(uint32_t));
}

// ws_merge_tree_from_arrival_device: the planes of a finished segmenting transform instead of an image and a seed list.  The stamped
// level loop reads nothing else (merge_host, arrival form), and the seed pixels tree_init and lake_stats want are in the planes:
// stamp 0 marks them (seed_pixels_from_planes).  The plane is taken as it stands -- a padded plane comes in padded -- so the
// weights have no offset.  No pixel (or no seed): the plane's record 0 alone.
int merge_tree_arrival_body(ws_ctx *c, const uint32_t *d_keys, const uint32_t *d_seg, size_t h, size_t w, size_t n_seeds, const ws_options *opt,
                            ws_tree_node *d_tree, const LakeStatsWanted *ls, const LakeShapesWanted *sh = nullptr) {
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
    if (sh) HIP_TRY(c, hipMemsetAsync(sh->shapes, 0, sizeof(ws_lake_shape), c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return WS_OK;
  }
  if (int rc = reserve_tree_arrival(c, n_seeds, ls != nullptr, sh != nullptr)) return rc;
  if (int rc = merge_host(c, LevelJob::from_arrival(true, d_keys, d_seg, h, w, n_seeds, &plain).with_history())) return rc;
  const uint32_t *seeds = (const uint32_t *)c->tree_seed_px.p;
  {
    Span sp(c, KC_OTHER);
    HIP_TRY(c, seed_pixels_from_planes(c->stream, d_keys, d_seg, (int)ph, (int)pw, n_seeds + 1, (uint32_t *)c->tree_seed_px.p));
  }
  if (int rc = build_tree(c, d_keys, d_seg, seeds, n_seeds, &plain, ph, pw, d_tree)) return rc;
  if (ls) {
    const LakeWeights wt{ls->weight, ls->stride, (uint32_t)h, (uint32_t)w, 0u, ls->dtype == WS_U16};
    if (int rc = build_lake_stats(c, d_keys, d_seg, seeds, n_seeds, &plain, ph, pw, d_tree, wt, ls->stats)) return rc;
    if (sh)
      if (int rc = build_lake_shapes(c, d_keys, d_seg, seeds, n_seeds, &plain, ph, pw, d_tree, wt, sh->shapes)) return rc;
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
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
  if (int rc = merge_host(c, LevelJob::from_device(merging != 0, d_img, h, w, stride, d_seeds_rc, n_seeds, opt).with_history())) return rc;
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
  if (int rc = merge_host(c, LevelJob::from_host(merging != 0, img, h, w, stride, seeds_rc, n_seeds, opt).with_history())) return rc;
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

int ws_merge_tree_shapes_device(ws_ctx *c, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc, size_t n_seeds,
                                const ws_options *opt, const void *d_weight, int weight_dtype, size_t weight_stride, ws_tree_node *d_tree,
                                ws_lake_stats *d_stats, ws_lake_shape *d_shapes, uint32_t *d_labels) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !d_tree || !d_stats || !d_shapes || (!d_img && h * w) || (!d_seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (reinterpret_cast<uintptr_t>(d_shapes) & 7u) return fail(c, WS_ERR_BAD_ARG, "d_shapes is not 8-byte aligned");
  LakeStatsWanted ls;
  ls.weight = d_weight; ls.dtype = weight_dtype; ls.stride = weight_stride; ls.stats = d_stats;
  LakeShapesWanted sh;
  sh.shapes = d_shapes;
  return merge_tree_device_body(c, d_img, h, w, stride, d_seeds_rc, n_seeds, opt, d_tree, d_labels, &ls, &sh);
}

int ws_merge_tree_shapes(ws_ctx *c, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                         const ws_options *opt, const void *weight, int weight_dtype, size_t weight_stride, ws_tree_node *tree,
                         ws_lake_stats *stats, ws_lake_shape *shapes, uint64_t *labels) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !tree || !stats || !shapes || (!img && h * w) || (!seeds_rc && n_seeds)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  LakeStatsWanted ls;
  ls.weight = weight; ls.dtype = weight_dtype; ls.stride = weight_stride; ls.stats = stats;
  LakeShapesWanted sh;
  sh.shapes = shapes;
  return merge_tree_host_body(c, img, h, w, stride, seeds_rc, n_seeds, opt, tree, labels, &ls, &sh);
}

int ws_merge_tree_shapes_from_arrival_device(ws_ctx *c, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w, size_t n_seeds,
                                             const ws_options *opt, const void *d_weight, int weight_dtype, size_t weight_row_stride,
                                             ws_tree_node *d_tree, ws_lake_stats *d_stats, ws_lake_shape *d_shapes) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (!opt || !d_tree || !d_stats || !d_shapes || ((!d_keys || !d_seg_labels) && h * w)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (reinterpret_cast<uintptr_t>(d_shapes) & 7u) return fail(c, WS_ERR_BAD_ARG, "d_shapes is not 8-byte aligned");
  LakeStatsWanted ls;
  ls.weight = d_weight; ls.dtype = weight_dtype; ls.stride = weight_row_stride; ls.stats = d_stats;
  LakeShapesWanted sh;
  sh.shapes = d_shapes;
  return merge_tree_arrival_body(c, d_keys, d_seg_labels, h, w, n_seeds, opt, d_tree, &ls, &sh);
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
  LevelJob job = LevelJob::from_host(true, img, h, w, stride, seeds_rc, n_seeds, opt);
  job.cb = cb; job.user = user; job.out_labels = out_labels;
  return merge_host(c, job);
}

int ws_transform_to_list_device(ws_ctx *c, int merging, const uint8_t *d_img, size_t h, size_t w, size_t stride,
                                const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt, ws_lake *d_lakes, size_t cap,
                                size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!n_lakes || !offsets || !uncoloured || (!d_lakes && cap) || (!d_img && h * w) || (!d_seeds_rc && n_seeds))
    return fail(c, WS_ERR_BAD_ARG, "null pointer");
  return merge_host(c, LevelJob::from_device(merging != 0, d_img, h, w, stride, d_seeds_rc, n_seeds, opt).with_lists(d_lakes, cap, n_lakes, offsets, uncoloured));
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
  return merge_host(c, LevelJob::from_arrival(merging != 0, d_keys, d_seg_labels, h, w, n_seeds, opt).with_lists(d_lakes, cap, n_lakes, offsets, uncoloured));
}

int ws_transform_to_list(ws_ctx *c, int merging, const uint8_t *img, size_t h, size_t w, size_t stride,
                         const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt, ws_lake *lakes, size_t cap,
                         size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!n_lakes || !offsets || !uncoloured || (!lakes && cap)) return fail(c, WS_ERR_BAD_ARG, "null output pointer");
  return merge_host(c, LevelJob::from_host(merging != 0, img, h, w, stride, seeds_rc, n_seeds, opt).with_lists(lakes, cap, n_lakes, offsets, uncoloured));
}

}  // extern "C"
