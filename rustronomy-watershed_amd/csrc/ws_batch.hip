// ws_batch.hip -- the cube drivers: every product of the library for a batch of equal-sized independent slices on the device
// (final labels segmenting and merging, lake lists, history planes, merge trees, lake catalogues, lake shapes).  One description of
// a batch (Batch, check_batch), one decision whether its slices run as stacks (stackable), one walk over the groups of a stack with the
// slice-by-slice loop behind it (run_batch); the products plug into the walk with what they do to a flooded group and to one slice.
// The per-level driver and the single-field forms they call: ws_lists.hip (ws_lists.hpp); the flood of a stack: ws_segment.hip.
#include "ws_lists.hpp"

namespace wsapi {

// A batch as the device forms are given it, with the (padded) plane of one slice as check_plane derives it
struct Batch {
  const uint8_t *d_cube = nullptr;
  size_t n_slices = 0, h = 0, w = 0, stride = 0, slice_stride = 0, ph = 0, pw = 0;
  const uint32_t *d_seeds_rc = nullptr;
  const size_t *seed_offsets = nullptr;
  const ws_options *opt = nullptr;

  size_t plane() const { return ph * pw; }
  const uint8_t *image(size_t k) const { return d_cube + k * slice_stride; }
  size_t seeds_in(size_t k0, size_t g) const { return seed_offsets[k0 + g] - seed_offsets[k0]; }      // of slices [k0, k0 + g)
  const uint32_t *seeds(size_t k) const { return seeds_in(k, 1) ? d_seeds_rc + 2 * seed_offsets[k] : nullptr; }
  bool missing_input() const { return n_slices && ((!d_cube && h * w) || (!d_seeds_rc && seeds_in(0, n_slices))); }
};

}  // namespace wsapi

using namespace wsapi;

namespace {

// how every cube entry point opens: a context with no transform in flight, no slice blamed yet
int open_batch(ws_ctx *c, size_t *failed_slice) {
  if (int busy_rc = refuse_if_in_flight(c)) return busy_rc;
  if (!c) return WS_ERR_BAD_ARG;
  if (failed_slice) *failed_slice = 0;
  return WS_OK;
}

// What every batch entry point checks before anything runs, check_plane included, and the batch it describes.  The host forms
// pass no device pointers and, without a seed list, n_slices 0: upload_batch completes their batch.  empty_has_plane false: the
// plane of a batch without slices is not looked at (the label and list forms leave that to their slices).
int check_batch(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, Batch *b, bool empty_has_plane = true) {
  if (n_slices && !seed_offsets) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (!opt) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (int v = ws_options_validate(opt)) return fail(c, v, ws_strerror(v));
  if (n_slices > 1 && slice_stride < h * row_stride) return fail(c, WS_ERR_BAD_ARG, "slice_stride < h * row_stride");
  for (size_t k = 0; k < n_slices; ++k)
    if (seed_offsets[k + 1] < seed_offsets[k]) return fail(c, WS_ERR_BAD_ARG, "seed_offsets must not decrease");
  *b = Batch{d_cube, n_slices, h, w, row_stride, slice_stride, 0, 0, d_seeds_rc, seed_offsets, opt};
  if (n_slices == 0 && !empty_has_plane) return WS_OK;
  return check_plane(c, h, w, row_stride, opt, &b->ph, &b->pw);
}

// Whether the batch runs as stacks: contiguous slices flooded as ONE plane of g * h rows whose slice border rows are walls (they
// are image-border rows of their slices: never flooded), one set of launches and one host round trip instead of g of each
// (8 x 4096^2: 2.0 -> ~1.4 ms; 16 x 1024^2: 2.2 ms -> ~0.3 ms).  Needs strictly increasing seed lists (the side-table form),
// w % 4 == 0, h * w % 128 == 0 and a seed in every group.  Returns the slices of a group (batch_max_px / plane); 0: the
// slice-by-slice loop takes the batch.
size_t stackable(ws_ctx *c, const Batch &b) {
  static const bool off = tuning_env("WS_NO_BATCH_STACK") != nullptr || tuning_env("WS_NO_SEED_TABLES") != nullptr;      // A/B knobs for tools/
  const size_t plane = b.plane();
  if (off || b.n_slices < 2 || b.slice_stride != b.h * b.stride || !b.d_cube || !b.d_seeds_rc || pick_engine(b.opt) != WS_ENGINE_FUSED ||
      !c->expect_sorted || (b.pw & 3) != 0 || plane == 0 || plane % 128 != 0 || plane >= 0x40000000ull || b.stride != b.w || b.h * b.w == 0)
    return 0;
  if (b.seeds_in(0, b.n_slices) >= 0xFFFFFFFFull) return 0;
  const size_t per_group = std::max<size_t>(1, c->batch_max_px / plane);      // (<= 2^31 - 1 pixels: the two-launch resolve indexes them with 31 bits)
  for (size_t k0 = 0; k0 < b.n_slices; k0 += per_group)      // (a flood needs a seed)
    if (b.seeds_in(k0, std::min(per_group, b.n_slices - k0)) == 0) return 0;
  return per_group;
}

// Slices [k_first, k_first + g) of a batch with ns seeds, their transform left on the context: a stack (labels restart at 1 in
// every slice; colour c of slice k_first + k is c + base[k] in the stack's numbering; first: the bases on the host) or one slice
// of the loop (g == 1, base and first null)
struct BatchGroup {
  size_t k_first, g, ns;
  const uint32_t *keys;
  uint32_t *labels;
  const uint32_t *base, *first;
};

// The flood of slices [k0, k0 + g) as one stack (flood_stack) into `labels`; first (g + 1): every slice's first seed within the
// group.  true: flooded, and the statistics span is still OPEN -- the products differ in where they close it.  false: the flood
// failed or mispredicted; the span is closed, the error cleared, and the slice-by-slice loop repeats the work and names the slice.
bool flood_group(ws_ctx *c, const Batch &b, size_t k0, size_t g, uint32_t *labels, std::vector<uint32_t> &first) {
  const size_t s0 = b.seed_offsets[k0];
  first.resize(g + 1);
  for (size_t k = 0; k <= g; ++k) first[k] = (uint32_t)(b.seed_offsets[k0 + k] - s0);
  stats_begin(c);
  bool mispredicted = false;
  const int rc = flood_stack(c, b.image(k0), b.stride, g, b.ph, b.pw, b.d_seeds_rc + 2 * s0, first.data(), b.opt, labels, &mispredicted);
  c->have_keys = false;      // the stamps are those of a stack, not of an image
  if (rc == WS_OK && !mispredicted) return true;
  (void)stats_end(c);
  c->err.clear();
  return false;
}

// closes the span flood_group left open and adds the group's statistics to the batch's
int close_span(ws_ctx *c, ws_stats &acc) {
  if (int rc = stats_end(c)) return rc;
  stats_add(acc, c->stats);
  return WS_OK;
}

// A batch, run: per_group != 0 (stackable) as stacks, group by group -- ensure(g, ns) before the flood, the flood into the caller's
// planes at d_labels (null: the context's stack_labels), then group(BatchGroup, acc) with the statistics span open.  A stack that
// fails or mispredicts is abandoned, whatever its earlier groups have written, and the batch runs again slice by slice, as does a
// batch that does not stack: slice(k) is the single-field transform of slice k, and the slice whose transform fails is named.
// Statistics are summed (the groups add their own to acc, close_span; the slices' are added here), and the stamps left on the
// context are no single image's.
template <class G, class S, class E = int (*)(size_t, size_t)>
int run_batch(ws_ctx *c, const Batch &b, size_t per_group, size_t *failed_slice, uint32_t *d_labels, G group, S slice,
              E ensure_for = [](size_t, size_t) { return (int)WS_OK; }) {
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t plane = b.plane();
  ws_stats acc{};
  std::vector<uint32_t> first;
  bool stacked = per_group != 0;
  for (size_t k0 = 0; stacked && k0 < b.n_slices; k0 += per_group) {
    const size_t g = std::min(per_group, b.n_slices - k0), ns = b.seeds_in(k0, g);
    if (!d_labels)
      if (int rc = ensure(c, c->stack_labels, g * plane * sizeof(uint32_t))) return rc;
    if (int rc = ensure_for(g, ns)) return rc;
    uint32_t *labels = d_labels ? d_labels + k0 * plane : (uint32_t *)c->stack_labels.p;
    stacked = flood_group(c, b, k0, g, labels, first);
    if (stacked)
      if (int rc = group(BatchGroup{k0, g, ns, (const uint32_t *)c->keys.p, labels, stacked_first(c, ns), first.data()}, acc)) return rc;
  }
  if (stacked) {
    c->stats = acc;
    return WS_OK;
  }
  acc = ws_stats{};
  for (size_t k = 0; k < b.n_slices; ++k) {
    if (int rc = slice(k)) {
      if (failed_slice) *failed_slice = k;
      return rc;
    }
    stats_add(acc, c->stats);
  }
  c->stats = acc;
  c->have_keys = false;
  return WS_OK;
}

// The arrival-form job of a flooded stack: the per-level driver over the stack's numbering of colours (the bucketing adds the
// slice's base to every colour and pairs no pixels across a slice border)
LevelJob stack_job(bool merging, const Batch &b, const BatchGroup &grp) {
  LevelJob job = LevelJob::from_arrival(merging, grp.keys, grp.labels, grp.g * b.ph, b.pw, grp.ns, b.opt);
  job.slice_h = (int)b.ph; job.d_slice_base = grp.base;
  return job;
}

// ---- final labels of a cube: ws_segment_batch_device, ws_merge_batch_device ----------------------------------------------------------

// ws_merge_batch_device: a flooded group's unions of the final level over the stack's numbering of colours and a relabel back to
// every slice's own (merge_stack); one ws_merge_device per slice
int merge_batch_body(ws_ctx *c, const Batch &b, uint32_t *d_labels, size_t *failed_slice) {
  const size_t plane = b.plane();
  return run_batch(
      c, b, d_labels ? stackable(c, b) : 0, failed_slice, d_labels,
      [&](const BatchGroup &grp, ws_stats &acc) -> int {
        HIP_TRY(c, uf_init(c->stream, (uint32_t *)c->uf_parent.p, (uint32_t *)c->uf_size.p, grp.ns + 1));
        {
          Span sp(c, KC_OTHER);
          HIP_TRY(c, merge_stack(c->stream, grp.labels, (int)b.ph, (int)b.pw, grp.g, grp.base, (uint32_t *)c->uf_parent.p, grp.ns + 1));
        }
        acc.merge_levels = 1;
        return close_span(c, acc);
      },
      [&](size_t k) { return ws_merge_device(c, b.image(k), b.h, b.w, b.stride, b.seeds(k), b.seeds_in(k, 1), b.opt, d_labels + k * plane); },
      [&](size_t, size_t ns) { return ensure_uf(c, ns + 1); });
}

// ---- transform_to_list of a cube (ws_transform_to_list_batch(_device)) ------------------------------------------------------------------

// Per group: the per-level driver on the stack (merge_host, arrival form), then the split of the group's records (level-major,
// stack colours) into the caller's slice-major layout in the slices' own colours; per slice: ws_transform_to_list_device, its
// records behind the previous slices'.  Records past cap are counted, not written: the caller learns how many to make room for.
int lists_batch_body(ws_ctx *c, bool merging, const Batch &b, ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets,
                     uint64_t *uncoloured, size_t *failed_slice) {
  const size_t plane = b.plane();
  const uint32_t levels = (uint32_t)b.opt->max_water_level + 1;
  size_t need = 0;      // records of the groups or slices so far; while need <= cap they are in d_lakes[0 .. need)
  std::vector<uint64_t> goff(levels + 1), gunc(levels);
  std::vector<u64c> bins;
  const auto room = [&] { return need <= cap ? cap - need : 0; };
  const int rc_run = run_batch(
      c, b, stackable(c, b), failed_slice, nullptr,
      [&](const BatchGroup &grp, ws_stats &acc) -> int {
        int rc = close_span(c, acc);
        if (rc) return rc;
        const size_t g = grp.g, ns = grp.ns, n_bins = g * levels;
        u64c *d_off = (u64c *)c->stack_bins.p, *d_bins = d_off + levels + 1, *d_hist = d_bins + n_bins;
        HIP_TRY(c, hipMemsetAsync(d_bins, 0, (n_bins + g * NLEVELS) * sizeof(u64c), c->stream));
        HIP_TRY(c, slice_arrivals(c->stream, grp.keys, plane, g, d_hist));
        size_t got = 0;
        rc = merge_host(c, stack_job(merging, b, grp).with_lists((ws_lake *)c->stack_records.p, room(), &got, goff.data(), gunc.data()));
        if (rc != WS_OK && rc != WS_ERR_CAPACITY) return rc;
        stats_add(acc, c->stats);
        need += got;
        if (rc == WS_ERR_CAPACITY || need > cap) {      // counted, not written
          c->err.clear();
          return WS_OK;
        }
        // counts per (slice, level) -> the bins' first records in the caller's layout, which the scatter takes as its cursors.
        // A bin holds at most one record per colour of its slice; segmenting lists that have ALL of them (every seed owns its pixel
        // from level 0 on: the usual case) are known without a pass over the records.
        HIP_TRY(c, hipMemcpyAsync(d_off, goff.data(), (levels + 1) * sizeof(u64c), hipMemcpyHostToDevice, c->stream));
        const bool full = !merging && got == (size_t)levels * ns;
        if (!full)
          HIP_TRY(c, split_records(c->stream, false, (const uint64_t *)c->stack_records.p, got, d_off, levels, grp.base, (uint32_t)g, d_bins, nullptr));
        bins.resize(n_bins + g * NLEVELS);
        HIP_TRY(c, hipMemcpyAsync(bins.data(), d_bins, bins.size() * sizeof(u64c), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        if (full)
          for (size_t k = 0; k < g; ++k)
            for (uint32_t l = 0; l < levels; ++l) bins[k * levels + l] = grp.first[k + 1] - grp.first[k];
        u64c at = need - got;
        for (size_t i = 0; i < n_bins; ++i) {
          const u64c count = bins[i];
          offsets[grp.k_first * levels + i] = at;
          bins[i] = at;
          at += count;
        }
        if (at != need) return fail(c, WS_ERR_HIP, "internal: the split of the stack's records lost some");
        for (size_t k = 0; k < g; ++k) {      // index 0 of lib.rs:630's vector: the slice's pixels not yet coloured
          u64c arrived = 0;
          for (uint32_t l = 0; l < levels; ++l) {
            arrived += bins[n_bins + k * NLEVELS + l];
            uncoloured[(grp.k_first + k) * levels + l] = plane - arrived;
          }
        }
        HIP_TRY(c, hipMemcpyAsync(d_bins, bins.data(), n_bins * sizeof(u64c), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(c, split_records(c->stream, true, (const uint64_t *)c->stack_records.p, got, d_off, levels, grp.base, (uint32_t)g, d_bins,
                                 (uint64_t *)d_lakes));
        HIP_TRY(c, hipStreamSynchronize(c->stream));      // `bins` and `goff` are the next group's
        return WS_OK;
      },
      [&](size_t k) -> int {
        if (k == 0) need = 0;      // (after an abandoned stack: from the start)
        size_t got = 0;
        const int rc = ws_transform_to_list_device(c, merging, b.image(k), b.h, b.w, b.stride, b.seeds(k), b.seeds_in(k, 1), b.opt,
                                                   need <= cap ? d_lakes + need : nullptr, room(), &got, goff.data(), uncoloured + k * levels);
        if (rc != WS_OK && rc != WS_ERR_CAPACITY) return rc;
        for (size_t l = 0; l < levels; ++l) offsets[k * levels + l] = need + goff[l];
        need += got;
        return WS_OK;
      },
      [&](size_t g, size_t) -> int {
        if (int rc = ensure(c, c->stack_records, std::max<size_t>(room(), 1) * sizeof(ws_lake))) return rc;
        return ensure(c, c->stack_bins, (levels + 1 + g * levels + g * NLEVELS) * sizeof(u64c));
      });
  if (rc_run) return rc_run;
  offsets[b.n_slices * levels] = need;
  *n_lakes = need;
  if (need > cap) return fail(c, WS_ERR_CAPACITY, "lake buffer too small");
  c->err.clear();
  return WS_OK;
}

// The host forms' inputs on the device, as the device forms take them: the cube as contiguous slices (c->batch_cube) and the
// seeds as u32 pairs (c->batch_seeds) -- seeds_rc == NULL: every slice's own find_local_minima (lib.rs:1178-1197), its seeds
// behind the previous slices'.  b (checked: its h, w and plane) becomes that batch; offs (n_slices + 1): its seed offsets;
// n_seeds (nullable): the counts.  The stacked minima keep the nibble plane of a whole run on the context (ws_find_local_minima_batch_device).
int upload_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t row_stride, size_t slice_stride, const uint64_t *seeds_rc,
                 const size_t *seed_offsets, Batch &b, std::vector<size_t> &offs, size_t *n_seeds, size_t *failed_slice) {
  int rc;
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t h = b.h, w = b.w, hw = h * w;
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
    // every slice's minima in one stacked call: one count, scan and write launch and one readback per run of slices
    size_t found = 0;
    if (bound && (rc = ws_find_local_minima_batch_device(c, d_cube, n_slices, h, w, w, hw, (uint32_t *)c->batch_seeds.p, n_slices * bound, offs.data(), &found)))
      return rc;      // (a failure of the stacked call belongs to no one slice: *failed_slice is left as it was)
  }
  if (n_seeds)
    for (size_t k = 0; k < n_slices; ++k) n_seeds[k] = offs[k + 1] - offs[k];
  b.d_cube = d_cube; b.n_slices = n_slices; b.stride = w; b.slice_stride = hw;
  b.d_seeds_rc = (const uint32_t *)c->batch_seeds.p; b.seed_offsets = offs.data();
  return WS_OK;
}

// ---- transform_history of a cube of slices (ws_transform_history_batch(_device)) ---------------------------------------------------

// slices [ka, kb) of the group (plane pixels each), tab's levels, into out: slice ka + r's plane of slot j at out + (r * per_slice + j) * plane_stride
int render_group(ws_ctx *c, bool merging, const BatchGroup &grp, size_t plane, size_t ka, size_t kb, const HistoryTable &tab, uint32_t *out,
                 size_t per_slice, size_t plane_stride) {
  if (!grp.base) return render_levels(c, merging, tab, out, plane_stride, plane);
  const HistoryStack st{grp.base + ka, (uint32_t)plane, (uint32_t)per_slice};
  HIP_TRY(c, render_history_stack(c->stream, merging, grp.keys + ka * plane, grp.labels + ka * plane, (const uint32_t *)c->uf_death.p,
                                  (const uint32_t *)c->uf_hook.p, tab, out, plane_stride, (kb - ka) * plane, st));
  return WS_OK;
}

// The transforms of a batch for transform_history, each handed to emit(BatchGroup) while its planes can be rendered: a flooded
// group after, merging, ONE run of the stamping per-level driver over the stack's numbering of colours (merge_host, arrival form,
// history: no pair crosses a slice border, so no lake either); a slice of the loop after the transform of ws_transform_history_device.
template <class F>
int history_batch_run(ws_ctx *c, bool merging, const Batch &b, size_t per_group, size_t *failed_slice, F emit) {
  return run_batch(
      c, b, per_group, failed_slice, nullptr,
      [&](const BatchGroup &grp, ws_stats &acc) -> int {
        if (int rc = close_span(c, acc)) return rc;
        if (merging) {
          if (int rc = merge_host(c, stack_job(true, b, grp).with_history())) return rc;
          stats_add(acc, c->stats);
        }
        return emit(grp);
      },
      [&](size_t k) -> int {
        const size_t ns = b.seeds_in(k, 1);
        if (int rc = merge_host(c, LevelJob::from_device(merging, b.image(k), b.h, b.w, b.stride, b.seeds(k), ns, b.opt).with_history())) return rc;
        return emit(BatchGroup{k, 1, ns, (const uint32_t *)c->keys.p, (uint32_t *)c->labels.p, nullptr, nullptr});
      });
}

// ---- merge_tree of a cube of slices (ws_merge_tree_batch(_device)) ----------------------------------------

// the records of a stacked group from the transform history_batch_run has just run on this context, into the caller's layout at d_tree
int build_tree_stack(ws_ctx *c, const BatchGroup &grp, const Batch &b, ws_tree_node *d_tree) {
  const uint32_t levels = (uint32_t)b.opt->max_water_level + 1;
  const size_t plane = b.plane(), ns = grp.ns;
  const uint32_t *death = (const uint32_t *)c->uf_death.p, *hook = (const uint32_t *)c->uf_hook.p;
  u64c *ws = (u64c *)c->tree_ws.p, *hist = ws + TREE_WS_WORDS;      // (behind the fold's counters: arrivals per (slice, level))
  TreeRec *forest = (TreeRec *)c->tree_forest.p;
  const TreeStack st{grp.base, (uint32_t)grp.g, (uint32_t)plane};
  Span sp(c, KC_OTHER);
  HIP_TRY(c, hipMemsetAsync(ws, 0, (TREE_WS_WORDS + grp.g * NLEVELS) * sizeof(u64c), c->stream));
  HIP_TRY(c, slice_arrivals(c->stream, grp.keys, plane, grp.g, hist));
  HIP_TRY(c, tree_init_stack(c->stream, death, hook, (const uint32_t *)c->seed_stack.p, grp.labels, (int)(grp.g * b.ph), (int)b.pw, forest, ns + 1, ws, st));
  HIP_TRY(c, tree_own_counts_stack(c->stream, grp.keys, grp.labels, death, hook, forest, grp.g * plane, st));
  HIP_TRY(c, tree_fold(c->stream, forest, ns + 1, levels, ws, (uint32_t *)c->tree_order.p));      // ONE launch per level for the group
  HIP_TRY(c, tree_unstack(c->stream, forest, ns, grp.base, grp.g, hist, levels, plane, reinterpret_cast<TreeRec *>(d_tree)));
  return WS_OK;
}

// ---- merge_tree_stats of a cube of slices (ws_merge_tree_stats_batch(_device)) ------------------------------

// the statistics request of a batch: the weight cube (null: the image cube itself, u8) with its strides in elements, and where the
// records go (the layout of the tree's) -- device pointers in the device form, host pointers in the host form.  with_shapes
// (ws_merge_tree_shapes_batch(_device)): the second moments too, from the same weights, into `shapes` in the same layout
struct LakeBatchWanted {
  const void *weight = nullptr;
  int dtype = 0;
  size_t stride = 0, slice_stride = 0;
  ws_lake_stats *stats = nullptr;
  bool with_shapes = false;
  ws_lake_shape *shapes = nullptr;
};

// what both forms check after check_batch, before anything runs: the weights as check_lake_weights for one slice's plane (the
// 64-bit bound is a slice's: rows and columns restart in every slice), their slice stride as check_batch treats the cube's
int check_lake_batch(ws_ctx *c, size_t n_slices, const Batch &b, const LakeBatchWanted &ls) {
  if (int rc = check_lake_weights(c, b.w, b.ph, b.pw, ls.weight, ls.dtype, ls.stride)) return rc;
  if (ls.weight && n_slices > 1 && ls.slice_stride < b.h * ls.stride) return fail(c, WS_ERR_BAD_ARG, "weight_slice_stride < h * weight_row_stride");
  return WS_OK;
}

// the weights of slices k .. of the batch: the request's cube, or the image cube read as u8 with its own strides
LakeWeights lake_weights_from(const LakeBatchWanted &ls, const Batch &b, size_t k) {
  const uint32_t off = b.opt->edge_correction ? 1u : 0u;
  if (!ls.weight) return LakeWeights{b.image(k), b.stride, (uint32_t)b.h, (uint32_t)b.w, off, 0, b.slice_stride};
  const size_t elem = ls.dtype == WS_U16 ? 2 : 1;
  return LakeWeights{(const uint8_t *)ls.weight + k * ls.slice_stride * elem, ls.stride, (uint32_t)b.h, (uint32_t)b.w, off, ls.dtype == WS_U16, ls.slice_stride};
}

// the statistics of the forest build_tree_stack has just folded in c->tree_forest (tree_fold's buckets are still in c->tree_ws and
// c->tree_order), into the caller's layout at d_stats
int build_lake_stats_stack(ws_ctx *c, const BatchGroup &grp, const Batch &b, const LakeWeights &wt, ws_lake_stats *d_stats) {
  const TreeStack st{grp.base, (uint32_t)grp.g, (uint32_t)b.plane()};
  Span sp(c, KC_OTHER);
  HIP_TRY(c, lake_stats_stack(c->stream, grp.keys, grp.labels, (const uint32_t *)c->uf_death.p, (const uint32_t *)c->uf_hook.p,
                              (const TreeRec *)c->tree_forest.p, (const uint32_t *)c->seed_stack.p, grp.ns + 1, (uint32_t)b.opt->max_water_level + 1,
                              (const u64c *)c->tree_ws.p, (const uint32_t *)c->tree_order.p, wt, st, (int)b.pw, c->lake_acc.p,
                              reinterpret_cast<LakeRec *>(d_stats)));
  return WS_OK;
}

// the shapes of the same forest, after build_lake_stats_stack (the buckets are still where tree_fold left them), into the caller's
// layout at d_shapes
int build_lake_shapes_stack(ws_ctx *c, const BatchGroup &grp, const Batch &b, const LakeWeights &wt, ws_lake_shape *d_shapes) {
  const TreeStack st{grp.base, (uint32_t)grp.g, (uint32_t)b.plane()};
  Span sp(c, KC_OTHER);
  HIP_TRY(c, lake_shapes_stack(c->stream, grp.keys, grp.labels, (const uint32_t *)c->uf_death.p, (const uint32_t *)c->uf_hook.p,
                               (const TreeRec *)c->tree_forest.p, (const uint32_t *)c->seed_stack.p, grp.ns + 1, (uint32_t)b.opt->max_water_level + 1,
                               (const u64c *)c->tree_ws.p, (const uint32_t *)c->tree_order.p, wt, st, (int)b.pw, c->shape_acc.p,
                               reinterpret_cast<ShapeRec *>(d_shapes)));
  return WS_OK;
}

// The trees of a batch into d_tree (device; slice k's n_k + 1 records from (seed_offsets[k] - seed_offsets[0]) + k on), every group's
// segmenting labels handed to labels(BatchGroup) while they are on the context; with ls, every group's statistics into
// ls->stats (device) in the same layout -- a stacked group's from the forest (lake_stats_stack: one fold launch per level for the group),
// a looped slice's as ws_merge_tree_stats_device's with that slice's weight plane; with ls->with_shapes, the shapes after them into
// ls->shapes, a stacked group's from the same forest and buckets (lake_shapes_stack), a looped slice's as
// ws_merge_tree_shapes_device's.  Every buffer the tree and statistics kernels
// need is sized for the largest group BEFORE the first transform (nothing moves under the level loop's captured graphs).
template <class F>
int tree_batch_run(ws_ctx *c, const Batch &b, ws_tree_node *d_tree, size_t *failed_slice, F labels, const LakeBatchWanted *ls) {
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t per_group = std::min(stackable(c, b), b.n_slices);
  size_t most = 0, most_group = 0;
  for (size_t k = 0; k < b.n_slices; ++k) most = std::max(most, b.seeds_in(k, 1));
  for (size_t k0 = 0; per_group && k0 < b.n_slices; k0 += per_group) most_group = std::max(most_group, b.seeds_in(k0, std::min(per_group, b.n_slices - k0)));
  int rc;
  if ((rc = ensure(c, c->tree_order, (std::max(most, most_group) + 1) * sizeof(uint32_t)))) return rc;
  if ((rc = ensure(c, c->tree_ws, (TREE_WS_WORDS + per_group * NLEVELS) * sizeof(u64c)))) return rc;
  if (per_group) {
    if ((rc = ensure(c, c->tree_forest, (most_group + 1) * sizeof(TreeRec)))) return rc;
    if ((rc = ensure(c, c->seed_stack, (most_group * 2 + per_group + 1) * sizeof(uint32_t)))) return rc;      // (flood_stack's, for its largest group)
  }
  // (the accumulator planes: a group's colours, the forest's entry 0 and one record 0 per slice of the group)
  if (ls && (rc = ensure(c, c->lake_acc, (std::max(most, most_group) + 1 + per_group) * LAKE_ACC_BYTES))) return rc;
  const bool shapes = ls && ls->with_shapes;
  if (shapes && (rc = ensure(c, c->shape_acc, (std::max(most, most_group) + 1 + per_group) * SHAPE_ACC_BYTES))) return rc;
  return history_batch_run(c, true, b, per_group, failed_slice, [&](const BatchGroup &grp) -> int {
    const size_t k = grp.k_first, at = b.seeds_in(0, k) + k;
    ws_tree_node *out = d_tree + at;
    ws_lake_stats *out_stats = ls ? ls->stats + at : nullptr;
    ws_lake_shape *out_shapes = shapes ? ls->shapes + at : nullptr;
    if (grp.base) {
      if (int rc_t = build_tree_stack(c, grp, b, out)) return rc_t;
      if (ls)
        if (int rc_t = build_lake_stats_stack(c, grp, b, lake_weights_from(*ls, b, k), out_stats)) return rc_t;
      if (shapes)
        if (int rc_t = build_lake_shapes_stack(c, grp, b, lake_weights_from(*ls, b, k), out_shapes)) return rc_t;
    } else {
      // the seed pairs as the flood took them: the caller's, or (shifted_seeds) moved into the padded plane
      const uint32_t *seeds = seed_shift_of(b.opt) && grp.ns ? (const uint32_t *)c->seeds.p : b.d_seeds_rc + 2 * b.seed_offsets[k];
      if (int rc_t = build_tree(c, grp.keys, grp.labels, seeds, grp.ns, b.opt, b.ph, b.pw, out)) return rc_t;
      if (ls)
        if (int rc_t = build_lake_stats(c, grp.keys, grp.labels, seeds, grp.ns, b.opt, b.ph, b.pw, out, lake_weights_from(*ls, b, k), out_stats)) return rc_t;
      if (shapes)
        if (int rc_t = build_lake_shapes(c, grp.keys, grp.labels, seeds, grp.ns, b.opt, b.ph, b.pw, out, lake_weights_from(*ls, b, k), out_shapes)) return rc_t;
    }
    return labels(grp);
  });
}

// ws_merge_tree_batch_device, with ls ws_merge_tree_stats_batch_device and, with ls->with_shapes, ws_merge_tree_shapes_batch_device
int tree_batch_device_body(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                           const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_tree_node *d_tree, uint32_t *d_labels,
                           size_t *failed_slice, LakeBatchWanted *ls) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  Batch b;
  if (int rc = check_batch(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, &b)) return rc;
  if (ls)
    if (int rc = check_lake_batch(c, n_slices, b, *ls)) return rc;
  if (n_slices == 0) return WS_OK;
  if (b.seeds_in(0, n_slices) >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (!d_tree || (ls && !ls->stats) || (ls && ls->with_shapes && !ls->shapes) || b.missing_input()) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (ls && ls->with_shapes && (reinterpret_cast<uintptr_t>(ls->shapes) & 7u)) return fail(c, WS_ERR_BAD_ARG, "d_shapes is not 8-byte aligned");
  if (ls && h * w == 0) ls->weight = nullptr;
  const size_t plane = b.plane();
  const auto labels_to_caller = [&](const BatchGroup &grp) -> int {
    if (d_labels && plane)
      HIP_TRY(c, hipMemcpyAsync(d_labels + grp.k_first * plane, grp.labels, grp.g * plane * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return WS_OK;
  };
  if (int rc = tree_batch_run(c, b, d_tree, failed_slice, labels_to_caller, ls)) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

// the host forms' weight cube contiguous on the context (c->lake_weight), before the first transform: nothing moves under the level
// loop's graphs; ls then describes it.  No weights or no pixel: ls keeps none (the cube itself weighs)
int upload_weights(ws_ctx *c, const LakeBatchWanted &want, size_t n_slices, size_t h, size_t w, LakeBatchWanted &ls) {
  if (!want.weight || h * w == 0) return WS_OK;
  const size_t elem = want.dtype == WS_U16 ? 2 : 1;
  if (int rc = ensure(c, c->lake_weight, n_slices * h * w * elem)) return rc;
  for (size_t k = 0; k < n_slices; ++k)
    HIP_TRY(c, hipMemcpy2DAsync((uint8_t *)c->lake_weight.p + k * h * w * elem, w * elem, (const uint8_t *)want.weight + k * want.slice_stride * elem,
                                want.stride * elem, w * elem, h, hipMemcpyHostToDevice, c->stream));
  ls.weight = c->lake_weight.p; ls.dtype = want.dtype; ls.stride = w; ls.slice_stride = h * w;
  return WS_OK;
}

// ws_merge_tree_batch, with want (host pointers) ws_merge_tree_stats_batch and, with want->with_shapes, ws_merge_tree_shapes_batch:
// the inputs to the device, the device form's run into the context's record buffers, the records back, one copy an array.  A cap below the need is counted, nothing flooded: the caller learns how
// many records to make room for.
int tree_batch_host_body(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                         const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_tree_node *tree, size_t cap, size_t *n_records,
                         uint64_t *labels, size_t *n_seeds, size_t *failed_slice, const LakeBatchWanted *want) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  Batch b;
  int rc = check_batch(c, nullptr, seeds_rc ? n_slices : 0, h, w, row_stride, slice_stride, nullptr, seed_offsets, opt, &b);
  if (rc) return rc;
  if (want && (rc = check_lake_batch(c, n_slices, b, *want))) return rc;
  if (n_slices == 0) {
    if (n_records) *n_records = 0;
    return WS_OK;
  }
  const bool shapes = want && want->with_shapes;
  if ((!cube && h * w) || ((!tree || (want && !want->stats) || (shapes && !want->shapes)) && cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (seeds_rc && seed_offsets[n_slices] - seed_offsets[0] >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  std::vector<size_t> offs;
  if ((rc = upload_batch(c, cube, n_slices, row_stride, slice_stride, seeds_rc, seed_offsets, b, offs, n_seeds, failed_slice))) return rc;
  const size_t total = offs[n_slices] + n_slices, plane = b.plane();
  if (n_records) *n_records = total;
  if (offs[n_slices] >= 0xFFFFFFFFull) return fail(c, WS_ERR_TOO_LARGE, "too many seeds");
  if (cap < total) return fail(c, WS_ERR_CAPACITY, want ? "record buffers too small" : "tree buffer too small");
  if ((rc = ensure(c, c->tree_out, total * sizeof(ws_tree_node)))) return rc;
  if (want && (rc = ensure(c, c->lake_out, total * sizeof(ws_lake_stats)))) return rc;
  if (shapes && (rc = ensure(c, c->shape_out, total * sizeof(ws_lake_shape)))) return rc;
  if (labels && (rc = ensure(c, c->out64, std::max<size_t>(plane, 1) * sizeof(uint64_t)))) return rc;      // (the plane-by-plane copy widens there)
  LakeBatchWanted ls;
  ls.stats = (ws_lake_stats *)c->lake_out.p;
  ls.with_shapes = shapes; ls.shapes = (ws_lake_shape *)c->shape_out.p;
  if (want && (rc = upload_weights(c, *want, n_slices, h, w, ls))) return rc;
  const auto labels_to_caller = [&](const BatchGroup &grp) -> int {
    if (!labels || !plane) return WS_OK;
    return planes_to_host(c, grp.labels, labels + grp.k_first * plane, grp.g, plane);
  };
  if ((rc = tree_batch_run(c, b, (ws_tree_node *)c->tree_out.p, failed_slice, labels_to_caller, want ? &ls : nullptr))) return rc;
  HIP_TRY(c, hipMemcpyAsync(tree, c->tree_out.p, total * sizeof(ws_tree_node), hipMemcpyDeviceToHost, c->stream));
  if (want) HIP_TRY(c, hipMemcpyAsync(want->stats, c->lake_out.p, total * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  if (shapes) HIP_TRY(c, hipMemcpyAsync(want->shapes, c->shape_out.p, total * sizeof(ws_lake_shape), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

// ---- the cut catalogue of a cube of slices (ws_merge_tree_cut_catalogue_batch(_device)) ---------------------

// what the cube's cut writes, in HBM (the device form: the caller's; the host form: the context's) but for the host arrays
struct CutBatchOut {
  const ws_lake_cut *cuts = nullptr;
  size_t n_cuts = 0;
  uint32_t *d_keys_out = nullptr, *d_out = nullptr;
  size_t plane_stride = 0;
  ws_lake *d_lakes = nullptr;
  ws_lake_stats *d_region_stats = nullptr;
  size_t cap = 0, *n_lakes = nullptr;
  uint64_t *offsets = nullptr, *hidden = nullptr;
  ws_lake_stats *hidden_stats = nullptr;
  bool measure() const { return d_region_stats || hidden_stats; }
};

// the group's part of the request: its records, planes and outputs, lists and records behind `need` records of the groups before
CutCube cut_cube_of(const Batch &b, const CutBatchOut &o, const LakeBatchWanted &ls, const ws_tree_node *d_tree, const ws_lake_stats *d_stats,
                    size_t k_first, size_t g, const uint32_t *keys, const uint32_t *labels, size_t need) {
  const size_t at = k_first ? b.seeds_in(0, k_first) + k_first : 0, i0 = k_first * o.n_cuts, room = need <= o.cap ? o.cap - need : 0;
  CutCube q;
  q.d_tree = d_tree ? d_tree + at : nullptr; q.d_stats = d_stats ? d_stats + at : nullptr;
  q.n_slices = g; q.seed_offsets = b.seed_offsets ? b.seed_offsets + k_first : nullptr; q.d_keys = keys; q.d_seg_labels = labels; q.h = b.ph; q.w = b.pw;
  q.cuts = o.cuts; q.n_cuts = o.n_cuts;
  q.d_out = o.d_out ? o.d_out + i0 * o.plane_stride : nullptr; q.plane_stride = o.plane_stride;
  q.d_lakes = o.d_lakes ? o.d_lakes + (room ? need : 0) : nullptr;
  q.d_region_stats = o.d_region_stats ? o.d_region_stats + (room ? need : 0) : nullptr;
  q.cap = room; q.n_lakes = o.n_lakes; q.offsets = o.offsets ? o.offsets + i0 : nullptr; q.hidden = o.hidden ? o.hidden + i0 : nullptr;
  q.hidden_stats = o.hidden_stats ? o.hidden_stats + i0 : nullptr;
  q.measure = o.measure();
  if (q.measure) q.wt = lake_weights_from(ls, b, k_first);
  return q;
}

// The trees of a checked batch (tree_batch_run; with ls.stats the catalogue) and, per group while its stamps and labels are on the
// context, the cut: a stacked group as its g slices in ONE run of the cut's driver, a looped slice as one slice of it.  Lists and
// region records continue behind the previous groups'; once they no longer fit the remaining groups still flood and count
// (lists_batch_body's rule).  Every buffer of the cut is reserved for the largest group before the first transform.
template <class F>
int cut_batch_run(ws_ctx *c, const Batch &b, const LakeBatchWanted &ls, ws_tree_node *d_tree, const CutBatchOut &o, size_t *failed_slice, F labels) {
  HIP_TRY(c, hipSetDevice(c->device));
  const size_t plane = b.plane(), n_slices = b.n_slices;
  {
    const size_t per_group = std::max<size_t>(std::min(stackable(c, b), n_slices), 1);
    size_t most = 0;
    for (size_t k0 = 0; k0 < n_slices; k0 += per_group) most = std::max(most, b.seeds_in(k0, std::min(per_group, n_slices - k0)));
    for (size_t k = 0; k < n_slices; ++k) most = std::max(most, b.seeds_in(k, 1));
    if (int rc = cut_cube_reserve(c, per_group, most, per_group * plane, cut_cube_of(b, o, ls, d_tree, ls.stats, 0, per_group, nullptr, nullptr, 0))) return rc;
  }
  size_t need = 0;
  const int rc_run = tree_batch_run(
      c, b, d_tree, failed_slice,
      [&](const BatchGroup &grp) -> int {
        if (int rc = labels(grp)) return rc;
        if (grp.k_first == 0) need = 0;      // (after an abandoned stack: from the start)
        if (o.d_keys_out && plane)
          HIP_TRY(c, hipMemcpyAsync(o.d_keys_out + grp.k_first * plane, grp.keys, grp.g * plane * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
        size_t got = 0;
        CutCube q = cut_cube_of(b, o, ls, d_tree, ls.stats, grp.k_first, grp.g, grp.keys, grp.labels, need);
        if (q.d_lakes) q.n_lakes = &got;
        const int rc = cut_cube_run(c, q);
        if (rc != WS_OK && rc != WS_ERR_CAPACITY) return rc;
        if (rc == WS_ERR_CAPACITY) c->err.clear();      // counted, not written
        else if (q.d_lakes)
          for (size_t i = 0; i < grp.g * o.n_cuts; ++i) q.offsets[i] += need;
        need += got;
        return WS_OK;
      },
      ls.stats ? &ls : nullptr);
  if (rc_run) return rc_run;
  if (o.d_lakes) {
    *o.n_lakes = need;
    if (need > o.cap) return fail(c, WS_ERR_CAPACITY, "lake buffer too small");
    o.offsets[n_slices * o.n_cuts] = need;
  }
  return WS_OK;
}

// what both forms refuse of the cut before anything runs, after check_batch: the cuts and the outputs as the single call, the
// weights when something reads them, the totals
int check_cut_batch(ws_ctx *c, size_t n_slices, const Batch &b, const LakeBatchWanted &ls, bool with_stats, const CutBatchOut &o) {
  if (int rc = cut_cube_check(c, cut_cube_of(b, o, ls, nullptr, nullptr, 0, 0, nullptr, nullptr, 0), with_stats)) return rc;
  if (with_stats || o.measure())
    if (int rc = check_lake_batch(c, n_slices, b, ls)) return rc;
  const size_t plane = b.plane();
  if (o.d_out && o.plane_stride < plane) return fail(c, WS_ERR_BAD_ARG, "plane_stride is shorter than the plane");
  // (the host form without a seed list: its batch has no offsets yet, the seeds are counted once the minima are found)
  return cut_cube_sizes(c, n_slices, b.n_slices ? b.seeds_in(0, b.n_slices) : 0, plane, o.n_cuts, o.d_lakes != nullptr);
}

}  // namespace

extern "C" {

int ws_merge_tree_cut_catalogue_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                                             const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, const void *d_weight,
                                             int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride, const ws_lake_cut *cuts,
                                             size_t n_cuts, ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *d_labels, uint32_t *d_keys_out,
                                             uint32_t *d_out, size_t plane_stride, ws_lake *d_lakes, ws_lake_stats *d_region_stats, size_t cap,
                                             size_t *n_lakes, uint64_t *offsets, uint64_t *hidden, ws_lake_stats *hidden_stats, size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  Batch b;
  if (int rc = check_batch(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, &b)) return rc;
  LakeBatchWanted ls{d_weight, weight_dtype, weight_row_stride, weight_slice_stride, d_stats};
  CutBatchOut o;
  o.cuts = cuts; o.n_cuts = n_cuts; o.d_keys_out = d_keys_out; o.d_out = d_out; o.plane_stride = plane_stride; o.d_lakes = d_lakes;
  o.d_region_stats = d_region_stats; o.cap = cap; o.n_lakes = n_lakes; o.offsets = offsets; o.hidden = hidden; o.hidden_stats = hidden_stats;
  if (int rc = check_cut_batch(c, n_slices, b, ls, d_stats != nullptr, o)) return rc;
  if (n_slices == 0 || n_cuts == 0) return WS_OK;
  if (!d_tree || b.missing_input()) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  if (h * w == 0) ls.weight = nullptr;
  const size_t plane = b.plane();
  const auto labels_to_caller = [&](const BatchGroup &grp) -> int {
    if (d_labels && plane)
      HIP_TRY(c, hipMemcpyAsync(d_labels + grp.k_first * plane, grp.labels, grp.g * plane * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    return WS_OK;
  };
  const int rc = cut_batch_run(c, b, ls, d_tree, o, failed_slice, labels_to_caller);
  if (rc) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int ws_merge_tree_cut_catalogue_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                                      const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, const void *weight, int weight_dtype,
                                      size_t weight_row_stride, size_t weight_slice_stride, const ws_lake_cut *cuts, size_t n_cuts, ws_tree_node *tree,
                                      ws_lake_stats *stats, size_t record_cap, size_t *n_records, uint64_t *out, ws_lake *lakes,
                                      ws_lake_stats *region_stats, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden,
                                      ws_lake_stats *hidden_stats, size_t *n_seeds, size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  Batch b;
  int rc = check_batch(c, nullptr, seeds_rc ? n_slices : 0, h, w, row_stride, slice_stride, nullptr, seed_offsets, opt, &b);
  if (rc) return rc;
  const size_t plane = b.plane();
  bool catalogue = false;      // a cut with a catalogue threshold: the statistics run whether the caller wants the records or not
  for (size_t j = 0; cuts && j < std::min<size_t>(n_cuts, 32); ++j) catalogue = catalogue || cuts[j].min_sum_w || cuts[j].min_w_max || cuts[j].min_depth;
  const bool with_stats = stats || catalogue;
  const LakeBatchWanted want{weight, weight_dtype, weight_row_stride, weight_slice_stride, stats};
  CutBatchOut o;      // (the checks look at which outputs are wanted, not at where they are)
  o.cuts = cuts; o.n_cuts = n_cuts; o.d_out = (uint32_t *)out; o.plane_stride = plane; o.d_lakes = lakes; o.d_region_stats = region_stats;
  o.cap = cap; o.n_lakes = n_lakes; o.offsets = offsets; o.hidden = hidden; o.hidden_stats = hidden_stats;
  if ((rc = check_cut_batch(c, n_slices, b, want, with_stats, o))) return rc;
  if (n_slices == 0 || n_cuts == 0) {
    if (n_records) *n_records = 0;
    return WS_OK;
  }
  if ((!cube && h * w) || (!tree && record_cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  std::vector<size_t> offs;
  if ((rc = upload_batch(c, cube, n_slices, row_stride, slice_stride, seeds_rc, seed_offsets, b, offs, n_seeds, failed_slice))) return rc;
  const size_t total = offs[n_slices] + n_slices;
  if (n_records) *n_records = total;
  if ((rc = cut_cube_sizes(c, n_slices, offs[n_slices], plane, n_cuts, lakes != nullptr))) return rc;
  if (record_cap < total) return fail(c, WS_ERR_CAPACITY, "record buffers too small");
  if ((rc = ensure(c, c->tree_out, total * sizeof(ws_tree_node)))) return rc;
  if (with_stats && (rc = ensure(c, c->lake_out, total * sizeof(ws_lake_stats)))) return rc;
  if (out && plane && (rc = ensure(c, c->cut_planes, n_slices * n_cuts * plane * sizeof(uint32_t)))) return rc;
  if (out && (rc = ensure(c, c->out64, std::max<size_t>(plane, 1) * sizeof(uint64_t)))) return rc;      // (the plane-by-plane copy widens there)
  if (lakes && (rc = ensure(c, c->cut_lakes, std::max<size_t>(cap, 1) * sizeof(ws_lake)))) return rc;
  if (region_stats && (rc = ensure(c, c->cut_region, std::max<size_t>(cap, 1) * sizeof(ws_lake_stats)))) return rc;
  LakeBatchWanted ls;
  ls.stats = with_stats ? (ws_lake_stats *)c->lake_out.p : nullptr;
  if ((with_stats || o.measure()) && (rc = upload_weights(c, want, n_slices, h, w, ls))) return rc;
  o.d_out = out && plane ? (uint32_t *)c->cut_planes.p : nullptr;
  o.d_lakes = lakes ? (ws_lake *)c->cut_lakes.p : nullptr;
  o.d_region_stats = region_stats ? (ws_lake_stats *)c->cut_region.p : nullptr;
  if (!o.d_out && !o.d_lakes) {      // (planes of no pixel were all that was asked for: the transforms still run, for their errors)
    rc = tree_batch_run(c, b, (ws_tree_node *)c->tree_out.p, failed_slice, [](const BatchGroup &) { return (int)WS_OK; }, with_stats ? &ls : nullptr);
  } else {
    rc = cut_batch_run(c, b, ls, (ws_tree_node *)c->tree_out.p, o, failed_slice, [](const BatchGroup &) { return (int)WS_OK; });
  }
  if (rc) return rc;
  HIP_TRY(c, hipMemcpyAsync(tree, c->tree_out.p, total * sizeof(ws_tree_node), hipMemcpyDeviceToHost, c->stream));
  if (stats) HIP_TRY(c, hipMemcpyAsync(stats, c->lake_out.p, total * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  if (lakes && *n_lakes) HIP_TRY(c, hipMemcpyAsync(lakes, o.d_lakes, *n_lakes * sizeof(ws_lake), hipMemcpyDeviceToHost, c->stream));
  if (region_stats && *n_lakes) HIP_TRY(c, hipMemcpyAsync(region_stats, o.d_region_stats, *n_lakes * sizeof(ws_lake_stats), hipMemcpyDeviceToHost, c->stream));
  if (o.d_out)
    if ((rc = planes_to_host(c, o.d_out, out, n_slices * n_cuts, plane))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

// A stack's labels are final as flooded; one ws_segment_device per slice.  The statistics and the stamps left on the context
// are the last group's or slice's, as after that many single calls.
int ws_segment_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t stride,
                            size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets,
                            const ws_options *opt, uint32_t *d_labels, size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  if (n_slices == 0) return WS_OK;
  Batch b;
  if (int rc = check_batch(c, d_cube, n_slices, h, w, stride, slice_stride, d_seeds_rc, seed_offsets, opt, &b)) return rc;
  const size_t plane = b.plane();
  ws_stats last = c->stats;
  bool keys = c->have_keys;
  const int rc = run_batch(
      c, b, d_labels ? stackable(c, b) : 0, failed_slice, d_labels,
      [&](const BatchGroup &, ws_stats &) {
        const int rc_end = stats_end(c);
        last = c->stats; keys = false;
        return rc_end;
      },
      [&](size_t k) {
        const int rc_k = ws_segment_device(c, b.image(k), b.h, b.w, b.stride, b.seeds(k), b.seeds_in(k, 1), b.opt, d_labels + k * plane);
        last = c->stats; keys = c->have_keys;
        return rc_k;
      });
  c->stats = last;
  c->have_keys = keys;
  return rc;
}

int ws_merge_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                          const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, uint32_t *d_labels,
                          size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  Batch b;
  if (int rc = check_batch(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, &b, false)) return rc;
  return merge_batch_body(c, b, d_labels, failed_slice);
}

int ws_transform_to_list_batch_device(ws_ctx *c, int merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w,
                                      size_t row_stride, size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets,
                                      const ws_options *opt, ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets,
                                      uint64_t *uncoloured, size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  if (!n_lakes || !offsets || !uncoloured || (!d_lakes && cap)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  Batch b;
  if (int rc = check_batch(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, &b, false)) return rc;
  if (b.missing_input()) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  return lists_batch_body(c, merging != 0, b, d_lakes, cap, n_lakes, offsets, uncoloured, failed_slice);
}

int ws_transform_to_list_batch(ws_ctx *c, int merging, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                               size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                               ws_lake *lakes, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured, size_t *n_seeds,
                               size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  if (!n_lakes || !offsets || !uncoloured || (!lakes && cap) || (!cube && h * w && n_slices)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  Batch b;
  int rc = check_batch(c, nullptr, seeds_rc ? n_slices : 0, h, w, row_stride, slice_stride, nullptr, seed_offsets, opt, &b);
  if (rc) return rc;
  const size_t plane = b.plane();
  // the cube as contiguous slices, the seeds as u32 pairs (the device form's inputs), then the records back as ws_transform_to_list's are
  std::vector<size_t> offs;
  if ((rc = upload_batch(c, cube, n_slices, row_stride, slice_stride, seeds_rc, seed_offsets, b, offs, n_seeds, failed_slice))) return rc;
  if ((rc = ensure(c, c->lakes, std::max<size_t>(cap, 1) * sizeof(ws_lake)))) return rc;
  if ((rc = ensure(c, c->out64, std::max<size_t>(plane, 1) * sizeof(uint64_t)))) return rc;      // (the narrowed records' staging)
  if ((rc = lists_batch_body(c, merging != 0, b, (ws_lake *)c->lakes.p, cap, n_lakes, offsets, uncoloured, failed_slice))) return rc;
  if ((rc = records_to_host(c, (const ws_lake *)c->lakes.p, lakes, 0, *n_lakes, std::max<size_t>(plane, 1), c->stream))) return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return WS_OK;
}

int ws_transform_history_batch_device(ws_ctx *c, int merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                      size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                      const uint8_t *levels, size_t n_levels, uint32_t *d_out, size_t plane_stride, size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  Batch b;
  size_t n = 0;
  if (int rc = check_batch(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, &b)) return rc;
  if (int rc = check_history(c, h, w, row_stride, opt, levels, n_levels, &n)) return rc;
  if (plane_stride < n) return fail(c, WS_ERR_BAD_ARG, "plane_stride is shorter than the plane");
  if (n_levels == 0 || n_slices == 0) return WS_OK;
  if (b.missing_input() || (!d_out && n)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  // every slice's planes at once, straight into the caller's buffer
  const HistoryTable tab = history_table(levels, 0, n_levels);
  return history_batch_run(c, merging != 0, b, stackable(c, b), failed_slice, [&](const BatchGroup &grp) {
    return render_group(c, merging != 0, grp, n, 0, grp.g, tab, d_out + grp.k_first * n_levels * plane_stride, n_levels, plane_stride);
  });
}

int ws_transform_history_batch(ws_ctx *c, int merging, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                               size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                               const uint8_t *levels, size_t n_levels, uint64_t *out, size_t *n_seeds, size_t *failed_slice) {
  if (int rc_open = open_batch(c, failed_slice)) return rc_open;
  Batch b;
  size_t n = 0;
  int rc = check_batch(c, nullptr, seeds_rc ? n_slices : 0, h, w, row_stride, slice_stride, nullptr, seed_offsets, opt, &b);
  if (rc) return rc;
  if ((rc = check_history(c, h, w, row_stride, opt, levels, n_levels, &n))) return rc;
  if (n_levels == 0 || n_slices == 0) return WS_OK;
  if ((!cube && h * w) || (!out && n)) return fail(c, WS_ERR_BAD_ARG, "null pointer");
  std::vector<size_t> offs;
  if ((rc = upload_batch(c, cube, n_slices, row_stride, slice_stride, seeds_rc, seed_offsets, b, offs, n_seeds, failed_slice))) return rc;
  if (n == 0)      // (no pixel: the transforms still run, for their errors)
    return history_batch_run(c, merging != 0, b, stackable(c, b), failed_slice, [](const BatchGroup &) { return (int)WS_OK; });
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
  return history_batch_run(c, merging != 0, b, stackable(c, b), failed_slice, [&](const BatchGroup &grp) -> int {
    if (slices_per) {
      for (size_t ka = 0; ka < grp.g; ka += slices_per) {
        const size_t kb = std::min(ka + slices_per, grp.g);
        if (int rc_r = render_group(c, merging != 0, grp, n, ka, kb, all, planes, n_levels, n)) return rc_r;
        if (int rc_c = planes_to_host(c, planes, out + (grp.k_first + ka) * slice_words, (kb - ka) * n_levels, n)) return rc_c;
      }
      return WS_OK;
    }
    for (size_t k = 0; k < grp.g; ++k)
      for (size_t j0 = 0; j0 < n_levels; j0 += levels_per) {
        const size_t j1 = std::min(j0 + levels_per, n_levels);
        if (int rc_r = render_group(c, merging != 0, grp, n, k, k + 1, history_table(levels, j0, j1), planes, 0, n)) return rc_r;
        if (int rc_c = planes_to_host(c, planes, out + (grp.k_first + k) * slice_words + j0 * n, j1 - j0, n)) return rc_c;
      }
    return WS_OK;
  });
}

int ws_merge_tree_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                               const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_tree_node *d_tree,
                               uint32_t *d_labels, size_t *failed_slice) {
  return tree_batch_device_body(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, d_tree, d_labels, failed_slice, nullptr);
}

int ws_merge_tree_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                        const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_tree_node *tree, size_t cap,
                        size_t *n_records, uint64_t *labels, size_t *n_seeds, size_t *failed_slice) {
  return tree_batch_host_body(c, cube, n_slices, h, w, row_stride, slice_stride, seeds_rc, seed_offsets, opt, tree, cap, n_records, labels, n_seeds,
                              failed_slice, nullptr);
}

int ws_merge_tree_stats_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                     size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                     const void *d_weight, int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride,
                                     ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *d_labels, size_t *failed_slice) {
  LakeBatchWanted ls{d_weight, weight_dtype, weight_row_stride, weight_slice_stride, d_stats};
  return tree_batch_device_body(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, d_tree, d_labels, failed_slice, &ls);
}

int ws_merge_tree_stats_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                              const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, const void *weight, int weight_dtype,
                              size_t weight_row_stride, size_t weight_slice_stride, ws_tree_node *tree, ws_lake_stats *stats, size_t cap,
                              size_t *n_records, uint64_t *labels, size_t *n_seeds, size_t *failed_slice) {
  const LakeBatchWanted want{weight, weight_dtype, weight_row_stride, weight_slice_stride, stats};
  return tree_batch_host_body(c, cube, n_slices, h, w, row_stride, slice_stride, seeds_rc, seed_offsets, opt, tree, cap, n_records, labels, n_seeds,
                              failed_slice, &want);
}

int ws_merge_tree_shapes_batch_device(ws_ctx *c, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                      size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                      const void *d_weight, int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride,
                                      ws_tree_node *d_tree, ws_lake_stats *d_stats, ws_lake_shape *d_shapes, uint32_t *d_labels,
                                      size_t *failed_slice) {
  LakeBatchWanted ls{d_weight, weight_dtype, weight_row_stride, weight_slice_stride, d_stats, true, d_shapes};
  return tree_batch_device_body(c, d_cube, n_slices, h, w, row_stride, slice_stride, d_seeds_rc, seed_offsets, opt, d_tree, d_labels, failed_slice, &ls);
}

int ws_merge_tree_shapes_batch(ws_ctx *c, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                               const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, const void *weight, int weight_dtype,
                               size_t weight_row_stride, size_t weight_slice_stride, ws_tree_node *tree, ws_lake_stats *stats,
                               ws_lake_shape *shapes, size_t cap, size_t *n_records, uint64_t *labels, size_t *n_seeds, size_t *failed_slice) {
  const LakeBatchWanted want{weight, weight_dtype, weight_row_stride, weight_slice_stride, stats, true, shapes};
  return tree_batch_host_body(c, cube, n_slices, h, w, row_stride, slice_stride, seeds_rc, seed_offsets, opt, tree, cap, n_records, labels, n_seeds,
                              failed_slice, &want);
}

}  // extern "C"
