/*
 * ws_hip.h -- C ABI of the MI355X (gfx950) watershed engine.
 *
 * This is the drop-in boundary for ONE path of smups/rustronomy-watershed v0.4.1:
 * the segmenting / merging watershed transform and its seed finder.  The reference
 * has no FFI of its own (it is a single Rust file); the seam this ABI replaces is
 * the body of the private drivers behind the `Watershed<T>` trait.  Every entry
 * point cites the reference interface it stands in for ("lib.rs:N" =
 * src/lib.rs line N of the reference).  The Rust-side binding a maintainer would
 * add is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types;
 *   - images are row-major u8 with a row stride in bytes (>= w);
 *   - seeds are (row, col) pairs, two uint64_t per seed (Rust `(usize, usize)` repacked);
 *   - host-side label planes are uint64_t (Rust `usize` on x86-64), row-major,
 *     shape (h + 2e) x (w + 2e) with e = 1 when edge correction is on (the
 *     reference's hook/transform outputs stay padded: lib.rs:1640-1666, 1812-1818);
 *   - device-side label planes are uint32_t (colours are 1..=n_seeds < 2^32);
 *   - every function returns WS_OK (0) or a negative ws_status; nothing aborts.
 *   - a ws_ctx is single-threaded; different contexts may be used from different
 *     host threads concurrently (the reference's structs are Send + Sync: lib.rs:65-67).
 *
 * Semantics fixed by the reference and reproduced here
 *   - find_local_minima returns strict 8-neighbour local MAXIMA of the interior,
 *     in row-major order (lib.rs:1178-1197);
 *   - colours are 1..=n_seeds in slice order, later duplicates overwrite (lib.rs:1670-1677);
 *   - only interior pixels are flooded (3x3 windows, lib.rs:220-222);
 *   - levels run 0..=max_water_level inclusive (lib.rs:1689);
 *   - where lakes of different colours meet, the reference picks a random neighbour
 *     colour (lib.rs:249-253); this engine always takes the first coloured neighbour
 *     in the reference's own order down,right,left,up (lib.rs:190, 245) -- a legal
 *     outcome of the reference, and the only tie rule offered (WS_TIE_FIRST_DRLU);
 *   - SegmentingWatershed::transform as written panics (lib.rs:1821 indexes the
 *     level-0 hook result); ws_segment returns the intended result, the labels after
 *     the last level (what transform_history(..).last() yields, lib.rs:1824-1835);
 *   - merged-lake ids DIFFER IN VALUE from the reference's: there a merged lake takes region[0] of
 *     make_colour_map's closure (lib.rs:508-541), which is a function of the order of the pair list
 *     (parallel unstable sort + dedup, lib.rs:440-443) -- deterministic for a given list, but not a
 *     property of the lake.  This engine returns the canonical id: the smallest seed colour whose
 *     seed pixel lies in the lake AND still carries it after seeding (a later list entry on the same
 *     pixel overwrites an earlier one, lib.rs:1670-1677: the earlier colour exists nowhere and is
 *     nobody's id, in any entry point).  The PARTITION into lakes is the reference's (tested against the
 *     oracle's faithful closure under random tie-breaks); the id values are a documented deviation,
 *     "parity unpinned" by the reference (it has no test or fixture for them).
 */
#ifndef WS_HIP_H
#define WS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WS_ABI_VERSION 3 /* 2: ws_options grew to 8 bytes (seed_shift); 3: ws_group_* / ws_*_tiled* / ws_segment_batch* / ws_segment_minima* / ws_lists_from_arrival_device / ws_ctx_set_host_threads, WS_ERR_RCCL */

/* lib.rs:138-141 */
#define WS_UNCOLOURED 0u
#define WS_NORMAL_MAX 254u
#define WS_ALWAYS_FILL 0u
#define WS_NEVER_FILL 255u

typedef enum ws_status {
  WS_OK = 0,
  WS_ERR_BAD_ARG = -1,       /* null pointer, stride < w, ... */
  WS_ERR_MAX_TOO_HIGH = -2,  /* BuildErr::MaxToHigh, lib.rs:1026-1027 */
  WS_ERR_MAX_TOO_LOW = -3,   /* BuildErr::MaxToLow,  lib.rs:1028-1029 */
  WS_ERR_SEED_OOB = -4,      /* the reference panics: lib.rs:1366 / 1676 */
  WS_ERR_HIP = -5,           /* a HIP runtime call failed; see ws_last_error */
  WS_ERR_OOM = -6,           /* device or host allocation failed */
  WS_ERR_NO_DEVICE = -7,
  WS_ERR_CAPACITY = -8,      /* output buffer too small; *n_found still holds the true count */
  WS_ERR_RING_OVERFLOW = -9, /* a flood reached ring 2^24-1 inside one level: the last ring allowed is 2^24-2, at every level
                                (from seeds that needs a corridor of 16.7 M pixels).  The flood is refused one ring BEFORE the 24-bit
                                field would carry: out of level 254 the carry itself is 0xFF000000, "never coloured" */
  WS_ERR_TOO_LARGE = -10,    /* plane has >= 2^32 pixels or seeds */
  WS_ERR_UNSUPPORTED = -11,
  WS_ERR_RCCL = -12          /* an RCCL call failed, or librccl.so could not be loaded; see ws_group_last_error */
} ws_status;

typedef enum ws_engine {
  WS_ENGINE_AUTO = 0,
  /* all water levels fused: every pixel carries its (level, ring) arrival stamp and the
   * flood is relaxed tile-by-tile in LDS; bit-identical to the sweep */
  WS_ENGINE_FUSED = 1,
  /* literal level sweep: one synchronous 4-neighbour flood step per launch, repeated
   * until unchanged, for every level (lib.rs:1689-1748 one-to-one) */
  WS_ENGINE_SWEEP = 2
} ws_engine;

#define WS_TIE_FIRST_DRLU 0

/* The runtime options of TransformBuilder (lib.rs:908-923) as plain data. */
typedef struct ws_options {
  uint8_t max_water_level; /* lib.rs:950; valid 1..=254 */
  uint8_t edge_correction; /* lib.rs:958; 0/1.  The (h+2) x (w+2) plane of lib.rs:1640-1666 is only ever the shape of the
                              label plane: the ring of zeros around the image is virtual, no padded image copy is made. */
  uint8_t engine;          /* ws_engine */
  uint8_t tie_rule;        /* WS_TIE_FIRST_DRLU */
  uint8_t seed_shift;      /* only with edge_correction.  0 (default): seeds index the PADDED plane with the caller's
                              coordinates, i.e. land one pixel up-left of where they were found -- what the reference does
                              (lib.rs:1364-1366, 1675-1677: `output[*seed_idx]` on the padded array).  1: every seed is moved by
                              (+1, +1) onto its own pixel -- what edge correction evidently intends; not reference behaviour. */
  uint8_t reserved[3];     /* must be zero */
} ws_options;

typedef struct ws_ctx ws_ctx;

/* Counters of the last transform run on a context (the reference's `debug` PerfReport,
 * lib.rs:640-696, restated for this engine). */
typedef struct ws_stats {
  uint32_t relax_passes;      /* fused engine: global relaxation passes launched */
  uint32_t resolve_passes;    /* fused engine: global label-resolve passes launched */
  uint32_t sweep_steps;       /* sweep engine: flood steps launched */
  uint32_t merge_levels;      /* merging: levels with at least one union */
  uint64_t tiles_run_relax;   /* tiles that actually did work, summed over passes, in units of 8192 pixels (a seam band of 256 x 8 is a quarter) */
  uint64_t tiles_run_resolve;
  float ms_relax;             /* HIP-event time per kernel class; filled only when */
  float ms_resolve;           /* profiling is enabled with ws_ctx_set_profiling     */
  float ms_sweep;
  float ms_other;
  float ms_total;             /* device time of the whole call between first and last launch */
  uint32_t launches_relax;
  uint32_t launches_resolve;
  uint32_t launches_sweep;
  uint32_t relax_tile_iterations; /* k_relax2: in-tile sweeps summed over tiles and passes */
  uint32_t graph_launches;    /* 1: the call's seed tables, first passes and gated resolve ran as one hipGraph launch
                                 (a transform repeating the previous one's buffers, sizes and seed count, on a
                                 non-null stream); occupies what was tail padding: the struct size is unchanged */
} ws_stats;

/* HookCtx (lib.rs:844-862) as a C callback, invoked once per water level, in order.
 * `labels` is a host plane valid only during the call.  The seeds slice of HookCtx is
 * the caller's own seed list, so it is not passed back. */
typedef void (*ws_level_cb)(void *user, uint8_t water_level, uint8_t max_water_level,
                            const uint8_t *image, const uint64_t *labels, size_t h, size_t w);

/* One lake of one level for transform_to_list (lib.rs:628-635, 1551-1561): the dense
 * Vec<usize> of length h*w+1 per level is returned sparsely. */
typedef struct ws_lake {
  uint64_t colour;
  uint64_t area;
} ws_lake;

/* One record of the merging transform's lake hierarchy (ws_merge_tree): record c belongs to seed colour c. */
#define WS_TREE_ALIVE 0xFFFFFFFFu
typedef struct ws_tree_node {
  uint32_t parent;       /* canonical id of the lake that swallowed this one; 0 if none */
  uint32_t death_level;  /* first water level after which this colour is no lake of its own; WS_TREE_ALIVE if none */
  uint32_t area;         /* pixels of the lake while it was last its own */
  uint32_t n_leaves;     /* seed colours in the lake at that moment, itself included */
} ws_tree_node;

/* One lake of that hierarchy measured (ws_merge_tree_stats): record c belongs to seed colour c, over the pixels `area` counts.
 * v(p) is the weight of pixel p; rows and columns are those of the padded plane.  72 bytes. */
typedef struct ws_lake_stats {
  uint64_t sum_w;    /* sum of v(p) over the lake's pixels */
  uint64_t sum_wr;   /* sum of v(p) * row(p) */
  uint64_t sum_wc;   /* sum of v(p) * col(p) */
  uint64_t sum_r;    /* sum of row(p) */
  uint64_t sum_c;    /* sum of col(p) */
  uint32_t r_min, r_max, c_min, c_max; /* bounding box, inclusive */
  uint32_t w_min, w_max;               /* smallest / largest v(p) */
  uint32_t peak_pixel; /* row-major index, in the padded plane, of the FIRST pixel in row-major order with v == w_max */
  uint32_t reserved;   /* 0 */
} ws_lake_stats;

/* The second moments of one lake (ws_merge_tree_shapes): record c belongs to seed colour c, over the pixels `area` counts (M_c of
 * ws_merge_tree_stats).  Every sum is exact in 128 bits: [0] the low, [1] the high 64 bits.  96 bytes. */
typedef struct ws_lake_shape {
  uint64_t sum_wrr[2], sum_wcc[2], sum_wrc[2];   /* sum of v(p) * row^2, v(p) * col^2, v(p) * row * col */
  uint64_t sum_rr[2],  sum_cc[2],  sum_rc[2];    /* sum of row^2, col^2, row * col */
} ws_lake_shape;

/* ---- context ------------------------------------------------------------------------- */

int ws_abi_version(void);
const char *ws_strerror(int status);

/* Creates a context on HIP device `device` with its own stream. */
int ws_ctx_create(int device, ws_ctx **out);
/* Same, but all work is enqueued on the caller's hipStream_t (e.g. PyTorch's current
 * stream), so the caller's events bracket the kernels. */
int ws_ctx_create_on_stream(int device, void *hip_stream, ws_ctx **out);
void ws_ctx_destroy(ws_ctx *ctx);
const char *ws_last_error(const ws_ctx *ctx);
int ws_ctx_set_profiling(ws_ctx *ctx, int enabled);
int ws_ctx_get_stats(const ws_ctx *ctx, ws_stats *out);
int ws_ctx_synchronize(ws_ctx *ctx);
/* ws_segment_batch_device stacks at most this many pixels into one transform (the stack needs 9 bytes per pixel of
 * context workspace); larger batches run as several stacks.  0 restores the default, 2^31 - 1, which is also the cap. */
int ws_ctx_set_batch_pixel_limit(ws_ctx *ctx, size_t max_px);
/* The segmenting transform of a plane with at least this many pixels repairs the seams of its first relaxation pass with
 * bands and strips instead of a second pass over every tile (same labels either way).  0 restores the
 * default, 2^24: smaller planes are bound by launch gaps and gain nothing.  (Tests lower it to cover the path on small planes.) */
int ws_ctx_set_seam_repair_min_pixels(ws_ctx *ctx, size_t min_px);
/* Long-range floods (smooth maps: a flood crosses thousands of pixels and the relaxation needs a hundred passes and more): with
 * mode 1 or 2 the first pass of the late, same-grid regime is ONE persistent launch in which workgroups pull 128 x 64 tiles from
 * a device-side queue and a tile that changes something its neighbour must see queues that neighbour at once (stamps handed
 * over write-through / past L1 at agent scope); the pass after it looks at every tile again, so the labels are the same in
 * every mode.  1: first come, first served (a ring).  2: in flood order -- 31 buckets by the level of the smallest stamp that
 * waits at a tile's borders, the lowest non-empty bucket first, and a run that announces a tile of its own bucket takes it
 * itself; it runs on 128 x 128 tiles and starts at pass 3.  0: the ordinary passes.  3 (the default): mode 2 when the seeds
 * are sparse -- fewer than one per two tiles, so that floods cross several tiles each -- the passes otherwise.  Measured on
 * 8192^2 smooth maps of correlation length 4 / 16 / 64 / 256 px (683 k / 8.6 k / 35 / 1 seeds): 3.0 / 5.8 / 6.7 / 3.5 ms with the
 * passes, 3.0 / 6.4 / 6.4 / 4.1 with mode 1, 4.2 / 5.8 / 3.9 / 3.2 with mode 2, 3.0 / 5.8 / 3.9 / 3.2 with the default
 * (profiles/r3_v1_persistent_ab.txt).  4: the passes on their EARLY schedule (one grid from pass 3,
 * scans from pass 2), what the default picks for between one seed per two tiles and ~30 per tile (5.8 -> 5.3 ms at 16 px).
 * Transforms that converge in a few passes (random fields) never reach those passes.  WS_ERR_BAD_ARG for any other mode. */
int ws_ctx_set_persistent_pass(ws_ctx *ctx, int mode);
/* Host threads the host-buffer entry points may start for the length of a call (default 4, at most 64, never more than the
 * machine has): from 2^21 pixels on a u64 label plane (ws_segment, ws_segment_minima, ws_merge ...) crosses the bus as the device's
 * u32 plane in chunks (a quarter of the plane, 16 MiB at most) and these threads widen each chunk into the caller's memory while the next ones are in flight --
 * half the bytes over PCIe (8192^2: ws_segment_minima 11.5 -> 7.2 ms).  0: no threads, the plane is widened on the device and
 * copied whole, as before. */
int ws_ctx_set_host_threads(ws_ctx *ctx, int n_threads);
/* The merging transform_to_list of a seed list with at least this many entries writes every level's lake records from the
 * list of the lakes alive at the level before, instead of looking at every colour at every level (same records, the order
 * inside a level differs).  0 restores the default, 2^20: fewer colours are bound by launch latency and gain nothing.
 * (Tests lower it to cover the form on small planes.) */
int ws_ctx_set_live_list_min_colours(ws_ctx *ctx, size_t min_colours);

/* TransformBuilder::build_segmenting / build_merging validation (lib.rs:999-1004, 1026-1030). */
int ws_options_default(ws_options *out);          /* lib.rs:936-946: max 254, no edge correction */
int ws_options_validate(const ws_options *opt);

/* ---- host-buffer entry points (what the Rust shim binds) ---------------------------- */

/* WatershedUtils::find_local_minima (lib.rs:1178-1197).  Writes up to `cap` (row, col)
 * pairs; *n_found receives the total.  WS_ERR_CAPACITY when cap is too small. */
int ws_find_local_minima(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride,
                         uint64_t *out_rc, size_t cap, size_t *n_found);

/* Watershed::transform for SegmentingWatershed (lib.rs:1810-1822, intended semantics).
 * out_labels is the reference's Array2<usize> plane.  From 2^21 pixels on the labels cross the bus as the device's u32 plane, in
 * chunks, and host threads of the library (ws_ctx_set_host_threads: four; 0 = none, one 8-byte copy) widen them into
 * out_labels while the next chunks are in flight: 8192^2 9.2 ms instead of 13.7.  The threads live for
 * the call only. */
int ws_segment(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride,
               const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt,
               uint64_t *out_labels);

/* The same with the labels as the device holds them, uint32_t (colours are 1..=n_seeds < 2^32): one plain copy, no host
 * threads, half the bytes in the caller's memory (8192^2: 8.7 ms; the transform itself is 0.56 ms of it, the rest is the link at
 * its 53 GB/s).  For callers that can hold u32 labels; not what transform() returns. */
int ws_segment_u32(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride,
                   const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt,
                   uint32_t *out_labels);

/* The README's call pair as ONE call (lib.rs:73-86: `let mins = ws.find_local_minima(img); ws.transform(img, &mins)`):
 * the seeds are find_local_minima(img) (lib.rs:1178-1197, in its row-major order: colour i + 1 for its i-th entry) and the labels
 * are transform's for that list.  The list never has to exist: with the fused engine, no edge correction and w % 32 == 0 the
 * seed tables come out of the minima kernels themselves; otherwise the two calls run one after the other.  seeds_rc (cap
 * pairs, may be NULL with cap 0) receives the list when the caller wants it; *n_seeds its length.  WS_ERR_CAPACITY when
 * cap > 0 is too small -- the labels are complete then, the list is cut.  8192^2 host form: 117 MB of seed pairs less each
 * way over PCIe than ws_find_local_minima + ws_segment. */
int ws_segment_minima(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const ws_options *opt,
                      uint64_t *out_labels, uint64_t *seeds_rc, size_t cap, size_t *n_seeds);
int ws_segment_minima_u32(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const ws_options *opt,
                          uint32_t *out_labels, uint64_t *seeds_rc, size_t cap, size_t *n_seeds);
/* ... on device-resident buffers: d_labels h x w (padded with edge correction) uint32_t, d_seeds_rc cap (row, col) uint32_t
 * pairs or NULL. */
int ws_segment_minima_device(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride, const ws_options *opt,
                             uint32_t *d_labels, uint32_t *d_seeds_rc, size_t cap, size_t *n_seeds);

/* Watershed::transform_with_hook for SegmentingWatershed (lib.rs:1638-1808): cb is called
 * after every level 0..=max with the label plane of that level; transform_history
 * (lib.rs:1824-1835) is this with a copying callback.  out_labels may be NULL. */
int ws_segment_with_hook(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride,
                         const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt,
                         ws_level_cb cb, void *user, uint64_t *out_labels);

/* Watershed::transform_with_hook for MergingWatershed (lib.rs:1328-1522).  Labels passed
 * to cb / written to out_labels carry canonical representatives (see top of file). */
int ws_merge_with_hook(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride,
                       const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt,
                       ws_level_cb cb, void *user, uint64_t *out_labels);

/* Watershed::transform_to_list (lib.rs:1551-1561 merging, 1837-1847 segmenting), sparse:
 * for level l the lakes with area > 0 are lakes[offsets[l] .. offsets[l+1]), every lake
 * once, as runs of increasing colours in no particular order of the runs (the reference's
 * vector is indexed by colour, so a caller scatters them: hist[colour] = area); the
 * uncoloured count (index 0 of the reference's vector) is uncoloured[l].
 * offsets has max_water_level+2 entries, uncoloured max_water_level+1.
 * *n_lakes receives the total number of records; WS_ERR_CAPACITY if cap is too small. */
int ws_transform_to_list(ws_ctx *ctx, int merging, const uint8_t *img, size_t h, size_t w,
                         size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                         const ws_options *opt, ws_lake *lakes, size_t cap, size_t *n_lakes,
                         uint64_t *offsets, uint64_t *uncoloured);

/* MergingWatershed::transform is a stub in the reference (lib.rs:1524-1536): zeros with the
 * interior set to 123, seeds ignored.  Reproduced for drop-in completeness. */
int ws_merge_transform_stub(size_t h, size_t w, uint64_t *out_labels);

/* A cube of n_slices independent h x w slices in HOST memory -- tests/integration.rs:267,356: the reference calls
 * find_local_minima + transform for one slice of a CGPS cube after the other.  Slice k starts at cube + k * slice_stride; its
 * seeds are seeds_rc[2 * seed_offsets[k] .. 2 * seed_offsets[k + 1]) (seed_offsets: n_slices + 1 entries), or, with seeds_rc ==
 * NULL, its own find_local_minima (lib.rs:1178-1197; n_seeds[k], nullable, receives how many); its labels go to out_labels +
 * k * (padded plane).  Equivalent to n_slices calls of ws_segment (ws_segment_minima) and bit-identical to them; the slices take
 * turns on four internal contexts with a stream each and a host thread each for the length of the call, so that one slice's
 * upload, another's transform and a third's label copy overlap on the two directions of the link: 16 x 4096^2 in 23 ms against
 * 34 ms for the loop (1.44 ms a slice; its labels alone take the link 1.17).  The context's statistics (ws_ctx_get_stats) and last
 * arrival stamps are not those of any slice afterwards.  On an error the lowest failing slice is reported in *failed_slice (nullable), its message through ws_last_error. */
int ws_segment_batch(ws_ctx *ctx, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                     size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                     uint64_t *out_labels, size_t *n_seeds, size_t *failed_slice);

/* ws_transform_to_list_batch_device from HOST memory: the cube and the (row, col) seed pairs as ws_segment_batch takes them
 * (seeds_rc == NULL: every slice's own find_local_minima, n_seeds[k], nullable, receives how many), the records into the host's
 * `lakes` (cap of them; the same transfer as ws_transform_to_list).  Offsets, uncoloured, WS_ERR_CAPACITY and *failed_slice as the
 * device form.  Context workspace: the cube, the seeds and cap records on the device besides the device form's. */
int ws_transform_to_list_batch(ws_ctx *ctx, int merging, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                               size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                               ws_lake *lakes, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured, size_t *n_seeds,
                               size_t *failed_slice);

/* ---- device-resident entry points (inputs and outputs stay in HBM) ------------------- */

/* d_img: device u8 plane; d_seeds_rc: device (row, col) pairs as uint32_t[2];
 * d_labels: device uint32_t plane of the (padded, if edge correction) shape.
 * Any seed list is accepted (duplicates: the later entry wins, lib.rs:1672-1677).  A list in strictly
 * increasing row-major order -- what ws_find_local_minima(_device) returns -- takes a faster path; the
 * engine checks the order on the device, nothing has to be declared. */
int ws_find_local_minima_device(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w,
                                size_t row_stride, uint32_t *d_out_rc, size_t cap,
                                size_t *n_found);
int ws_segment_device(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                      const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt,
                      uint32_t *d_labels);
/* ws_segment_device in two halves, for pipelines: _begin queues the transform and returns, _end waits for it and
 * returns its status.  Between the two the context belongs to that transform (no other call on it) and the caller's
 * buffers must stay as they are.  Only a transform that repeats the previous call's arguments on this context (same
 * buffers, sizes and seed count: its launches are replayed as one graph) is actually left in flight; any other runs
 * whole inside _begin.  Contexts taking turns keep the GPU's queue from running dry between transforms (created on one
 * stream: 8192^2 0.55 -> 0.53 ms per transform), and on streams of their own their transforms overlap on the GPU, one
 * filling the CUs another leaves idle (four contexts: 0.45 ms per transform; a single transform still takes 0.55). */
int ws_segment_device_begin(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                            const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt,
                            uint32_t *d_labels);
int ws_segment_device_end(ws_ctx *ctx);
/* A stack of independent slices (BASELINE config C4: a cube cut into 2-D slices, as the reference's own
 * integration tests do, tests/integration.rs:267,356): slice k starts at d_cube + k * slice_stride, its
 * seeds are d_seeds_rc[2 * seed_offsets[k] .. 2 * seed_offsets[k+1]) (seed_offsets: n_slices + 1 entries, on
 * the HOST), its labels go to d_labels + k * (padded plane).  Equivalent to n_slices calls of
 * ws_segment_device; stops at the first slice that fails and reports its index in *failed_slice.
 * Contiguous slices (slice_stride == h * row_stride, row_stride == w unless edge correction copies them anyway) with
 * strictly increasing seed lists, w' % 4 == 0 and h' * w' % 128 == 0 (h', w': the padded plane) run as ONE transform
 * over the stacked slices -- the border rows of a slice never flood, so they wall the slices off from each other --
 * instead of n_slices transforms: 16 x 1024^2 in 0.28 ms instead of 2.2 ms.  Results are identical either way.
 * After a stacked batch ws_last_arrival_device reports "unsupported" (the stamps are those of the stack). */
int ws_segment_batch_device(ws_ctx *ctx, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w,
                            size_t row_stride, size_t slice_stride, const uint32_t *d_seeds_rc,
                            const size_t *seed_offsets, const ws_options *opt, uint32_t *d_labels,
                            size_t *failed_slice);
/* Merging transform, final canonical labels only. */
int ws_merge_device(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                    const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt,
                    uint32_t *d_labels);
/* ... in two halves, as ws_segment_device_begin / _end (same rules). */
int ws_merge_device_begin(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                          const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt,
                          uint32_t *d_labels);
int ws_merge_device_end(ws_ctx *ctx);
/* Watershed::transform_to_list with everything in HBM: the image, the u32 seed pairs and the lake RECORDS (d_lakes: cap
 * records in the caller's device buffer; at 1024^2 they are 155 MB that the host form spends most of its time copying).
 * Only the per-level offsets (max_water_level + 2) and uncoloured counts (max_water_level + 1) go to the host arrays.
 * Same record layout, order and WS_ERR_CAPACITY protocol as ws_transform_to_list. */
int ws_transform_to_list_device(ws_ctx *ctx, int merging, const uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                                const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt, ws_lake *d_lakes,
                                size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured);

/* The same lists from a segmenting transform that has already run -- here or on other devices: d_keys = its arrival stamps
 * (ws_last_arrival_device / ws_copy_last_arrival_device), d_seg_labels = its labels, both h x w u32 planes as they stand (a
 * padded plane is passed padded; opt->edge_correction is ignored), n_seeds = the number of colours.  Everything the per-level
 * paths read is in those two planes: no image, no seed list, no second flood.  Records, offsets, uncoloured and
 * WS_ERR_CAPACITY as ws_transform_to_list_device. */
int ws_lists_from_arrival_device(ws_ctx *ctx, int merging, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w,
                                 size_t n_seeds, const ws_options *opt, ws_lake *d_lakes, size_t cap, size_t *n_lakes,
                                 uint64_t *offsets, uint64_t *uncoloured);
/* transform_to_list of every slice of a cube (tests/integration.rs:122-601: find_local_minima and transform_to_list on one
 * slice after the other), merging (merging != 0) or segmenting, everything in HBM.  Slices, seeds, seed_offsets (n_slices + 1
 * entries, on the HOST) and *failed_slice as ws_segment_batch_device; L = opt->max_water_level.
 * Layout, slice-major then level: the records of slice k at level l are d_lakes[offsets[k * (L + 1) + l] .. offsets[k * (L + 1) + l + 1])
 * (offsets: n_slices * (L + 1) + 1 entries on the host), in the slice's own colours 1 .. n_k; uncoloured[k * (L + 1) + l] (n_slices *
 * (L + 1) entries on the host) is index 0 of the reference's vector for that slice and level.  Every (slice, level) holds the same
 * records as ws_transform_to_list_device on that slice, in no particular order.  *n_lakes receives the total; WS_ERR_CAPACITY when
 * cap is too small (then only *n_lakes is meaningful: call again with that many).
 * When the slices stack (the conditions of ws_segment_batch_device, and a seed in every group of slices) the whole cube runs as one
 * flood and ONE set of per-level launches over the stack, whose records are then split into the layout above; anything else runs
 * as a loop of ws_transform_to_list_device.  Scratch of the stacked form, kept by the context: 4 B per pixel of the stack (its
 * labels), 16 B per record of cap (the stack's records before the split), and 8 B per (slice, level) bin.  Statistics are summed
 * over the call's transforms; afterwards ws_last_arrival_device reports "unsupported". */
int ws_transform_to_list_batch_device(ws_ctx *ctx, int merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w,
                                      size_t row_stride, size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets,
                                      const ws_options *opt, ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets,
                                      uint64_t *uncoloured, size_t *failed_slice);
/* The merging transform's final canonical labels of every slice of a cube: arguments as ws_segment_batch_device, labels as
 * ws_merge_device on each slice, bit for bit (the smallest seed colour of the lake, in the slice's own colours).  Slices that stack
 * run as one flood and one union pass over the stack; the rest as a loop of ws_merge_device.  Scratch: the union-find of all the
 * stack's colours (16 B a colour). */
int ws_merge_batch_device(ws_ctx *ctx, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                          size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                          uint32_t *d_labels, size_t *failed_slice);
/* Arrival stamps of the last ws_segment_device / ws_merge_device call on this context:
 * (level << 24 | ring), 0 for seeds, 0xFF000000 for never coloured.  Device pointer owned
 * by the context, valid until the next call; shape as the label plane. */
int ws_last_arrival_device(ws_ctx *ctx, const uint32_t **d_keys, size_t *h, size_t *w);
/* Copies those stamps into the caller's device buffer of n_elems >= h*w words (stream ordered). */
int ws_copy_last_arrival_device(ws_ctx *ctx, uint32_t *d_dst, size_t n_elems);
/* transform_history on the device, one level at a time (lib.rs:1824-1835 without the 255 host copies): the SEGMENTING
 * label plane as the reference's hook sees it after `water_level` (lib.rs:1796-1804) -- a pixel carries its final colour
 * once its arrival level is <= water_level, 0 before -- from d_labels (what the last ws_segment_device on this context
 * wrote) and the context's arrival stamps; d_out is a plane of the same shape (may equal d_labels).  Stream ordered. */
int ws_level_snapshot_device(ws_ctx *ctx, const uint32_t *d_labels, uint8_t water_level, uint32_t *d_out);
/* transform_history (lib.rs:1233-1237; merging 1538-1549, segmenting 1824-1835) for a caller-chosen list of water levels, in
 * one transform and with the planes left in HBM: plane k -- the label plane the reference's hook sees after water level
 * levels[k] -- goes to d_out + k * plane_stride (u32 words, plane_stride >= the padded h * w; the fast path, 16-byte stores,
 * needs plane_stride % 4 == 0 and d_out 16-byte aligned -- otherwise every pixel is stored on its own).  levels: n_levels host bytes,
 * each <= opt->max_water_level, in any order, repeats allowed; 1 <= n_levels <= 256, or 0: nothing runs, nothing is written.
 * merging != 0: the merging transform, whose planes carry canonical ids (the smallest seed colour of the lake, as
 * ws_merge_with_hook delivers them); 0: the segmenting one (ws_level_snapshot_device's planes).  Image, seeds, edge correction
 * and duplicate seeds as ws_segment_device / ws_merge_device; the flood is the fused one whatever opt->engine says.  A level
 * above max_water_level or a short plane_stride (also with n_levels == 0) is WS_ERR_BAD_ARG before anything runs.  Afterwards ws_last_arrival_device
 * reports this transform's stamps.  The merging transform keeps a level-stamped merge forest while its per-level unions run
 * (8 B per colour of context workspace), then ONE pass over the plane writes every requested level. */
int ws_transform_history_device(ws_ctx *ctx, int merging, const uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                                const uint32_t *d_seeds_rc, size_t n_seeds, const ws_options *opt,
                                const uint8_t *levels, size_t n_levels, uint32_t *d_out, size_t plane_stride);
/* The same from and into HOST memory: u64 planes (usize, as the reference's), n_levels * padded h * w words, contiguous, plane
 * k for levels[k].  Scratch, kept by the context: the planes are rendered in chunks of at most 256 MiB of u32 words on the
 * device (at least one plane); a chunk of 2^21 words and more crosses the bus as u32, widened by the host threads
 * (ws_ctx_set_host_threads), smaller ones plane by plane. */
int ws_transform_history(ws_ctx *ctx, int merging, const uint8_t *img, size_t h, size_t w, size_t row_stride,
                         const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt,
                         const uint8_t *levels, size_t n_levels, uint64_t *out);
/* The merging transform's lake hierarchy -- which lake swallowed which, after what water level, and how big each was -- as one
 * record per seed colour, from one flood and one run of the stamping per-level unions of ws_transform_history_device(merging);
 * no plane is written.  d_tree: n_seeds + 1 records in HBM, record c for colour c (the c-th seed, from 1).  With P_L the
 * canonical merging plane after level L (ws_transform_history_device's) and "c exists" meaning that c's seed pixel carries c
 * right after seeding (a later seed on the same pixel overwrites, lib.rs:1670-1677):
 *   death_level  the first L in 0 ..= max_water_level with P_L[seed pixel of c] != c, WS_TREE_ALIVE if there is none;
 *   parent       that value, the canonical id (smallest seed colour) of the lake c went into: 0 < parent < c, and the parent
 *                dies strictly later or never; 0 if c never died;
 *   area         pixels equal to c in P_(death_level - 1) (in P_max if c never died; 1 if death_level == 0: the seed alone);
 *   n_leaves     existing colours whose seed pixel shows c in that plane (1 if death_level == 0).
 * A colour that does not exist is (0, WS_TREE_ALIVE, 0, 0); record 0 is (0, WS_TREE_ALIVE, pixels of the padded plane still
 * uncoloured after the last level, 0).  Following `parent` from c while death_level <= L gives P_L at c's seed pixel, so with
 * the segmenting labels the plane of any level is a table lookup.  d_labels (nullable): receives those labels, the padded h * w
 * plane of u32 the tree's colours refer to.  Image, strides, seeds, edge correction, seed_shift and duplicate seeds as
 * ws_merge_device; n_seeds == 0 writes record 0 only.  Null pointers with non-zero sizes, bad options and a context that holds
 * a begun transform are refused before anything runs.  Returns with the records complete; afterwards ws_last_arrival_device
 * reports this transform's stamps.  Workspace kept by the context: the merge forest (8 B a colour, as transform_history), the
 * unions' buckets (at most 20 B a pixel, as transform_to_list), 4 B a colour for the colours ordered by death level and 6 KB of
 * counters; the records themselves are the accumulators. */
int ws_merge_tree_device(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride, const uint32_t *d_seeds_rc,
                         size_t n_seeds, const ws_options *opt, ws_tree_node *d_tree, uint32_t *d_labels);
/* The same from and into HOST memory: u64 (row, col) seed pairs, the records into `tree` (n_seeds + 1), the segmenting labels
 * (nullable) as a u64 plane of the padded shape.  Keeps 16 B a colour more on the device (the records before they cross). */
int ws_merge_tree(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                  const ws_options *opt, ws_tree_node *tree, uint64_t *labels);
/* ws_merge_tree_device and a catalogue of its lakes from the same flood: d_tree receives exactly what ws_merge_tree_device writes,
 * d_stats n_seeds + 1 records, record c for colour c.  For an existing colour c let M_c be the pixels equal to c in
 * P_(death_level - 1) (P_max if c never died; the seed pixel alone if death_level == 0): the set whose size is `area`.  Record c
 * holds the sums, the extrema and the box of M_c; record 0 those of the pixels still uncoloured after the last level.  row and col
 * are coordinates of the padded plane (shifted by one under edge correction).  v(p) comes from the weight plane: h x w elements,
 * unpadded, weight_row_stride ELEMENTS a row, weight_dtype WS_U8 or WS_U16 (anything else: WS_ERR_UNSUPPORTED); under edge
 * correction weight pixel (r, x) sits at padded (r + 1, x + 1) and the ring weighs 0.  d_weight == NULL: the image itself as u8
 * (dtype and stride are ignored).  A colour that does not exist, and record 0 when nothing is uncoloured, get the identity of the
 * fold: every sum 0, r_min = c_min = w_min = peak_pixel = 0xFFFFFFFF, r_max = c_max = w_max = 0; reserved is always 0.
 * n_seeds == 0 writes record 0 of both arrays only.  Null pointers with non-zero sizes, bad options, a short image or weight
 * stride and a context that holds a begun transform are refused before anything runs and leave the outputs untouched, and so is
 * (WS_ERR_TOO_LARGE) a plane for which wmax(dtype) * pixels * max(padded h, padded w) does not fit in 64 bits.  Everything is
 * integer and every record reproducible to the bit; float data is quantised by the caller (ws_pre_processor).  d_labels
 * (nullable) as ws_merge_tree_device.  Workspace kept by the context on top of ws_merge_tree_device's: 68 B a colour. */
int ws_merge_tree_stats_device(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride, const uint32_t *d_seeds_rc,
                               size_t n_seeds, const ws_options *opt, const void *d_weight, int weight_dtype,
                               size_t weight_row_stride, ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *d_labels);
/* The same from and into HOST memory, as ws_merge_tree: the weight plane is uploaded (contiguous, on the context) and the records
 * come back into `tree` and `stats` (n_seeds + 1 each).  Keeps 88 B a colour more on the device and the weight plane. */
int ws_merge_tree_stats(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc,
                        size_t n_seeds, const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride,
                        ws_tree_node *tree, ws_lake_stats *stats, uint64_t *labels);
/* The same tree, and with d_stats != NULL the same catalogue, from a segmenting transform that has already run -- here or on other
 * devices -- without a second flood: d_keys and d_seg_labels as ws_lists_from_arrival_device (h x w u32 planes as they stand, a
 * padded plane passed padded; opt->edge_correction is ignored, only max_water_level is read), n_seeds = the number of colours.
 * No seed list comes in: seeds are coloured before level 0 and nothing else is (lib.rs:1675-1677), so stamp 0 marks the seed
 * pixels and the label there is the colour that survived seeding (lib.rs:1670-1677); a colour without a stamp-0 pixel does not
 * exist.  d_tree: n_seeds + 1 records, bit-identical to ws_merge_tree_device's for the transform that produced the planes.
 * d_stats == NULL: the tree alone, the weight arguments are ignored.  d_stats != NULL: n_seeds + 1 records, bit-identical to
 * ws_merge_tree_stats_device's; d_weight is an h x w plane of the shape passed, no offset, WS_U8 or WS_U16 (anything else:
 * WS_ERR_UNSUPPORTED), weight_row_stride elements a row -- this form has no image, so d_weight == NULL is WS_ERR_BAD_ARG; a
 * plane too large for 64-bit moments is WS_ERR_TOO_LARGE as there.  n_seeds == 0 or h * w == 0 writes record 0 only.  Null
 * planes with a non-zero size, bad options and a context that holds a begun transform are refused before anything runs and
 * leave the outputs untouched.  The planes stay the caller's (they may be views off 16-byte alignment: scalar loads then), and
 * ws_last_arrival_device keeps reporting what it reported before.  Workspace as ws_merge_tree(_stats)_device's without the
 * flood's, plus 8 B a colour for the recovered seed pixels. */
int ws_merge_tree_from_arrival_device(ws_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w,
                                      size_t n_seeds, const ws_options *opt, const void *d_weight, int weight_dtype,
                                      size_t weight_row_stride, ws_tree_node *d_tree, ws_lake_stats *d_stats);
/* ws_merge_tree_stats_device and the second moments of every lake from the same flood -- how big and how elongated a lake is and
 * which way it points: d_tree and d_stats receive, byte for byte, what ws_merge_tree_stats_device writes for the same arguments,
 * d_shapes (device, 8-byte aligned, else WS_ERR_BAD_ARG) n_seeds + 1 records, record c for colour c.  All three arrays are
 * required; d_labels is nullable.  Record c holds the six sums over exactly the set M_c of the first-moment record (the pixels
 * equal to c in P_(death_level - 1), in P_max if c never died, the seed pixel alone if death_level == 0), record 0 over the pixels
 * still uncoloured after the last level; rows and columns are those of the padded plane and v(p) is ws_merge_tree_stats_device's
 * (the u8 or u16 weight plane, NULL for the image itself, the ring weighs 0 under edge correction).  A colour that does not exist,
 * and record 0 when nothing is uncoloured, get the identity: all twelve words 0.  n_seeds == 0 writes record 0 of all three arrays
 * only.  Every refusal of ws_merge_tree_stats_device holds, in the same order, and leaves all three outputs untouched.  There is
 * no further WS_ERR_TOO_LARGE: the stats call already refuses a plane unless wmax * pixels * max(ph, pw) < 2^64 with ph, pw <
 * 2^32, and a sum of v * row^2 is at most wmax * pixels * max(ph, pw)^2 < 2^64 * 2^32 = 2^96 -- so are the other five.  Every sum
 * is an exact integer, accumulated as two 64-bit limbs that never exchange a carry (the terms' low 32 bits: below 2^64 for fewer
 * than 2^32 pixels; the terms >> 32: below 2^64 because the sum is below 2^96), so every record is reproducible to the bit
 * (DESIGN.md section 4.3.2).  Stream ordered; returns with the records complete; afterwards ws_last_arrival_device behaves as
 * after ws_merge_tree_stats_device.  Workspace kept by the context on top of ws_merge_tree_stats_device's: 96 B a colour, all of
 * it reserved before the transform.  Cubes: ws_merge_tree_shapes_batch(_device); tiled groups and the regions of a cut have no such
 * call yet. */
int ws_merge_tree_shapes_device(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride, const uint32_t *d_seeds_rc,
                                size_t n_seeds, const ws_options *opt, const void *d_weight, int weight_dtype,
                                size_t weight_row_stride, ws_tree_node *d_tree, ws_lake_stats *d_stats, ws_lake_shape *d_shapes,
                                uint32_t *d_labels);
/* The same from and into HOST memory, as ws_merge_tree_stats: u64 seed pairs, u64 labels, the records into `tree`, `stats` and
 * `shapes` (n_seeds + 1 each).  Keeps 96 B a colour more on the device (the records before they cross). */
int ws_merge_tree_shapes(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc,
                         size_t n_seeds, const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride,
                         ws_tree_node *tree, ws_lake_stats *stats, ws_lake_shape *shapes, uint64_t *labels);
/* The same from a segmenting transform that has already run: the planes, weights and refusals of
 * ws_merge_tree_from_arrival_device with d_stats != NULL (d_weight == NULL is WS_ERR_BAD_ARG), d_tree and d_stats byte for byte
 * what that call writes, d_shapes as ws_merge_tree_shapes_device's for the transform that produced the planes.  All three arrays
 * are required.  n_seeds == 0 writes record 0 only; h * w == 0 writes the identity.  ws_last_arrival_device keeps reporting what
 * it reported before. */
int ws_merge_tree_shapes_from_arrival_device(ws_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w,
                                             size_t n_seeds, const ws_options *opt, const void *d_weight, int weight_dtype,
                                             size_t weight_row_stride, ws_tree_node *d_tree, ws_lake_stats *d_stats,
                                             ws_lake_shape *d_shapes);
/* One cut of a merge tree (ws_tree_cut_device).  12 bytes. */
typedef struct ws_tree_cut {
  uint32_t min_area;    /* a lake that was swallowed counts only if it had reached this many pixels ... */
  uint32_t min_leaves;  /* ... and held this many seed colours; lakes that never died always count */
  uint8_t show_level;   /* pixels that arrive after this water level are 0; <= 254 */
  uint8_t merge_level;  /* every merge up to this water level is applied; <= 254 */
  uint8_t reserved[2];  /* must be zero */
} ws_tree_cut;
/* Label planes and lake lists of a merge tree pruned by lake size, number of leaves and level, from a tree the caller holds in HBM
 * and the two planes of the flood it came from -- no image, no second run of the level loop.  d_tree: n_seeds + 1 records as
 * ws_merge_tree*_device writes them; d_keys: the arrival stamps (level << 24 | ring, 0xFF000000 never coloured); d_seg_labels: the
 * segmenting labels; both h x w u32 planes taken as they stand (a padded plane is passed padded, as ws_lists_from_arrival_device;
 * views off 16-byte alignment fall back to scalar loads).  Node a is KEPT by a cut iff death_level[a] == WS_TREE_ALIVE or
 * (area[a] >= min_area and n_leaves[a] >= min_leaves).  For pixel p with c = d_seg_labels[p] and t = d_keys[p] >> 24:
 *   out[p] = 0 if c == 0 or t > show_level; otherwise the first a on the chain c, parent[c], parent[parent[c]], ... that is kept
 *   and has death_level[a] > max(t, merge_level) (an alive node has).
 * min_area = min_leaves = 0 and show_level = merge_level = L is the merging history plane of level L (ws_transform_history_device);
 * show_level = 254, merge_level = 0, min_area = A sends every pixel to the smallest lake it ever belonged to that reached A pixels
 * before it was swallowed.  The regions of a cut need not be connected.
 * cuts: 1 <= n_cuts <= 32 on the HOST, in any order, repeats allowed; n_cuts == 0 runs nothing and writes nothing.  Plane k goes to
 * d_out + k * plane_stride (plane_stride >= h * w; 16-byte stores when d_out is 16-byte aligned and plane_stride % 4 == 0,
 * otherwise every pixel is stored on its own); d_out == NULL: lists only.  d_lakes != NULL: the records d_lakes[offsets[k] ..
 * offsets[k + 1]) are (colour a, pixels with out_k == a) for every a != 0 with pixels, in INCREASING colour; hidden[k] = pixels
 * with out_k == 0; offsets (n_cuts + 1) and hidden (n_cuts) on the host; *n_lakes and WS_ERR_CAPACITY as
 * ws_transform_to_list_device (on overflow only *n_lakes is meaningful).  d_lakes == NULL with d_out != NULL: planes only, and
 * n_lakes, offsets and hidden may be NULL.
 * Refused with WS_ERR_BAD_ARG before any walk runs, outputs untouched: null pointers with non-zero sizes, both outputs NULL, a
 * level above 254, non-zero reserved, more than 32 cuts, a short plane_stride, d_out equal to d_keys or d_seg_labels, a context
 * that holds a begun transform, and a tree that is no merge tree -- one pass over the records (it reads no index above n_seeds)
 * wants of every record either death_level == WS_TREE_ALIVE and parent == 0, or death_level <= 254, 0 < parent < c and
 * death_level[parent] > death_level[c]; the host reads its verdict before anything else is launched.  A label above n_seeds is
 * compared before it indexes anything, written as 0, and the call returns WS_ERR_BAD_ARG with the outputs unspecified.
 * WS_ERR_TOO_LARGE: a plane of 2^32 pixels or more, and, with lists, n_cuts * (n_seeds + 1) >= 2^32 (the counters are indexed in 32 bits).
 * n_seeds == 0 or h * w == 0: the planes are zero, the lists empty, hidden = h * w.  Stream ordered; returns with the host
 * arrays complete.  ws_last_arrival_device keeps reporting what it reported before.  Workspace kept by the context: 4 B per
 * colour per cut (the tables), 4 B per colour per cut with lists (the counters, and 12 B per 1024 of them), and four flag words
 * (DESIGN.md section 4.4). */
int ws_tree_cut_device(ws_ctx *ctx, const ws_tree_node *d_tree, size_t n_seeds, const uint32_t *d_keys, const uint32_t *d_seg_labels,
                       size_t h, size_t w, const ws_tree_cut *cuts, size_t n_cuts, uint32_t *d_out, size_t plane_stride,
                       ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden);
/* The whole route from and into HOST memory (the host ws_merge_tree hands back no stamps): upload, ws_merge_tree, ws_tree_cut_device
 * on its labels and stamps, download.  Image, seeds, edge correction, seed_shift and duplicate seeds as ws_merge_tree; tree
 * (nullable): the n_seeds + 1 records; out (nullable): n_cuts contiguous u64 planes of the padded shape; lakes (nullable: planes
 * only), cap, n_lakes, offsets, hidden as above, in host memory.  Keeps the planes as u32 (4 B per pixel and cut) and cap records
 * on the device. */
int ws_merge_tree_cut(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                      const ws_options *opt, const ws_tree_cut *cuts, size_t n_cuts, ws_tree_node *tree, uint64_t *out, ws_lake *lakes,
                      size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden);
/* One cut of a merge tree by catalogue quantities as well (ws_tree_cut_stats_device).  32 bytes. */
typedef struct ws_lake_cut {
  uint64_t min_sum_w;   /* a lake that was swallowed counts only if its weights summed to this much (ws_lake_stats.sum_w) ... */
  uint32_t min_area;    /* ... it had reached this many pixels ... */
  uint32_t min_leaves;  /* ... held this many seed colours ... */
  uint32_t min_w_max;   /* ... its largest weight was at least this (ws_lake_stats.w_max) ... */
  uint32_t min_depth;   /* ... and it died this far above its smallest weight (below); lakes that never died always count */
  uint8_t show_level;   /* as ws_tree_cut */
  uint8_t merge_level;  /* as ws_tree_cut */
  uint8_t reserved[6];  /* must be zero */
} ws_lake_cut;
/* ws_tree_cut_device with three more thresholds, on the lake catalogue of the same flood: d_stats is n_seeds + 1 records as
 * ws_merge_tree_stats*_device (or ws_merge_tree_from_arrival_device) writes them, in HBM, 8-byte aligned.  For node a with tree
 * record t and catalogue record s let depth(a) = t.death_level - s.w_min if t.death_level != WS_TREE_ALIVE and t.death_level >
 * s.w_min, else 0 -- with the image as the weight plane, the basin's depth below its spill level.  Node a is KEPT iff it is alive,
 * or area >= min_area and n_leaves >= min_leaves and s.sum_w >= min_sum_w (a 64-bit compare) and s.w_max >= min_w_max and
 * depth(a) >= min_depth.  The plane of a cut is DEFINED as table, then walk: T[c] = the first kept node on the chain c, parent[c],
 * ...; a pixel with c = d_seg_labels[p] != 0 and t = d_keys[p] >> 24 <= show_level starts at T[c] and goes up while death_level
 * <= max(t, merge_level); it is 0 if c == 0 or t > show_level.  For the catalogue of the tree's own flood every one of the five
 * quantities is monotone up the chain (a parent's pixels contain the child's, and it dies later), so the plane is also "the first
 * node that is kept and dies after max(t, merge_level)", as ws_tree_cut_device states it.  A catalogue that belongs to ANOTHER flood
 * is not detected and is not unsafe: the check of the tree bounds every walk whatever d_stats holds, and the planes are then what
 * table-then-walk gives on those numbers.
 * Everything else is ws_tree_cut_device's: the cuts (1 .. 32 on the host, any order, repeats allowed), the planes, the lists,
 * hidden, capacity, the refusals with the outputs untouched, the check of the tree with its verdict read on the host before
 * anything walks, the late report of a label above n_seeds, WS_ERR_TOO_LARGE, the empty cases and the refusal of a context that
 * holds a begun transform.  On top: non-zero reserved bytes, and a cut with a non-zero min_sum_w, min_w_max or min_depth while
 * d_stats == NULL, are WS_ERR_BAD_ARG before anything runs.  d_stats may be NULL when no cut has such a threshold; d_stats is
 * then never read, and the call launches exactly what ws_tree_cut_device launches for the same cuts.  One table per distinct
 * five thresholds.  Workspace on top of ws_tree_cut_device's, only when two or more tables of the call have a catalogue threshold:
 * 16 B a colour, what the keep test reads of a record (sum_w, w_max, depth) packed by one pass over d_stats; a single such
 * table reads d_stats itself. */
int ws_tree_cut_stats_device(ws_ctx *ctx, const ws_tree_node *d_tree, const ws_lake_stats *d_stats, size_t n_seeds, const uint32_t *d_keys,
                             const uint32_t *d_seg_labels, size_t h, size_t w, const ws_lake_cut *cuts, size_t n_cuts, uint32_t *d_out,
                             size_t plane_stride, ws_lake *d_lakes, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden);
/* The whole route from and into HOST memory, as ws_merge_tree_cut with ws_merge_tree_stats in the place of ws_merge_tree: image,
 * seeds and options as there, the weight plane as ws_merge_tree_stats (NULL: the image itself); tree and stats (both nullable):
 * the n_seeds + 1 records each; out, lakes, cap, n_lakes, offsets, hidden as ws_merge_tree_cut.  The catalogue always runs, whatever
 * the thresholds.  Keeps on the device what both of those calls keep. */
int ws_merge_tree_stats_cut(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc, size_t n_seeds,
                            const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride, const ws_lake_cut *cuts,
                            size_t n_cuts, ws_tree_node *tree, ws_lake_stats *stats, uint64_t *out, ws_lake *lakes, size_t cap,
                            size_t *n_lakes, uint64_t *offsets, uint64_t *hidden);
/* ws_tree_cut_stats_device, and the regions its cuts show MEASURED in the same call: the source list of a cut, not only its label
 * plane.  Everything ws_tree_cut_stats_device takes and does stays as it is -- the cuts, the planes, the lists in increasing colour,
 * hidden, the capacity rule, the check of the tree before anything walks, the late report of a label above n_seeds, every refusal
 * with its outputs untouched, d_stats nullable when no cut has a catalogue threshold.  On top:
 *   d_region_stats[i] (device, 8-byte aligned, cap records next to d_lakes) is the ws_lake_stats of the pixels d_lakes[i] counts: the
 *   region {p : out_k(p) == d_lakes[i].colour} of the cut k whose range offsets[k] .. offsets[k + 1] holds i.  Field meanings and
 *   the coordinates are those of ws_merge_tree_stats_device, over the plane as it is passed; peak_pixel is the FIRST pixel in
 *   row-major order with v == w_max; reserved is 0; the region's pixel count is d_lakes[i].area.
 *   hidden_stats[k] (HOST, n_cuts records) is the same fold over the pixels with out_k == 0, the identity of the fold (as
 *   ws_merge_tree_stats_device states it) when there are none.
 * This is NOT a row of the catalogue d_stats: record c there measures M_c, the lake as it was when it died, while a region depends
 * on every pixel's arrival level, on show_level and merge_level and on which descendants the cut keeps as regions of their own.
 * The two coincide only for zero thresholds, show_level = merge_level = L and a node that dies at L + 1 (or never, at L = max).
 * d_weight: an h x w plane of the shape passed, no offset, weight_row_stride ELEMENTS a row, WS_U8 or WS_U16 (anything else:
 * WS_ERR_UNSUPPORTED), as ws_merge_tree_from_arrival_device; NULL is WS_ERR_BAD_ARG (there is no image), a short stride too, and a
 * plane too large for 64-bit moments is WS_ERR_TOO_LARGE by the same division.  d_region_stats and hidden_stats are both nullable:
 * d_region_stats != NULL needs d_lakes (else WS_ERR_BAD_ARG before anything runs); with BOTH NULL the weight arguments are not
 * looked at and the call is ws_tree_cut_stats_device, launch for launch.  On WS_ERR_CAPACITY only *n_lakes is meaningful and no
 * measuring kernel has run: d_region_stats is untouched.  n_seeds == 0 with h * w > 0: the lists are empty and hidden_stats[k] is the
 * record of the whole plane (the fold still runs); h * w == 0: the identity.  n_cuts == 0 runs nothing and writes nothing.
 * Integer sums, minima and maxima only: every record is reproducible to the bit.  Stream ordered; returns with the host arrays
 * complete.  The walk runs a second time for the measuring (no plane is read back, so d_out == NULL works).  Workspace kept by the
 * context on top of ws_tree_cut_stats_device's, reserved before anything runs: 68 B per accumulator entry, of which there are
 * min(cap, n_cuts * min(n_seeds, h * w)) + n_cuts with d_region_stats (the records a call can end with, and one per cut) and
 * n_cuts without, and 72 B per cut. */
int ws_tree_cut_catalogue_device(ws_ctx *ctx, const ws_tree_node *d_tree, const ws_lake_stats *d_stats, size_t n_seeds,
                                 const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w, const void *d_weight,
                                 int weight_dtype, size_t weight_row_stride, const ws_lake_cut *cuts, size_t n_cuts, uint32_t *d_out,
                                 size_t plane_stride, ws_lake *d_lakes, ws_lake_stats *d_region_stats, size_t cap, size_t *n_lakes,
                                 uint64_t *offsets, uint64_t *hidden, ws_lake_stats *hidden_stats);
/* The whole route from and into HOST memory, as ws_merge_tree_stats_cut: image, seeds, options, cuts, tree, stats, out, lakes, cap,
 * n_lakes, offsets and hidden as there; the weight plane as ws_merge_tree_stats (h x w, unpadded, NULL: the image itself; under
 * edge correction the ring weighs 0 and rows and columns are those of the padded plane).  region_stats (nullable, needs lakes): cap
 * records, record i measured over the pixels lakes[i] counts; hidden_stats (nullable): n_cuts records.  Keeps on the device what
 * ws_merge_tree_stats_cut and ws_tree_cut_catalogue_device keep, and cap records of 72 B. */
int ws_merge_tree_cut_catalogue(ws_ctx *ctx, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc,
                                size_t n_seeds, const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride,
                                const ws_lake_cut *cuts, size_t n_cuts, ws_tree_node *tree, ws_lake_stats *stats, uint64_t *out,
                                ws_lake *lakes, ws_lake_stats *region_stats, size_t cap, size_t *n_lakes, uint64_t *offsets,
                                uint64_t *hidden, ws_lake_stats *hidden_stats);
/* transform_history of every slice of a cube for a list of water levels (tests/integration.rs:267,356 take a cube apart slice by
 * slice), everything in HBM.  Slices, seeds, seed_offsets (n_slices + 1 entries, on the HOST), edge correction, duplicate seeds
 * and *failed_slice as ws_transform_to_list_batch_device; levels, n_levels (0: nothing runs, nothing is written), merging and the
 * planes as ws_transform_history_device.  Layout, slice-major then list order: plane (k, j) -- slice k's label plane after water
 * level levels[j], in the slice's own colours, bit-identical to what ws_transform_history_device writes for that slice alone --
 * is at d_out + (k * n_levels + j) * plane_stride.  A bad level or a short plane_stride is WS_ERR_BAD_ARG before anything runs.
 * When the slices stack (as ws_transform_to_list_batch_device) every group of slices runs as one flood, and merging as ONE run
 * of the stamping per-level unions over the stack's colours, then one render pass writes all of the group's planes; anything
 * else runs as a loop of ws_transform_history_device.  Scratch of the stacked form, kept by the context: 4 B per pixel of the
 * stack (its labels) and, merging, the merge forest of all its colours (8 B a colour).  Statistics are summed over the call's
 * transforms; afterwards ws_last_arrival_device reports "unsupported". */
int ws_transform_history_batch_device(ws_ctx *ctx, int merging, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w,
                                      size_t row_stride, size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets,
                                      const ws_options *opt, const uint8_t *levels, size_t n_levels,
                                      uint32_t *d_out, size_t plane_stride, size_t *failed_slice);
/* The same from and into HOST memory: the cube and the (row, col) seed pairs as ws_transform_to_list_batch takes them (seeds_rc ==
 * NULL: every slice's own find_local_minima, n_seeds[k], nullable, receives how many); u64 planes, contiguous, plane (k, j) at
 * out + (k * n_levels + j) * padded h * w.  Scratch, kept by the context: the cube and the seeds on the device, and the planes
 * rendered in chunks of at most 256 MiB of u32 words -- a run of whole slices where a slice's planes fit (it crosses the bus as
 * ONE copy of u32 words widened by the host threads), a run of one slice's levels where they do not. */
int ws_transform_history_batch(ws_ctx *ctx, int merging, const uint8_t *cube, size_t n_slices, size_t h, size_t w,
                               size_t row_stride, size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets,
                               const ws_options *opt, const uint8_t *levels, size_t n_levels,
                               uint64_t *out, size_t *n_seeds, size_t *failed_slice);
/* ws_merge_tree_device of every slice of a cube in one call, everything in HBM.  Slices, seeds, seed_offsets (n_slices + 1 entries,
 * on the HOST), edge correction, seed_shift, duplicate seeds and *failed_slice as ws_transform_history_batch_device.  Records,
 * slice-major: slice k with its n_k seeds owns n_k + 1 records from index (seed_offsets[k] - seed_offsets[0]) + k on, record c of
 * them colour c of the slice's own colours 1 .. n_k, `parent` in those colours too; seed count + n_slices records in all, and no
 * other word of d_tree is written.  Every record is bit-identical to what ws_merge_tree_device writes for that slice alone: a
 * slice's record 0 is (0, WS_TREE_ALIVE, pixels of that slice's padded plane still uncoloured after the last level, 0), and a
 * slice without seeds owns that one record.  d_labels (nullable): the segmenting labels of every slice, n_slices padded planes of
 * u32 in the slices' own colours (ws_segment_batch_device's).  Null pointers with non-zero sizes, bad options, offsets that
 * decrease, 0xFFFFFFFF seeds or more and a context that holds a begun transform are refused before anything runs; n_slices == 0
 * writes nothing.  When the slices stack (as ws_transform_history_batch_device) every group of slices runs as one flood and ONE run
 * of the stamping per-level unions over the stack's colours -- the captured graphs are those of the stacked history loop -- and
 * the tree kernels run once over the group: one fold launch per level for all of its slices.  Anything else, and a stack that
 * fails or mispredicts, runs as a loop of ws_merge_tree_device, which names the failing slice.  Scratch of the stacked form, kept
 * by the context: as ws_transform_history_batch_device, 16 B a colour of the largest group (its records in the stack's numbering)
 * and 2 KB a slice of arrival counts.  Statistics are summed over the call's transforms; afterwards ws_last_arrival_device reports
 * "unsupported". */
int ws_merge_tree_batch_device(ws_ctx *ctx, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                               size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                               ws_tree_node *d_tree, uint32_t *d_labels, size_t *failed_slice);
/* The same from and into HOST memory: the cube and the u64 (row, col) seed pairs as ws_transform_history_batch takes them (seeds_rc
 * == NULL: every slice's own find_local_minima, n_seeds[k], nullable, receives how many, and the records' offsets are the running
 * sum of those counts).  `tree` holds `cap` records; *n_records (nullable) receives the total, seed count + n_slices.  cap smaller
 * than that: WS_ERR_CAPACITY once the minima are found or counted and before any flood -- only *n_records and n_seeds[] are
 * meaningful then, `tree` and `labels` are untouched.  labels (nullable): n_slices padded planes of u64. */
int ws_merge_tree_batch(ws_ctx *ctx, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                        const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, ws_tree_node *tree, size_t cap,
                        size_t *n_records, uint64_t *labels, size_t *n_seeds, size_t *failed_slice);
/* ws_merge_tree_stats_device of every slice of a cube in one call, everything in HBM.  The cube, the seeds, seed_offsets, the
 * options, d_labels and *failed_slice as ws_merge_tree_batch_device; d_tree is exactly what that call writes.  d_stats has the
 * same slice-major layout: slice k's n_k + 1 records start at (seed_offsets[k] - seed_offsets[0]) + k, seed count + n_slices
 * records in all, and no other word of either array is written.  Every d_stats record is bit-identical to what
 * ws_merge_tree_stats_device writes for that slice alone with that slice's weight plane: rows, columns and peak_pixel are those of
 * the slice's own padded plane, record 0 of a slice measures the pixels of THAT slice the last level leaves uncoloured, and a
 * slice without seeds owns that one record.  d_weight (nullable: the cube itself weighs, as u8): n_slices planes of h x w elements
 * of weight_dtype (WS_U8 or WS_U16), weight_row_stride elements a row and weight_slice_stride elements from one slice's plane to
 * the next -- both independent of the cube's strides.  Refused before anything runs, every output untouched: what
 * ws_merge_tree_batch_device refuses, a null d_stats, another dtype (WS_ERR_UNSUPPORTED), weight_row_stride < w,
 * weight_slice_stride < h * weight_row_stride with more than one slice, and a slice whose weighted moments could pass 64 bits
 * (WS_ERR_TOO_LARGE: the bound of ws_merge_tree_stats_device, per slice).  n_slices == 0 writes nothing.  A group of slices that
 * stacks runs the tree kernels and the statistics kernels once over the group -- one fold launch per level for all of its
 * slices, the uncoloured pixels of every slice kept apart in an accumulator entry of their own; anything else, and a stack that
 * fails or mispredicts, runs as a loop of ws_merge_tree_stats_device, which names the failing slice.  Scratch, kept by the
 * context: as ws_merge_tree_batch_device and 68 B for every colour of the largest group, one more, and one per slice of a group. */
int ws_merge_tree_stats_batch_device(ws_ctx *ctx, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                     size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                     const void *d_weight, int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride,
                                     ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *d_labels, size_t *failed_slice);
/* The same from and into HOST memory: the cube, the seeds (seeds_rc == NULL: every slice's own find_local_minima), cap,
 * *n_records, labels and n_seeds[] as ws_merge_tree_batch; `tree` and `stats` hold `cap` records each.  cap too small:
 * WS_ERR_CAPACITY once the minima are found or counted and before any flood, `tree`, `stats` and `labels` untouched.  The weight
 * cube (nullable) is copied contiguous onto the context before the first transform; both record arrays cross the bus once. */
int ws_merge_tree_stats_batch(ws_ctx *ctx, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                              const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, const void *weight,
                              int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride, ws_tree_node *tree,
                              ws_lake_stats *stats, size_t cap, size_t *n_records, uint64_t *labels, size_t *n_seeds, size_t *failed_slice);
/* ws_merge_tree_shapes_device of every slice of a cube in one call, everything in HBM.  Every argument
 * but d_shapes as ws_merge_tree_stats_batch_device, and d_tree and d_stats are byte for byte what that call writes for the same
 * arguments.  d_shapes (device, 8-byte aligned) has the same slice-major layout: slice k's n_k + 1 records start at
 * (seed_offsets[k] - seed_offsets[0]) + k, and no other word of it is written.  Every d_shapes record is bit-identical to what
 * ws_merge_tree_shapes_device writes for that slice alone with that slice's weight plane: rows and columns are those of the slice's
 * own padded plane, record 0 of a slice covers the pixels of THAT slice the last level leaves uncoloured, a slice without seeds
 * owns that one record, and the identity is twelve zero words.  Refused before anything runs, all three outputs and d_labels
 * untouched: what ws_merge_tree_stats_batch_device refuses, in its order, then a null d_shapes and a d_shapes off 8-byte alignment
 * (WS_ERR_BAD_ARG).  There is no further WS_ERR_TOO_LARGE: the bound of the stats call is a slice's (wmax * pixels of a slice *
 * its longer side < 2^64), rows and columns restart in every slice, and every accumulator entry -- a colour, or a slice's
 * uncoloured pixels -- takes pixels of ONE slice only, so the limb argument of ws_merge_tree_shapes_device (a sum below 2^96, both
 * limbs below 2^64) holds entry by entry however many slices a group stacks.  n_slices == 0 writes nothing.  A group that stacks
 * runs the shape kernels once over the group after the statistics kernels, one fold launch per level for all of its slices;
 * anything else, and a stack that fails or mispredicts, runs as a loop that names the failing slice.  Scratch, kept by the context
 * and reserved before the first transform: as ws_merge_tree_stats_batch_device and 96 B for every colour of the largest group, one
 * more, and one per slice of a group.  Tiled groups and the regions of a cut have no such call. */
int ws_merge_tree_shapes_batch_device(ws_ctx *ctx, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                      size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                      const void *d_weight, int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride,
                                      ws_tree_node *d_tree, ws_lake_stats *d_stats, ws_lake_shape *d_shapes, uint32_t *d_labels,
                                      size_t *failed_slice);
/* The same from and into HOST memory, as ws_merge_tree_stats_batch: `tree`, `stats` and `shapes` hold `cap` records each (all three
 * required unless cap == 0).  cap too small: WS_ERR_CAPACITY once the minima are found or counted and before any flood, *n_records
 * set, the three arrays and `labels` untouched.  The three record arrays cross the bus once each; keeps 96 B a record more on the
 * device. */
int ws_merge_tree_shapes_batch(ws_ctx *ctx, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride, size_t slice_stride,
                               const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt, const void *weight,
                               int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride, ws_tree_node *tree,
                               ws_lake_stats *stats, ws_lake_shape *shapes, size_t cap, size_t *n_records, uint64_t *labels,
                               size_t *n_seeds, size_t *failed_slice);
/* ws_tree_cut_catalogue_device of every slice of a cube in one call, from records and planes held in HBM.
 * d_tree and d_stats (nullable when no cut has a catalogue threshold) in the slice-major layout ws_merge_tree(_stats)_batch_device
 * writes: seed_offsets (n_slices + 1 entries, on the HOST), slice k with its n_k = seed_offsets[k + 1] - seed_offsets[k] seeds owns
 * n_k + 1 records from rb[k] = seed_offsets[k] - seed_offsets[0] + k on, `parent` in the slice's own colours.  d_keys and
 * d_seg_labels: n_slices contiguous h x w u32 planes each, as they stand (padded planes are passed padded).  d_weight: n_slices
 * planes of h x w elements, weight_row_stride and weight_slice_stride in ELEMENTS, WS_U8 or WS_U16, nullable exactly as in the single
 * call (with both measuring outputs NULL the weight arguments are not looked at and nothing that measures is launched).  The cuts:
 * 1 .. 32 ws_lake_cut on the host.  Outputs, slice-major then cut (as ws_transform_history_batch_device lays out planes): plane
 * (k, j) at d_out + (k * n_cuts + j) * plane_stride; list (k, j) is d_lakes[offsets[k * n_cuts + j] .. offsets[k * n_cuts + j + 1]),
 * in the slice's own colours, in increasing colour; offsets (n_slices * n_cuts + 1 entries) and hidden (n_slices * n_cuts) on the
 * HOST; d_region_stats[i] next to d_lakes[i]; hidden_stats[k * n_cuts + j] on the HOST; rows, columns and peak_pixel are those of
 * the slice's own plane.  Every plane, record, offset difference, hidden count, region record and hidden record of slice k is
 * bit-identical to ws_tree_cut_catalogue_device on slice k alone with that slice's records, planes and weight plane and the same
 * cuts; slice k's lists are that call's, shifted by offsets[k * n_cuts].
 * Refused with WS_ERR_BAD_ARG before any walk runs, every output untouched: everything the single call refuses, seed_offsets that
 * decrease, weight_slice_stride < h * weight_row_stride with more than one slice, and a tree that is no merge tree WITHIN ITS SLICE:
 * record c of slice k is alive with parent 0, or dies at a level <= 254 into 0 < parent < c of the same slice that dies strictly
 * later (ONE check pass and ONE verdict, read on the host, for the whole cube; the record of a slice without seeds is not read).
 * A label above ITS OWN slice's n_k -- which may well be a valid record index of the next slice -- is compared before it indexes
 * anything, written as 0 and reported late as WS_ERR_BAD_ARG; the labels of a slice without seeds are not looked at.
 * WS_ERR_TOO_LARGE on the cube's totals: n_slices * h * w >= 2^32, seeds + n_slices >= 2^32 - 1, or with lists n_cuts * (seeds +
 * n_slices) >= 2^32.  n_slices == 0 or n_cuts == 0 writes nothing; slices without seeds and h * w == 0 behave as the single call's
 * empty cases, per slice.  Records past cap are counted, not written: *n_lakes is the need, WS_ERR_CAPACITY, and no measuring
 * kernel has run.  Workspace kept by the context: 16 B a record (the records with parents as indices into the whole array), 4 B a
 * record and table, with lists 4 B a record and cut and 12 B per 1024 of those, 16 B per slice and cut and 4 B a slice; measuring:
 * 68 B per accumulator entry -- min(cap, n_cuts * min(seeds, pixels)) + n_slices * n_cuts with d_region_stats, n_slices * n_cuts
 * without -- and 72 B per slice and cut.  No term pads a slice. */
int ws_tree_cut_catalogue_batch_device(ws_ctx *ctx, const ws_tree_node *d_tree, const ws_lake_stats *d_stats, size_t n_slices,
                                       const size_t *seed_offsets, const uint32_t *d_keys, const uint32_t *d_seg_labels, size_t h, size_t w,
                                       const void *d_weight, int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride,
                                       const ws_lake_cut *cuts, size_t n_cuts, uint32_t *d_out, size_t plane_stride, ws_lake *d_lakes,
                                       ws_lake_stats *d_region_stats, size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *hidden,
                                       ws_lake_stats *hidden_stats);
/* Cube in, everything out: ws_merge_tree_stats_batch_device and, group by group while the stamps and the labels of a flood are still
 * on the context, the cut above.  The cube, the seeds, seed_offsets, the options, the weight cube (unpadded h x w planes, the ring
 * weighs 0, NULL: the cube itself), d_labels and *failed_slice as ws_merge_tree_stats_batch_device.  d_tree is required; d_stats is
 * nullable: NULL and no catalogue threshold, the statistics pass does not run; NULL with one, WS_ERR_BAD_ARG before anything runs.
 * d_keys_out (nullable): the arrival stamps of every slice as n_slices padded planes, each bit-identical to
 * ws_copy_last_arrival_device after ws_merge_tree_device on that slice alone -- with d_labels what a later
 * ws_tree_cut_catalogue_batch_device needs to cut the same flood again.  The cut outputs are that call's, over the padded planes.
 * A stacked group is cut once, as its slices; a looped slice as one slice; lists and region records continue behind the previous
 * groups'.  Once the lists no longer fit, the remaining groups still flood and count: *n_lakes is the need, WS_ERR_CAPACITY.  A
 * stack that fails or mispredicts is abandoned and the loop starts over from record 0.  Every buffer is reserved for the largest
 * group before the first transform. */
int ws_merge_tree_cut_catalogue_batch_device(ws_ctx *ctx, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                             size_t slice_stride, const uint32_t *d_seeds_rc, const size_t *seed_offsets,
                                             const ws_options *opt, const void *d_weight, int weight_dtype, size_t weight_row_stride,
                                             size_t weight_slice_stride, const ws_lake_cut *cuts, size_t n_cuts, ws_tree_node *d_tree,
                                             ws_lake_stats *d_stats, uint32_t *d_labels, uint32_t *d_keys_out, uint32_t *d_out,
                                             size_t plane_stride, ws_lake *d_lakes, ws_lake_stats *d_region_stats, size_t cap,
                                             size_t *n_lakes, uint64_t *offsets, uint64_t *hidden, ws_lake_stats *hidden_stats,
                                             size_t *failed_slice);
/* The same from and into HOST memory: the cube, the seeds (seeds_rc == NULL: every slice's own find_local_minima), the weight cube,
 * *n_records, n_seeds[] and *failed_slice as ws_merge_tree_stats_batch; the cuts and the cut outputs as the device form, planes as
 * u64 (plane (k, j) at out + (k * n_cuts + j) * padded h * w).  Two capacities: `tree` (required) and `stats` (nullable: the
 * statistics still run when a cut has a catalogue threshold) hold record_cap records each -- too few is WS_ERR_CAPACITY once the
 * minima are found or counted and before any flood, everything else untouched; `lakes` and `region_stats` hold cap records, with the
 * device form's rule (*n_lakes is the need).  One download per output.  Keeps on the device what ws_merge_tree_stats_batch keeps,
 * the u32 planes of the whole cube and cap records of 16 B and of 72 B. */
int ws_merge_tree_cut_catalogue_batch(ws_ctx *ctx, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                      size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                                      const void *weight, int weight_dtype, size_t weight_row_stride, size_t weight_slice_stride,
                                      const ws_lake_cut *cuts, size_t n_cuts, ws_tree_node *tree, ws_lake_stats *stats, size_t record_cap,
                                      size_t *n_records, uint64_t *out, ws_lake *lakes, ws_lake_stats *region_stats, size_t cap,
                                      size_t *n_lakes, uint64_t *offsets, uint64_t *hidden, ws_lake_stats *hidden_stats, size_t *n_seeds,
                                      size_t *failed_slice);

/* ---- input preparation (first "next" row) ---------------------------------------
 *
 * WatershedUtils::pre_processor / pre_processor_with_max::<MAX> (lib.rs:1081-1173): any numeric
 * array (any dimension, passed flattened) -> u8 in [0, MAX].  Quirks reproduced as coded: min and
 * max folds are seeded with 0; values that are not `is_normal` in f64 -- NaN, -inf, subnormals AND
 * exact 0 -- become NEVER_FILL (255); +inf becomes ALWAYS_FILL (0); the rest is
 * trunc((x - min) / (max - min) * MAX) in f64.  max_value must be in 1..=254 (the reference asserts).
 *
 * Range overflow: when max - min is not finite -- WS_F64 data only, e.g. {-1e308, 1e308} -- the element equal to max is
 * inf / inf = NaN and the reference panics (`to_u8().unwrap()` on None, lib.rs:1164).  Both functions then return
 * WS_ERR_UNSUPPORTED, ws_last_error names that line, and the contents of `out` / `d_out` are unspecified.  To decide this
 * ws_pre_processor_device reads (min, max) back between its two kernels: for WS_F64 it waits for the context's stream once per
 * call (every other dtype stays asynchronous; the host form waits for its result anyway).
 *
 * n_elems == 0 writes nothing (null pointers allowed).  A context that holds a begun transform refuses both calls. */
typedef enum ws_dtype { WS_F32 = 0, WS_F64 = 1, WS_I32 = 2, WS_U16 = 3, WS_I16 = 4, WS_U8 = 5 } ws_dtype;
int ws_pre_processor(ws_ctx *ctx, const void *data, int dtype, size_t n_elems, uint8_t max_value, uint8_t *out);
int ws_pre_processor_device(ws_ctx *ctx, const void *d_data, int dtype, size_t n_elems, uint8_t max_value,
                            uint8_t *d_out);

/* ---- the front end of a cube of slices, one call each (tests/integration.rs:267-290, 356-380: pre_processor and
 * find_local_minima of one slice after the other, before any transform) ----------------------------------------------
 *
 * ws_pre_processor_batch_device: slice k of d_out is exactly ws_pre_processor_device (pre_processor_with_max::<MAX>,
 * lib.rs:1134-1173) of the h x w view whose element (r, c) sits at d_data + k * slice_stride + r * row_stride + c * col_stride --
 * strides in ELEMENTS of dtype, any non-negative values: its OWN zero-seeded (min, max), then the same quantiser.  d_out is the
 * contiguous (n_slices, h, w) u8 cube every *_batch_device call takes.  d_minmax (nullable): 2 * n_slices doubles, (min, max) of
 * every slice as the folds leave them (written before a range refusal too).  A channel-last cube (slice_stride == 1, what slicing
 * a FITS cube along its last axis gives) is read with lanes along the slice axis (and, with fewer than 64 slices, along
 * neighbouring pixels too) and transposed on the chip: no copy into contiguous planes is needed first.  max_value and dtype are checked as in the single call.  WS_F64 slices whose max - min is
 * not finite: WS_ERR_UNSUPPORTED and *failed_slice (nullable) = the lowest such slice, decided by one device word read back once
 * per call (the stream is waited for once); every other dtype stays asynchronous.  n_slices * h * w == 0 writes nothing.  A
 * context that holds a begun transform refuses the call.  Scratch kept by the context: at most 1 MiB + 32 B a slice. */
int ws_pre_processor_batch_device(ws_ctx *ctx, const void *d_data, int dtype, size_t n_slices, size_t h, size_t w,
                                  size_t slice_stride, size_t row_stride, size_t col_stride, uint8_t max_value, uint8_t *d_out,
                                  double *d_minmax, size_t *failed_slice);
/* The same from and into HOST memory: the bytes between the view's first and last element cross in ONE copy and the kernels read
 * them with the caller's strides; the u8 cube and (nullable) minmax are copied back; returns with both complete. */
int ws_pre_processor_batch(ws_ctx *ctx, const void *data, int dtype, size_t n_slices, size_t h, size_t w, size_t slice_stride,
                           size_t row_stride, size_t col_stride, uint8_t max_value, uint8_t *out, double *minmax,
                           size_t *failed_slice);

/* find_local_minima (lib.rs:1178-1197) of every slice of a u8 cube: slice k (at d_cube + k * slice_stride, row_stride >= w) gives
 * exactly the list of ws_find_local_minima_device, coordinates local to the slice; the lists lie back to back in d_out_rc -- what
 * every *_batch_device call takes as d_seeds_rc -- and seed_offsets (HOST, n_slices + 1 entries) is the array those calls take:
 * slice k's seeds are pairs [seed_offsets[k], seed_offsets[k + 1]).  *n_found = the total; cap smaller than that: WS_ERR_CAPACITY,
 * the list cut at cap, the offsets complete (d_out_rc may be NULL with cap 0: a count).  One count launch, one scan, one write
 * launch and ONE readback per run of slices; a run is as many whole slices as stay under ws_ctx_set_batch_pixel_limit, under
 * 2^31 - 16 stacked rows and under 512 MiB of scratch (256 B per row and 1024 columns).  Slices with h < 3 or w < 3 have no
 * seeds.  Each slice must have fewer than 2^32 - 1 pixels.  Scratch kept by the context: the nibble plane and the counts of the
 * largest run (up to 512 MiB + 4.5 B a stacked row).  The host *_batch forms called with seeds_rc == NULL find their seeds with this
 * call and keep that scratch too (70 001 slices of 8 x 16: 143 MB, where the per-slice loop they ran before kept one slice's). */
int ws_find_local_minima_batch_device(ws_ctx *ctx, const uint8_t *d_cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                                      size_t slice_stride, uint32_t *d_out_rc, size_t cap, size_t *seed_offsets, size_t *n_found);
/* The same from and into HOST memory, the pairs as uint64_t (what the host *_batch calls take as seeds_rc). */
int ws_find_local_minima_batch(ws_ctx *ctx, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                               size_t slice_stride, uint64_t *out_rc, size_t cap, size_t *seed_offsets, size_t *n_found);

/* ---- one field tiled over several GPUs: row blocks with halo rows ----------------------
 *
 * A rank holds its rows of the global field plus one extra (halo) row on every side that has a
 * neighbour.  The local plane's first and last rows are then either the global border or a halo,
 * which the flood never writes (lib.rs:220-222), so a block is relaxed exactly like a whole
 * image.  The caller alternates: ws_block_relax on every rank -> exchange halo rows of d_keys
 * (RCCL send/recv) -> all-reduce of `changed`, until no rank changed; then the same loop with
 * ws_block_resolve and d_labels.  Seeds carry GLOBAL colours (index in the caller's slice + 1,
 * lib.rs:1670-1672) and LOCAL coordinates; every rank paints the seeds that fall on any of its
 * local rows, halo rows included.  rustronomy-watershed_amd/distributed.py drives this. */
int ws_block_init(ws_ctx *ctx, size_t h, size_t w, const uint32_t *d_seeds_rc, const uint32_t *d_colours,
                  size_t n_seeds, uint32_t *d_keys, uint32_t *d_labels);
int ws_block_relax(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                   uint8_t max_water_level, uint32_t *d_keys, int *changed);
int ws_block_resolve(ws_ctx *ctx, const uint32_t *d_keys, uint32_t *d_labels, size_t h, size_t w, int *changed);
/* A tile of a field cut in both directions: the labels of the whole plane from painted labels, in two launches.  Seeds hold
 * their colours; the plane's border ring holds what is known of the neighbours' pixels so far (0: nothing yet) and is a set
 * of roots like the seeds.  The caller swaps the ring and repeats until nobody receives anything new (ws_segment_tiled2d*
 * do). */
int ws_block_resolve_ring(ws_ctx *ctx, const uint32_t *d_keys, uint32_t *d_labels, size_t h, size_t w);

/* The same block in its fast form, for seed lists in strictly increasing row-major order (what ws_find_local_minima
 * returns): a rank's seeds -- those on any of its local rows, halo rows included -- are then entries [g0, g0 + n) of the
 * caller's list, in local coordinates, and first_colour = g0 + 1.  Needs w % 4 == 0 and h * w < 2^31; anything else
 * (WS_ERR_UNSUPPORTED) goes through ws_block_init / _relax / _resolve above.  Sequence on every rank (distributed.py):
 *   ws_block_begin;  repeat { swap halo rows of d_keys with the neighbours; stop when no rank received a row that
 *   differs from what it held; ws_block_relax_halo };  ws_block_resolve_local;  ws_block_export_boundary;  all-gather the
 *   2 * w words of every rank into one table;  ws_block_import_boundary.
 * Stamps need that iteration (a flood may cross a seam more than once); labels do not: after the local resolve every
 * label is a colour or a reference to a neighbour's boundary-row pixel, the boundary rows of all ranks form a closed
 * table (entry (rank r, side s, column x) at (2 r + s) * w + x; s = 0 first own row, 1 last own row; a reference is
 * 0x80000000 | entry index), and every rank resolves the gathered table for itself. */
int ws_block_begin(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride, uint8_t max_water_level,
                   const uint32_t *d_seeds_rc, size_t n_seeds, uint32_t first_colour, uint32_t *d_keys);
int ws_block_relax_halo(ws_ctx *ctx, const uint8_t *d_img, size_t h, size_t w, size_t row_stride, uint8_t max_water_level,
                        int halo_top, int halo_bottom, uint32_t *d_keys);
int ws_block_resolve_local(ws_ctx *ctx, const uint32_t *d_keys, uint32_t *d_labels, size_t h, size_t w, int halo_top,
                           int halo_bottom);
int ws_block_export_boundary(ws_ctx *ctx, const uint32_t *d_labels, size_t h, size_t w, int halo_top, int halo_bottom,
                             size_t rank, uint32_t *d_rows /* 2 * w words */);
int ws_block_import_boundary(ws_ctx *ctx, const uint32_t *d_table /* world * 2 * w words */, size_t world, size_t rank,
                             uint32_t *d_labels, size_t h, size_t w, int halo_top, int halo_bottom);

/* The MERGING transform's final canonical labels of a tiled field (lib.rs:1328-1522 over row blocks), after the tiled
 * segmenting transform has left d_labels (halo rows included) final.  d_parent: n_colours_total + 1 words (colour 0 =
 * uncoloured), a union-find over ALL seed colours of the field, owned by the caller.  row0 = field row of the block's
 * first local row.  Sequence: ws_block_merge_local; ws_block_merge_export (4 * w (colour, root) pairs: the block's two
 * boundary rows and its halo rows); all-gather of the pairs; ws_block_merge_import; ws_block_merge_relabel.  One
 * exchange, no rounds: a lake that spans several blocks is a chain of local pieces linked at boundary colours. */
int ws_block_merge_local(ws_ctx *ctx, const uint32_t *d_labels, size_t h, size_t w, size_t row0, size_t field_rows,
                         size_t n_colours_total, uint32_t *d_parent);
int ws_block_merge_export(ws_ctx *ctx, const uint32_t *d_labels, size_t h, size_t w, uint32_t *d_parent, uint32_t *d_pairs);
int ws_block_merge_import(ws_ctx *ctx, const uint32_t *d_pairs, size_t n_pairs, uint32_t *d_parent);
int ws_block_merge_relabel(ws_ctx *ctx, const uint32_t *d_labels, size_t n, uint32_t *d_parent, size_t n_colours_total,
                           uint32_t *d_out);

/* ---- several GPUs driven inside the library --------------------------------------------------------
 *
 * The reference's drivers are one address space and one rayon pool (lib.rs:1689-1748); a drop-in that wants the GPUs of a
 * node behind the same transform() call cannot ask its caller to bring torch.distributed or MPI.  A ws_group is a set of
 * RANKS, each with a context of its own on one device, plus the three exchange steps the tiled transform needs -- swap the
 * halo rows with the neighbour ranks, max-reduce one word, all-gather a small table -- in one of two implementations:
 *
 *   local  all ranks live in THIS process (one host thread each while a call runs); rank r sits on devices[r].  The
 *          exchange steps are stream-ordered copies between the ranks' buffers (peer-to-peer between devices).  A device
 *          may appear more than once: ranks then share it -- the protocol rehearsed on a one-GPU box, and what the tests run.
 *   rccl   THIS process is ONE rank of `world` (one process per GPU: torchrun / mpirun).  Halo rows travel as grouped
 *          ncclSend / ncclRecv pairs, the flag word through ncclAllReduce(max), tables through ncclAllGather, all on the
 *          rank's own stream, over xGMI.  librccl.so is loaded when the first such group is created.  Every rank passes the
 *          same 128-byte id, made by ONE rank with ws_group_rccl_unique_id and handed to the others by whatever the job
 *          already uses (MPI_Bcast, a file, torch.distributed.broadcast).
 *
 * Either way the transform is the single-domain one bit for bit (the arrival-stamp fixpoint is unique, DESIGN.md section
 * 2 and 6): row blocks with one halo row per neighbour; stamps iterate (relax to local convergence, swap halo rows, stop
 * when no rank received a row that differs from the one it held -- the difference is found on the device and reduced
 * there, one host read per round); labels need one all-gather of the ranks' boundary rows (2 * w words per rank). */
typedef struct ws_group ws_group;
#define WS_RCCL_ID_BYTES 128

int ws_group_create_local(int n_ranks, const int *devices /* n_ranks entries; NULL: every rank on device 0 */, ws_group **out);
int ws_group_rccl_unique_id(void *id /* WS_RCCL_ID_BYTES */);
int ws_group_create_rccl(int device, int rank, int world, const void *id /* WS_RCCL_ID_BYTES */, ws_group **out);
void ws_group_destroy(ws_group *g);
/* world: ranks of the whole group; n_local: ranks driven by this process (local: all; rccl: 1); first_local: the first of them */
int ws_group_info(const ws_group *g, int *world, int *n_local, int *first_local);
const char *ws_group_last_error(const ws_group *g);
/* Runs every exchange step of the group once on small buffers and checks the results (WS_OK, or WS_ERR_RCCL / WS_ERR_HIP):
 * a deployment check that the transport works before a field is committed to it.  Collective: every rank calls it. */
int ws_group_selftest(ws_group *g);

/* Rows of a field of `h` rows that rank `rank` of `world` OWNS: [*r0, *r1); its local plane is rows [*lo, *hi) = the same
 * plus one halo row on every side that has a neighbour.  WS_ERR_BAD_ARG when h < world (every rank must own a row). */
int ws_tile_rows(size_t h, int rank, int world, size_t *r0, size_t *r1, size_t *lo, size_t *hi);

/* The ws_*_tiled* calls below.  A call that is wrong in several ways reports the first of: the group and the options (a null
 * options pointer, ws_options_validate, the sweep engine on more than one rank); a null `blocks` or host output pointer; py * px
 * against the group's ranks; edge correction on a device form (WS_ERR_UNSUPPORTED: pad first, the host forms do); a field with
 * fewer rows (tiles: or columns) than ranks; a seed count of 2^31 - 1 or more (WS_ERR_TOO_LARGE); a null device output on the
 * process that holds rank 0; the catalogue's weights; a block descriptor.  A refused call has queued no work. */

/* One field tiled over the ranks of a group, host buffers in and out -- what a caller of transform(ArrayView2<u8>, &seeds)
 * (lib.rs:1810) has.  Every rank of the group calls it with the SAME arguments (local: one call drives all ranks); rank r
 * uploads its rows of the image, takes its part of the seed list (any list: one that is not strictly increasing, or a
 * width that is not a multiple of 4, takes the general form -- painted seeds, iterative label rounds -- on all ranks
 * together), and writes the rows it owns of out_labels -- for a local group that is all of them.  merging != 0: the
 * MERGING transform's final canonical labels (lib.rs:1328-1522 after the last level).  Edge correction pads the field
 * first, as the reference does (lib.rs:1640-1666): out_labels is (h + 2) x (w + 2) then.  *exchange_rounds (nullable):
 * collective steps of the call. */
int ws_segment_tiled(ws_group *g, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc,
                     size_t n_seeds, const ws_options *opt, int merging, uint64_t *out_labels, uint32_t *exchange_rounds);

/* The same with everything resident in HBM: one descriptor per LOCAL rank (ws_group_info), in rank order. */
typedef struct ws_tile_block {
  const uint8_t *d_img;        /* the rank's local plane: rows [lo, hi) of the field (ws_tile_rows), row stride w, on the rank's device */
  const uint32_t *d_seeds_rc;  /* the seeds that fall on ANY local row, halo rows included, in LOCAL coordinates (row - lo, col) */
  const uint32_t *d_colours;   /* their colours (index in the caller's list + 1, lib.rs:1670-1672); NULL: first_colour, first_colour + 1, ...
                                  -- a contiguous range of a strictly increasing list, which is what the fast form needs */
  size_t n_seeds;
  uint32_t first_colour;
  uint32_t reserved;           /* must be zero */
  uint32_t *d_labels;          /* out: the local plane's labels, (hi - lo) x w u32; rows 0 / last are halo rows where the rank has neighbours */
} ws_tile_block;
int ws_segment_tiled_device(ws_group *g, size_t field_h, size_t w, size_t n_seeds_total, const ws_tile_block *blocks,
                            const ws_options *opt /* edge_correction must be 0: pad the field first */, int merging,
                            uint32_t *exchange_rounds);

/* transform_to_list (lib.rs:1551-1561 merging, 1837-1847 segmenting) of a field in row blocks (blocks as for
 * ws_segment_tiled_device, whose segmenting transform runs first and leaves every block's labels in d_labels): the ranks then
 * send the arrival stamps and labels of their owned rows to rank 0 (8 B per pixel, one message per rank and plane), and rank
 * 0's context writes the lake records of all levels from the whole plane (ws_lists_from_arrival_device).  d_lakes (cap
 * records, on rank 0's device), n_lakes, offsets (max_water_level + 2) and uncoloured (max_water_level + 1) are filled in the
 * process that holds rank 0; elsewhere *n_lakes = 0 and the arrays are left alone.  A lake spans blocks and its area is a sum
 * over them: the lists are global, so they are made where the whole plane is -- 28 B per pixel of one device's 288 GB. */
int ws_transform_to_list_tiled_device(ws_group *g, size_t field_h, size_t w, size_t n_seeds_total, const ws_tile_block *blocks,
                                      const ws_options *opt, int merging, ws_lake *d_lakes, size_t cap, size_t *n_lakes,
                                      uint64_t *offsets, uint64_t *uncoloured, uint32_t *exchange_rounds);
/* ... and with host buffers, as ws_segment_tiled takes them (edge correction by padding: the lists are those of the padded
 * plane, as ws_transform_to_list's): every rank uploads its rows, the records come back from rank 0's device into `lakes`
 * (cap records; WS_ERR_CAPACITY with the count in *n_lakes when that is too few).  What a Rust caller of transform_to_list gets
 * from several GPUs. */
int ws_transform_to_list_tiled(ws_group *g, int merging, const uint8_t *img, size_t h, size_t w, size_t row_stride,
                               const uint64_t *seeds_rc, size_t n_seeds, const ws_options *opt, ws_lake *lakes, size_t cap,
                               size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured, uint32_t *exchange_rounds);

/* The field cut in BOTH directions (BASELINE config 5's "2-D tiles"): py x px tiles, rank = ty * px + tx, py * px = the
 * group's ranks.  ws_tile_grid: rows[4] = {r0, r1, lo, hi} and cols[4] = {c0, c1, clo, chi} of a rank's tile -- owned
 * [r0, r1) x [c0, c1), held [lo, hi) x [clo, chi) with a halo row / column on every side that has a neighbour (ws_tile_rows
 * in each direction).  One descriptor per LOCAL rank; seeds carry their colours (index in the caller's list + 1,
 * lib.rs:1670-1672: a tile's seeds are no contiguous range of the list).  The exchange is halo rows AND columns, 2 (w + h)
 * words a tile and round; the block steps are the general form's (painted seeds, relaxation rounds, label rounds: the
 * seed-table / boundary-table shortcuts of the row-block form are not built for tiles).  merging != 0: the MERGING transform's
 * final canonical labels (one more gather: (colour, root) pairs of every tile's outermost rows and columns). */
typedef struct ws_tile_block2d {
  const uint8_t *d_img;        /* the tile's plane [lo, hi) x [clo, chi) of the field, on the rank's device */
  size_t img_stride;           /* >= chi - clo (a view into the whole field works) */
  const uint32_t *d_seeds_rc;  /* seeds on ANY pixel of the plane, halo ring included, LOCAL coordinates (row - lo, col - clo) */
  const uint32_t *d_colours;   /* their colours */
  size_t n_seeds;
  uint32_t *d_labels;          /* out: (hi - lo) x (chi - clo) u32 */
} ws_tile_block2d;
int ws_tile_grid(size_t h, size_t w, int rank, int py, int px, size_t *rows /* 4 */, size_t *cols /* 4 */);
int ws_segment_tiled2d_device(ws_group *g, size_t field_h, size_t field_w, int py, int px, size_t n_seeds_total,
                              const ws_tile_block2d *blocks, const ws_options *opt, int merging, uint32_t *exchange_rounds);
/* transform_to_list of a field in py x px tiles: ws_transform_to_list_tiled_device with the owned rectangles gathered on rank 0. */
int ws_transform_to_list_tiled2d_device(ws_group *g, size_t field_h, size_t field_w, int py, int px, size_t n_seeds_total,
                                        const ws_tile_block2d *blocks, const ws_options *opt, int merging, ws_lake *d_lakes,
                                        size_t cap, size_t *n_lakes, uint64_t *offsets, uint64_t *uncoloured,
                                        uint32_t *exchange_rounds);
/* ... with host buffers in and out, as ws_segment_tiled: every rank of the group calls it with the SAME arguments, uploads its
 * tile, takes its seeds (any list), writes the rectangle it owns of out_labels.  Edge correction pads the field first. */
int ws_segment_tiled2d(ws_group *g, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc,
                       size_t n_seeds, const ws_options *opt, int py, int px, int merging, uint64_t *out_labels,
                       uint32_t *exchange_rounds);

/* The merging transform's lake hierarchy (ws_merge_tree_device) and, with d_stats != NULL, the catalogue of its lakes
 * (ws_merge_tree_stats_device) of a field in row blocks: blocks and flood as ws_transform_to_list_tiled_device -- the segmenting
 * flood runs on all ranks and leaves every block's labels in d_labels -- then the owned rows of stamps and labels are gathered on
 * rank 0 (8 B per pixel), whose context calls ws_merge_tree_from_arrival_device on the whole plane.  d_tree, d_stats (n_seeds_total
 * + 1 records each) and d_weight (the whole field_h x w plane, weight_row_stride elements a row) live on rank 0's device, in the
 * process that holds rank 0; elsewhere they are ignored.  No rank holds the whole image: d_stats != NULL with d_weight == NULL is
 * WS_ERR_BAD_ARG before anything runs.  Edge correction is WS_ERR_UNSUPPORTED (pad the field first), colours stay below 2^31 and
 * every rank owns a row, as for the lists.  The records equal the single-context call's on the whole field bit for bit.  Rank 0
 * holds, per pixel, the 8 B gathered and the unions' buckets (at most 20 B); per colour 16 B of union-find and forest, 8 B of
 * recovered seed pixels, 4 B of ordering, and 68 B more with the catalogue -- all reserved before the first gather. */
int ws_merge_tree_tiled_device(ws_group *g, size_t field_h, size_t w, size_t n_seeds_total, const ws_tile_block *blocks,
                               const ws_options *opt, const void *d_weight, int weight_dtype, size_t weight_row_stride,
                               ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *exchange_rounds);
/* ... of a field in py x px tiles: blocks and flood as ws_transform_to_list_tiled2d_device, the owned rectangles gathered on rank 0. */
int ws_merge_tree_tiled2d_device(ws_group *g, size_t field_h, size_t field_w, int py, int px, size_t n_seeds_total,
                                 const ws_tile_block2d *blocks, const ws_options *opt, const void *d_weight, int weight_dtype,
                                 size_t weight_row_stride, ws_tree_node *d_tree, ws_lake_stats *d_stats, uint32_t *exchange_rounds);
/* ... and with host buffers, as ws_transform_to_list_tiled takes them: every rank of the group calls it with the SAME arguments
 * and uploads its rows; `tree` and `stats` (nullable; n_seeds + 1 records each) are filled in the process that holds rank 0.
 * Edge correction pads the field first (lib.rs:1640-1666): the tree is that of the padded plane, seed_shift is honoured and the
 * weight plane gets a ring of weight 0, as ws_merge_tree_stats does it.  weight == NULL: the image itself as u8, which rank 0
 * uploads whole.  For every option combination ws_merge_tree_stats accepts the records equal its records on the same arguments. */
int ws_merge_tree_tiled(ws_group *g, const uint8_t *img, size_t h, size_t w, size_t row_stride, const uint64_t *seeds_rc,
                        size_t n_seeds, const ws_options *opt, const void *weight, int weight_dtype, size_t weight_row_stride,
                        ws_tree_node *tree, ws_lake_stats *stats, uint32_t *exchange_rounds);

/* BASELINE config C4 over a group: a batch of independent slices, slice i on rank i % world, a rank's slices as ONE stacked
 * transform (ws_segment_batch_device) -- no exchange step at all.  One descriptor per LOCAL rank: the rank's own slices,
 * contiguous in its HBM.  Local groups run their ranks side by side (a host thread each). */
typedef struct ws_batch_part {
  const uint8_t *d_cube;         /* n_slices slices of h x w, contiguous (slice stride h * w), on the rank's device */
  const uint32_t *d_seeds_rc;    /* all of its slices' (row, col) pairs, concatenated */
  const size_t *seed_offsets;    /* n_slices + 1 entries, on the HOST */
  size_t n_slices;
  uint32_t *d_labels;            /* n_slices planes */
} ws_batch_part;
int ws_segment_batch_group(ws_group *g, size_t h, size_t w, const ws_batch_part *parts, const ws_options *opt,
                           size_t *failed_rank, size_t *failed_slice);

/* The same batch from HOST memory (ws_segment_batch above) over the ranks of a group: rank r takes the slices
 * [n_slices r / world, n_slices (r + 1) / world) of the cube and pipelines them on its own device -- every device on its own link
 * to the host, the config-4 shape for a caller whose cube lives in host memory.  Arguments as ws_segment_batch (seed_offsets and
 * n_seeds index the WHOLE cube); a process drives its local ranks only: in an RCCL group, its one rank's block of slices, read
 * from and written to that process's pointers.  No exchange step.  *failed_slice: the lowest failing slice of the local ranks. */
int ws_segment_batch_host(ws_group *g, const uint8_t *cube, size_t n_slices, size_t h, size_t w, size_t row_stride,
                          size_t slice_stride, const uint64_t *seeds_rc, const size_t *seed_offsets, const ws_options *opt,
                          uint64_t *out_labels, size_t *n_seeds, size_t *failed_slice);

/* Bench/test synthetic field: v = mix64((seed << 40) + index) % 254. */
int ws_random_field_device(ws_ctx *ctx, uint8_t *d_img, size_t h, size_t w, size_t row_stride,
                           uint64_t seed);

#ifdef __cplusplus
}
#endif
#endif
