// ws_lists.hpp -- what the cube drivers (ws_batch.hip) call of the per-level driver and the single-field forms (ws_lists.hip).
#pragma once

#include "ws_ctx.hpp"
#include "ws_level_plan.hpp"

namespace wsapi {

constexpr size_t HISTORY_SCRATCH_BYTES = (size_t)256 << 20;      // the host forms' u32 planes on the device, at most, per chunk of levels

int merge_host(ws_ctx *c, const LevelJob &job);
int ensure_uf(ws_ctx *c, size_t n_colours);
void stats_add(ws_stats &a, const ws_stats &b);
int records_to_host(ws_ctx *c, const ws_lake *d_rec, ws_lake *lakes, size_t from, size_t end, size_t n, hipStream_t on);
int planes_to_host(ws_ctx *c, const uint32_t *src, uint64_t *dst, size_t n_planes, size_t n);
int check_history(ws_ctx *c, size_t h, size_t w, size_t stride, const ws_options *opt, const uint8_t *levels, size_t n_levels, size_t *n_px);
HistoryTable history_table(const uint8_t *levels, size_t k0, size_t k1);
int render_levels(ws_ctx *c, bool merging, const HistoryTable &tab, uint32_t *d_out, size_t plane_stride, size_t n);
int check_lake_weights(ws_ctx *c, size_t w, size_t ph, size_t pw, const void *weight, int dtype, size_t weight_stride);
int build_tree(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph, size_t pw,
               ws_tree_node *d_tree);
int build_lake_stats(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph,
                     size_t pw, const ws_tree_node *d_tree, const LakeWeights &wt, ws_lake_stats *d_stats);
int build_lake_shapes(ws_ctx *c, const uint32_t *keys, const uint32_t *seg, const uint32_t *d_seeds, size_t n_seeds, const ws_options *opt, size_t ph,
                      size_t pw, const ws_tree_node *d_tree, const LakeWeights &wt, ws_lake_shape *d_shapes);

// The cut of a cube of slices, or of one group of it (ws_tree_cut.hip): the records of n_slices trees one
// behind the other (slice k's from seed_offsets[k] - seed_offsets[0] + k on), their stamps and labels as n_slices contiguous h x w
// planes, the cuts, and the outputs of ws_tree_cut_catalogue_batch_device.  measure: wt is set and the measuring outputs count.
struct CutCube {
  const ws_tree_node *d_tree = nullptr;
  const ws_lake_stats *d_stats = nullptr;
  size_t n_slices = 0;
  const size_t *seed_offsets = nullptr;
  const uint32_t *d_keys = nullptr, *d_seg_labels = nullptr;
  size_t h = 0, w = 0;
  const ws_lake_cut *cuts = nullptr;
  size_t n_cuts = 0;
  uint32_t *d_out = nullptr;
  size_t plane_stride = 0;
  ws_lake *d_lakes = nullptr;
  ws_lake_stats *d_region_stats = nullptr;
  size_t cap = 0, *n_lakes = nullptr;
  uint64_t *offsets = nullptr, *hidden = nullptr;
  ws_lake_stats *hidden_stats = nullptr;
  bool measure = false;
  LakeWeights wt{};
};
int cut_cube_check(ws_ctx *c, const CutCube &q, bool have_stats);      // the cuts and the outputs: the single call's refusals
int cut_cube_sizes(ws_ctx *c, size_t n_slices, size_t seeds, size_t plane, size_t n_cuts, bool lists);      // WS_ERR_TOO_LARGE on the totals
int cut_cube_reserve(ws_ctx *c, size_t n_slices, size_t seeds, size_t n, const CutCube &q);      // the workspace of a group that large
int cut_cube_run(ws_ctx *c, const CutCube &q);      // checked arguments, n_slices and n_cuts > 0; WS_ERR_CAPACITY: *n_lakes is the need

}  // namespace wsapi
