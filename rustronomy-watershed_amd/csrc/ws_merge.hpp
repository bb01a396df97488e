// ws_merge.hpp -- launch wrappers of the merging-transform kernels, in three sources: ws_merge.hip (the level loop),
// ws_merge_final.hip (final labels only) and ws_merge_tree.hip (what reads the stamped forest); ws_uf.hpp is what they share.
//
// The reference's merging driver (lib.rs:1328-1522) floods exactly like the segmenting one
// and, after every level, merges every pair of touching lakes (find_merge lib.rs:393-445,
// make_colour_map 467-542, recolour 589-592).  Because a flooded pixel always takes the
// colour of an already coloured neighbour, the lakes after level l are the connected
// components of the pixels coloured by level l, and -- expressed over the SEGMENTING
// result -- the classes of a union-find over seed colours joined by every adjacent pixel
// pair (p, q) with different segmenting colours and max(level(p), level(q)) <= l, where
// at least one of p, q is interior (find_merge only looks at 3x3 window centres).
// The canonical lake id is the smallest colour of the class = the union-by-min root.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace wsk {

constexpr int NLEVELS = 256;

typedef unsigned long long u64c;

// ==== ws_merge.hip: the level loop -- buckets, unions, areas, lake records, the live-lake list, the stamped unions ====
// parent[i] = i for i in 0..n, size[i] = 0
hipError_t uf_init(hipStream_t s, uint32_t *parent, uint32_t *size, size_t n);

// per-level histograms of arriving pixels and of label-crossing edges (256 bins each)
// slice_base (nullable): the plane is a stack of slices of slice_h rows whose labels restart at 1 in every slice; colour c of
// slice k is c + slice_base[k] (one numbering for the stack) and no pair crosses a slice border
hipError_t level_hist(hipStream_t s, const uint32_t *keys, const uint32_t *labels, int h, int w, u64c *hist_px, u64c *hist_edge, int slice_h, const uint32_t *slice_base);
// bucketed scatter: px_items[cursor_px[lvl]++] = colour, edge_items[cursor_edge[lvl]++] = (a,b)
hipError_t level_scatter(hipStream_t s, const uint32_t *keys, const uint32_t *labels, int h, int w, u64c *cursor_px, u64c *cursor_edge,
                         uint32_t *px_items, uint2 *edge_items, int slice_h, const uint32_t *slice_base);

// exclusive prefix sums of the histograms (NLEVELS + 1 entries each) and the scatter cursors, all on the device
hipError_t level_offsets(hipStream_t s, const u64c *hist_px, const u64c *hist_ed, u64c *off_px, u64c *off_ed, u64c *cur_px, u64c *cur_ed);
// the per-level kernels on a bucket whose bounds {first, end} sit in device memory (range = off + level): fixed grid,
// grid-stride loops -- nothing the host has to read before it launches, so the whole level loop can be captured
// lock-free union-by-min of the bucket's edges; every node that loses its root status is appended to hooked (nullable)
hipError_t union_edges_ranged(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned grid, uint32_t *parent, uint32_t *hooked,
                              uint32_t *hooked_count);
// areas of the nodes hooked in this level to their roots (hooked may be null: nothing was hooked) + arriving pixels counted
hipError_t fold_and_add_ranged(hipStream_t s, const uint32_t *hooked, const uint32_t *hooked_count, const uint32_t *px_items,
                               const u64c *range, unsigned grid, uint32_t *parent, uint32_t *size);
// the same unions of n edges the host holds the count of (the gathered pairs of a tiled field's blocks)
hipError_t union_edges(hipStream_t s, const uint2 *edges, size_t n, uint32_t *parent, uint32_t *hooked, uint32_t *hooked_count);
// appends (colour, area) of every root with area > 0 behind the records of the earlier levels; counts past cap too
// level_counts: one record counter per level, zero on entry; the records of level l start at the sum of
// level_counts[0 .. l) (earlier launches) and level_counts[l] receives this level's count
// death (nullable): per colour, the level at which it stopped being a root (union_emit keeps it); then "lake of `level`"
// means death[c] > level instead of parent[c] == c
hipError_t emit_lakes(hipStream_t s, const uint32_t *parent, const uint32_t *size, size_t n_colours,
                      uint64_t *lakes, size_t cap, u64c *level_counts, uint32_t level, const uint32_t *death = nullptr);
// the unions of `level` (bucket bounds in device memory) and the lake records of level - 1 in one launch; death: n_colours
// words, 0xFFFFFFFF at the start
hipError_t union_emit(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned union_grid, uint32_t *parent, uint32_t *hooked,
                      uint32_t *hooked_count, uint32_t *death, uint32_t level, const uint32_t *size, size_t n_colours, uint64_t *lakes,
                      size_t cap, u64c *level_counts);

// merging transform_to_list at size (ws_merge.hip, "records from the list of LIVE lakes"): sd[c] = (area, death level);
// alive: two lists of alive_list_words(n_colours) words; level L reads list (L + 1) & 1 (level 0: every colour) and writes list L & 1
hipError_t sd_init(hipStream_t s, uint2 *sd, size_t n);      // (0, 0xFFFFFFFF)
size_t alive_list_words(size_t n_colours);                   // words of ONE of the two live lists
hipError_t union_emit_alive(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned union_grid, uint32_t *parent, uint32_t *hooked,
                            uint32_t *hooked_count, uint2 *sd, uint32_t level, size_t n_colours, uint32_t *alive, unsigned emit_grid,
                            uint64_t *lakes, size_t cap, u64c *level_counts);
hipError_t emit_alive(hipStream_t s, const uint2 *sd, size_t n_colours, uint32_t *alive, unsigned emit_grid, uint64_t *lakes, size_t cap,
                      u64c *level_counts, uint32_t L);
hipError_t fold_and_add_sd(hipStream_t s, const uint32_t *hooked, const uint32_t *hooked_count, const uint32_t *px_items, const u64c *range,
                           unsigned grid, uint32_t *parent, uint2 *sd);

// out[p] = coloured by `level` ? root(labels[p]) : 0
hipError_t relabel_u32(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *parent, uint32_t *out, size_t n, uint32_t level);
hipError_t relabel_u64(hipStream_t s, const uint32_t *keys, const uint32_t *labels, uint32_t *parent, uint64_t *out, size_t n, uint32_t level);

// transform_history (ws_transform_history_device): the unions of `level` that also stamp the merge forest -- hook[b] = the root b
// was hooked under, death[b] = level (death: 0xFFFFFFFF at the start; hook is read only where death is set)
hipError_t union_stamped_ranged(hipStream_t s, const uint2 *edge_items, const u64c *range, unsigned grid, uint32_t *parent, uint32_t *death,
                                uint32_t *hook, uint32_t level);

// A stack of n_slices slices of slice_h x w pixels flooded as one plane (labels restart at 1 in every slice; base: n_slices + 1
// words, colour c of slice k is c + base[k] in the stack's numbering).
// hist[k * NLEVELS + l] += pixels of slice k that arrive at level l (n_slices * NLEVELS words, zeroed by the caller)
hipError_t slice_arrivals(hipStream_t s, const uint32_t *keys, size_t plane, size_t n_slices, u64c *hist);
// the stack's lake records (level-major, off: levels + 1 prefix sums, stack colours) into slice-major bins k * levels + l:
// scatter false adds the bins' counts into `bins`; true writes every record, as (colour - base[k], area), at out[bins[bin]++]
hipError_t split_records(hipStream_t s, bool scatter, const uint64_t *rec, size_t n_rec, const u64c *off, uint32_t levels,
                         const uint32_t *base, uint32_t g, u64c *bins, uint64_t *out);

// ==== ws_merge_final.hip: final labels only (coloured <=> label != 0) ====
// merging across the row blocks of a tiled field: joins the touching colours of one block (seam pairs to its halo rows
// included; row0 = field row of the block's first local row, H = rows of the whole field), and the (colour, root) pairs
// of the block's boundary and halo rows (4 * w of them) that the ranks exchange
hipError_t block_union_pixels(hipStream_t s, const uint32_t *labels, int h, int w, int row0, int H, uint32_t *parent, int col0 = 0, int W = -1);      // (a tile: its first column in the field, the field's width)
hipError_t block_colour_roots2d(hipStream_t s, const uint32_t *labels, int h, int w, uint32_t *parent, uint2 *pairs, size_t n_pairs);      // rows and columns: 4 w + 4 h pairs, (0, 0) after them
hipError_t block_colour_roots(hipStream_t s, const uint32_t *labels, int h, int w, uint32_t *parent, uint2 *pairs);

// the whole image: every crossing edge joined, tile by tile; tile_min: union_image_tiles(h, w) words of scratch
// preclassified: resolve_two_launch filled tile_min; tile_root_mark: n_seeds + 1 zeroed words (k_union_seeds' plain-store hooks)
size_t union_image_tiles(int h, int w);
hipError_t union_image(hipStream_t s, const uint32_t *labels, const uint32_t *seeds_rc, size_t n_seeds, int h, int w,
                       uint32_t *parent, uint32_t *tile_min, bool preclassified, uint32_t *tile_root_mark);
// flattens the forest (n_colours entries, entry 0 = "uncoloured" points at itself) and gathers out[i] = root(labels[i])
hipError_t relabel_final_u32(hipStream_t s, const uint32_t *labels, uint32_t *parent, size_t n_colours, uint32_t *out, size_t n,
                             uint32_t *tile_min = nullptr, int h = 0, int w = 0);      // tile_min: union_image's classification of the h x w plane's tiles (one-lake tiles are filled)
// a stack of slices (as slice_arrivals'): final canonical labels of every slice, in place (parent: n_colours = base[n_slices] + 1
// words, uf_init'ed)
hipError_t merge_stack(hipStream_t s, uint32_t *labels, int slice_h, int w, size_t n_slices, const uint32_t *base, uint32_t *parent,
                       size_t n_colours);

// ==== ws_merge_tree.hip: what reads the stamped forest (death / hook) -- history planes, the merge tree, lake statistics ====
// the requested levels in ascending order: e[j] = level | slot << 8 (slot: the output plane, at out + slot * plane_stride)
constexpr int HISTORY_MAX_LEVELS = 256;
struct HistoryTable {
  uint32_t n;
  uint32_t e[HISTORY_MAX_LEVELS];
};
// one pass over the plane's stamps and segmenting colours for all of tab's levels: out = coloured by L ? colour : 0, the colour
// being the segmenting one or (merging) the lake's canonical id at L found up the stamped forest
hipError_t render_history(hipStream_t s, bool merging, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                          const HistoryTable &tab, uint32_t *out, size_t plane_stride, size_t n);
// the same over slices [k0, k1) of a stack (ws_transform_history_batch_device): keys / labels from slice k0 on, n = (k1 - k0) *
// plane pixels (below 2^32), labels in each slice's own colours; base: the colour bases of slices k0 .. k1 in the forest's
// numbering (merging only); plane kr * per_slice + slot of out is slice k0 + kr's plane of the table's slot
struct HistoryStack {
  const uint32_t *base;
  uint32_t plane, per_slice;
};
hipError_t render_history_stack(hipStream_t s, bool merging, const uint32_t *keys, const uint32_t *labels, const uint32_t *death,
                                const uint32_t *hook, const HistoryTable &tab, uint32_t *out, size_t plane_stride, size_t n,
                                const HistoryStack &st);

// merge tree (ws_merge_tree_device): one record per seed colour from the stamped forest (death / hook) of a merging transform_history
// run, the flood's stamps and segmenting colours.  The records are their own accumulators: area and n_leaves are added to in place.
constexpr uint32_t TREE_ALIVE = 0xFFFFFFFFu;
struct TreeRec {      // == ws_tree_node
  uint32_t parent, death_level, area, n_leaves;
};
constexpr int TREE_WS_WORDS = 3 * (NLEVELS + 1);      // u64 words of scratch: deaths per level, their prefix sums, the scatter's cursors
// every record: death level, canonical parent (the walk from hook[c] while death[x] <= death[c]), n_leaves = 1 where the seed pixel
// of c carries c (seeds_rc: n_colours - 1 pairs in the plane's own coordinates), area 0; record 0: n - arrived[0] uncoloured pixels.
// ws: TREE_WS_WORDS zeroed words; ws[l] += colours that die at level l
hipError_t tree_init(hipStream_t s, const uint32_t *death, const uint32_t *hook, const uint32_t *seeds_rc, const uint32_t *seg_labels, int h, int w,
                     const u64c *arrived, TreeRec *tree, size_t n_colours, u64c *ws);
// the seed pairs tree_init and lake_stats read, recovered from a finished transform's planes (ws_merge_tree_from_arrival_device):
// out_rc (2 * (n_colours - 1) words, 8-byte aligned) is filled with 0xFFFFFFFF -- "never was" -- and every stamp-0 pixel whose
// label c lies in 1 .. n_colours - 1 writes its (row, col) to pair c - 1.  keys and seg need only be 4-byte aligned.
hipError_t seed_pixels_from_planes(hipStream_t s, const uint32_t *keys, const uint32_t *seg, int h, int w, size_t n_colours, uint32_t *out_rc);
// tree[r].area += 1 for every coloured pixel, r = the root of its colour at its arrival level
hipError_t tree_own_counts(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, TreeRec *tree, size_t n);
// order[]: the colours that die, bucketed by death level (bounds: ws[NLEVELS + 1 + l]); then level by level, ascending, every dying
// colour hands area and n_leaves to its parent (children die strictly before their parents)
hipError_t tree_fold(hipStream_t s, TreeRec *tree, size_t n_colours, uint32_t levels, u64c *ws, uint32_t *order);
// The same over the forest of a stack of slices (ws_merge_tree_batch_device): g slices of `plane` pixels (plane % 4 == 0), colour c
// of the forest = colour c - base[k] of its slice k (base: g + 1 words on the device, sorted).  tree_init_stack / tree_own_counts_stack
// fill `tree` in the FOREST's numbering (n_colours = the stack's seeds + 1; parents too), tree_fold folds it as it is -- one launch per
// level for the whole stack -- and tree_unstack writes the caller's layout: slice k's records at out[base[k] + k ...], own colours,
// record 0 = plane - the slice's arrivals of levels 0 .. levels - 1 (hist: slice_arrivals').
struct TreeStack {
  const uint32_t *base;
  uint32_t g, plane;
};
hipError_t tree_init_stack(hipStream_t s, const uint32_t *death, const uint32_t *hook, const uint32_t *stacked_rc, const uint32_t *seg_labels, int h, int w,
                           TreeRec *tree, size_t n_colours, u64c *ws, const TreeStack &st);
hipError_t tree_own_counts_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, TreeRec *tree,
                                 size_t n, const TreeStack &st);
hipError_t tree_unstack(hipStream_t s, const TreeRec *forest, size_t n_seeds, const uint32_t *base, size_t g, const u64c *hist, uint32_t levels,
                        size_t plane, TreeRec *out);

// lake statistics (ws_merge_tree_stats_device): per colour the weighted and plain first moments, the box,
// the extrema of the weight and the first pixel that holds the largest, over the pixels `area` counts.  Integers only.
struct LakeRec {      // == ws_lake_stats
  u64c sum_w, sum_wr, sum_wc, sum_r, sum_c;
  uint32_t r_min, r_max, c_min, c_max, w_min, w_max, peak_pixel, reserved;
};
// the weight plane: h x w elements of u8 or u16 (u16 != 0), `stride` elements a row; pixel (r, x) of it sits at (r + off, x + off)
// of the padded plane and every other pixel of that plane weighs 0.  A stack of slices (lake_stats_stack) reads slice k's plane
// slice_stride elements behind slice k - 1's (last, so that the single field's aggregate initialisers leave it 0).
struct LakeWeights {
  const void *p;
  size_t stride;
  uint32_t h, w, off;
  int u16;
  size_t slice_stride;
};
constexpr size_t LAKE_ACC_BYTES = 6 * sizeof(u64c) + 5 * sizeof(uint32_t);      // per colour: five sums and the packed peak, then the box and w_min
// After tree_init / tree_own_counts / tree_fold of the same transform (tree: finished records; ws, order: tree_fold's buckets, left
// as they are): own statistics in one pass over the stamps, the segmenting labels and the weights, one fold launch per death level
// from 1 up, and the records into out (n_colours of them).  acc: n_colours * LAKE_ACC_BYTES of scratch, 8-byte aligned.
hipError_t lake_stats(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, const TreeRec *tree,
                      const uint32_t *seeds_rc, size_t n_colours, uint32_t levels, const u64c *ws, const uint32_t *order, const LakeWeights &wt, int h,
                      int w, void *acc, LakeRec *out);
// The same over the forest of a stack (ws_merge_tree_stats_batch_device), after tree_init_stack / tree_own_counts_stack / tree_fold:
// `forest` in the forest's numbering (n_colours = the stack's seeds + 1), stacked_rc the stacked seed pairs (flood_stack: row =
// slice * slice rows + the row in the padded plane), w the plane's width.  Rows, columns and peak_pixel are those of a pixel within
// its own slice, its weight comes from its slice's plane, and an uncoloured pixel of slice k goes to accumulator entry n_colours + k:
// acc holds (n_colours + st.g) * LAKE_ACC_BYTES.  Writes the caller's slice-major layout: forest colour c at out[c + its slice],
// slice k's record 0 at out[base[k] + k] -- n_colours - 1 + st.g records.
hipError_t lake_stats_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                            const TreeRec *forest, const uint32_t *stacked_rc, size_t n_colours, uint32_t levels, const u64c *ws,
                            const uint32_t *order, const LakeWeights &wt, const TreeStack &st, int w, void *acc, LakeRec *out);

// lake shapes (ws_merge_tree_shapes_device): per colour six exact 128-bit sums -- v row^2, v col^2, v row col,
// row^2, col^2, row col -- over the pixels `area` counts, each as (low, high) 64 bits.  Integers only.
struct ShapeRec {      // == ws_lake_shape
  u64c s[6][2];
};
constexpr size_t SHAPE_ACC_BYTES = 12 * sizeof(u64c);      // per colour: two carry-less limbs a sum (ws_shape_part.hpp)
// After lake_stats' tree (tree: finished records; ws, order: tree_fold's buckets, left as they are; wt as lake_stats'): own sums in one
// pass over the stamps, the segmenting labels and the weights, one fold launch per death level from 1 up, and the records into out
// (n_colours of them, 8-byte aligned).  acc: n_colours * SHAPE_ACC_BYTES of scratch, 8-byte aligned.
hipError_t lake_shapes(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook, const TreeRec *tree,
                       const uint32_t *seeds_rc, size_t n_colours, uint32_t levels, const u64c *ws, const uint32_t *order, const LakeWeights &wt, int h,
                       int w, void *acc, ShapeRec *out);
// The same over the forest of a stack (ws_merge_tree_shapes_batch_device), after lake_stats_stack and with its arguments: rows and
// columns are those of a pixel within its own slice, its weight comes from its slice's plane, an uncoloured pixel of slice k goes to
// accumulator entry n_colours + k: acc holds (n_colours + st.g) * SHAPE_ACC_BYTES, cleared here.  The 96-bit bound of a sum is a
// slice's (every entry belongs to one slice), and so is the choice of the wave join: the sides of ONE slice, st.plane / w and w.
// Writes the caller's slice-major layout as lake_stats_stack does -- n_colours - 1 + st.g records, out 8-byte aligned.
hipError_t lake_shapes_stack(hipStream_t s, const uint32_t *keys, const uint32_t *labels, const uint32_t *death, const uint32_t *hook,
                             const TreeRec *forest, const uint32_t *stacked_rc, size_t n_colours, uint32_t levels, const u64c *ws,
                             const uint32_t *order, const LakeWeights &wt, const TreeStack &st, int w, void *acc, ShapeRec *out);

}  // namespace wsk
