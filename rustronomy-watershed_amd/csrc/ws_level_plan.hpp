// ws_level_plan.hpp -- the per-level driver's job and its plan: what merge_host (ws_lists.hip) is asked for, and what its
// level loop launches for it.
//
// Plain C++17, no HIP: level_job_refusal() and level_plan() are pure functions of the job and the context's threshold, and the
// one place where the mode of the level loop is decided.  merge_host asks them once and its stages do what the plan says;
// tests/cpp/test_level_plan.cpp runs both on a CPU against the table of modes written out as data.
#pragma once

#include "../../include/ws_hip.h"

#include <cstddef>
#include <cstdint>

namespace wsapi {

// Where the flood's stamps and labels come from.
enum class LevelSource {
  HOST,        // img, seeds_rc: staged and flooded here
  DEVICE,      // d_img, d_seeds_rc: already in HBM; lake records stay there too (d_lakes)
  ARRIVAL      // d_keys, d_seg: the segmenting transform has been run elsewhere -- its stamps and labels are all the per-level
               // paths read; no image, no seed list, h x w is the plane as it stands
};

// One run of the per-level driver.  Every member has a default: an entry point names what it sets.
struct LevelJob {
  bool merging = false;
  size_t h = 0, w = 0, stride = 0, n_seeds = 0;
  const ws_options *opt = nullptr;

  LevelSource source = LevelSource::HOST;
  const uint8_t *img = nullptr;                             // HOST
  const uint64_t *seeds_rc = nullptr;
  const uint8_t *d_img = nullptr;                           // DEVICE
  const uint32_t *d_seeds_rc = nullptr;
  const uint32_t *d_keys = nullptr, *d_seg = nullptr;       // ARRIVAL
  // ... of a stack of slices of slice_h rows whose labels restart at 1 in every slice: colour c of slice k is c + d_slice_base[k]
  // (ws_transform_to_list_batch_device)
  int slice_h = 0;
  const uint32_t *d_slice_base = nullptr;

  // the products
  ws_level_cb cb = nullptr;              // hook: every level's plane to the host, then cb(user, ...)
  void *user = nullptr;
  uint64_t *out_labels = nullptr;        // final labels, host
  // lists (n_lakes != null): (colour, area) records per level into `lakes` (host; HOST source) or `d_lakes` (the caller's device
  // buffer; DEVICE and ARRIVAL sources), cap of them; the per-level offsets and uncoloured counts always go to the host
  ws_lake *lakes = nullptr, *d_lakes = nullptr;
  size_t cap = 0;
  size_t *n_lakes = nullptr;
  uint64_t *offsets = nullptr, *uncoloured = nullptr;
  // history: no lists, no hook, no labels; merging: unions that stamp the merge forest (hook parents in uf_hook, death levels in
  // uf_death; the planes are rendered afterwards)
  bool history = false;

  bool lists() const { return n_lakes != nullptr; }
  bool device_records() const { return source != LevelSource::HOST; }

  // the three sources; what a job wants on top of its flood is named behind them (with_lists, with_history, cb, out_labels)
  static LevelJob plane(bool merging, LevelSource source, size_t h, size_t w, size_t stride, size_t n_seeds, const ws_options *opt) {
    LevelJob j;
    j.merging = merging; j.source = source; j.h = h; j.w = w; j.stride = stride; j.n_seeds = n_seeds; j.opt = opt;
    return j;
  }
  static LevelJob from_host(bool merging, const uint8_t *img, size_t h, size_t w, size_t stride, const uint64_t *seeds_rc, size_t n_seeds,
                            const ws_options *opt) {
    LevelJob j = plane(merging, LevelSource::HOST, h, w, stride, n_seeds, opt);
    j.img = img; j.seeds_rc = seeds_rc;
    return j;
  }
  static LevelJob from_device(bool merging, const uint8_t *d_img, size_t h, size_t w, size_t stride, const uint32_t *d_seeds_rc, size_t n_seeds,
                              const ws_options *opt) {
    LevelJob j = plane(merging, LevelSource::DEVICE, h, w, stride, n_seeds, opt);
    j.d_img = d_img; j.d_seeds_rc = d_seeds_rc;
    return j;
  }
  static LevelJob from_arrival(bool merging, const uint32_t *d_keys, const uint32_t *d_seg, size_t h, size_t w, size_t n_seeds, const ws_options *opt) {
    LevelJob j = plane(merging, LevelSource::ARRIVAL, h, w, w, n_seeds, opt);
    j.d_keys = d_keys; j.d_seg = d_seg;
    return j;
  }
  // records: on the source's side of the bus
  LevelJob with_lists(ws_lake *records, size_t cap_, size_t *n_lakes_, uint64_t *offsets_, uint64_t *uncoloured_) const {
    LevelJob j = *this;
    (j.device_records() ? j.d_lakes : j.lakes) = records;
    j.cap = cap_; j.n_lakes = n_lakes_; j.offsets = offsets_; j.uncoloured = uncoloured_;
    return j;
  }
  LevelJob with_history() const {
    LevelJob j = *this;
    j.history = true;
    return j;
  }
};

// A job that no entry point builds: what is wrong with it (null: nothing).
inline const char *level_job_refusal(const LevelJob &j) {
  if (j.history && (j.cb || j.lists() || j.out_labels)) return "internal: a history job with a hook, lists or labels";
  const bool host = j.img || j.seeds_rc, device = j.d_img || j.d_seeds_rc, arrival = j.d_keys || j.d_seg || j.slice_h || j.d_slice_base;
  if ((host && j.source != LevelSource::HOST) || (device && j.source != LevelSource::DEVICE) || (arrival && j.source != LevelSource::ARRIVAL))
    return "internal: a job with two sources";
  if ((j.n_lakes || j.offsets || j.uncoloured || j.lakes || j.d_lakes || j.cap) && !(j.n_lakes && j.offsets && j.uncoloured))
    return "internal: a lists job without n_lakes, offsets and uncoloured";
  if (j.device_records() ? j.lakes != nullptr : j.d_lakes != nullptr) return "internal: lake records on the other side of the bus from the source";
  return nullptr;
}

// The level loop's mode.
enum class LevelMode {
  NONE,            // segmenting history: the flood's stamps and labels are the result, nothing per level
  STAMPED,         // merging history: the unions stamp the merge forest; nothing else
  FUSED,           // merging lists without a hook: the records of level l - 1 ride in the launch that joins level l's edges
                   // (k_union_emit; ws_merge.hip) -- two launches per level instead of three; the last level's follow the loop
  FUSED_LIVE,      // ... with many colours: areas and death levels live side by side in uf_sd, level l - 1's records are found among
                   // level l - 2's LIVE lakes instead of by a look at every colour, and the arrivals of a level are added up per
                   // wave and workgroup before they reach a lake's counter
  PLAIN            // everything else: unions, areas, records and the hook as launches of their own
};

// One launch of a level, by its wrapper (ws_merge.hpp)
enum class LevelStep {
  UNION_STAMPED,         // union_stamped_ranged
  UNION_EMIT,            // union_emit
  UNION_EMIT_ALIVE,      // union_emit_alive (split: with no workgroups for the records ...
  EMIT_ALIVE_PREV,       // ... which emit_alive(l - 1) writes, from level 1 on)
  UNION_EDGES,           // union_edges_ranged: this level's crossing edges (lib.rs:1449-1466 in closed form)
  FOLD_ADD,              // fold_and_add_ranged: areas of the nodes hooked in this level move to their roots, arriving pixels are counted (lib.rs:628-635)
  FOLD_ADD_SD,           // fold_and_add_sd
  EMIT_LAKES,            // emit_lakes: the kernel leaves this level's record count in its counter
  HOOK                   // the level's plane rendered, copied to the host and handed to the caller's function
};

enum class LevelTail { NONE, EMIT_LAKES_DEATH, EMIT_ALIVE };      // the last level's records of the fused modes, with a marker behind them

constexpr int LEVEL_MAX_STEPS = 4;

struct LevelPlan {
  LevelMode mode = LevelMode::PLAIN;
  // the start state, behind uf_init
  bool ensure_hook = false;           // uf_hook
  bool ensure_live = false;           // uf_sd and alive
  bool death_all_ones = false;        // uf_death set to 0xFF: every colour a root
  bool sd_init = false;               // uf_sd: no pixels yet, every colour a root
  // every level, in order
  LevelStep steps[LEVEL_MAX_STEPS] = {};
  int n_steps = 0;
  // PLAIN: the unions note the nodes they hook and the fold moves those nodes' areas (merging lists; the fused modes always do).
  // Unions without lists have nobody to note them for; lists without unions hook nothing.
  bool hooked_list = false;
  bool split_emit = false;            // FUSED_LIVE under WS_TOLIST_SPLIT: UNION_EMIT_ALIVE gets no workgroups for the records
  LevelTail tail = LevelTail::NONE;
  // the marker a group's record copy waits for: its own group's (0) or the next one's (1: in the fused modes a group's last level
  // is complete one launch later)
  uint32_t marker_shift = 0;
  void add(LevelStep s) { steps[n_steps++] = s; }
};

// live_list_min: fewest seeds for which merging lists are written from the live-lake list (ws_ctx_set_live_list_min_colours).
// Planes with a million colours and more (4096^2 random fields on) write their lake records from the list of the lakes
// still alive, not from a look at every colour at every level (8192^2: 66.8 -> 20.5 ms); below that the per-level
// launches are latency-bound either way and the older, shorter kernels win (1024^2, the core_bench shape: 3.8 against 5.0 ms).
// split_emit (WS_TOLIST_SPLIT, an A/B knob for tools/): FUSED_LIVE's two jobs as launches of their own.
inline LevelPlan level_plan(const LevelJob &j, size_t live_list_min, bool split_emit = false) {
  LevelPlan p;
  const bool lists = j.lists(), hook = j.cb != nullptr;
  if (j.history) p.mode = j.merging ? LevelMode::STAMPED : LevelMode::NONE;
  else if (j.merging && lists && !hook) p.mode = j.n_seeds >= live_list_min ? LevelMode::FUSED_LIVE : LevelMode::FUSED;
  switch (p.mode) {
    case LevelMode::NONE:
      break;
    case LevelMode::STAMPED:
      p.ensure_hook = p.death_all_ones = true;
      p.add(LevelStep::UNION_STAMPED);
      break;
    case LevelMode::FUSED:
      p.death_all_ones = p.hooked_list = true;
      p.add(LevelStep::UNION_EMIT);
      p.add(LevelStep::FOLD_ADD);
      p.tail = LevelTail::EMIT_LAKES_DEATH;
      p.marker_shift = 1;
      break;
    case LevelMode::FUSED_LIVE:
      p.ensure_live = p.sd_init = p.hooked_list = true;
      p.add(LevelStep::UNION_EMIT_ALIVE);
      p.split_emit = split_emit;
      if (split_emit) p.add(LevelStep::EMIT_ALIVE_PREV);
      p.add(LevelStep::FOLD_ADD_SD);
      p.tail = LevelTail::EMIT_ALIVE;
      p.marker_shift = 1;
      break;
    case LevelMode::PLAIN:
      p.hooked_list = j.merging && lists;
      if (j.merging) p.add(LevelStep::UNION_EDGES);
      if (lists) p.add(LevelStep::FOLD_ADD);
      if (lists) p.add(LevelStep::EMIT_LAKES);
      if (hook) p.add(LevelStep::HOOK);
      break;
  }
  return p;
}

// May the level loop be captured and replayed as graphs?  It has no host decision in it unless a hook is called.
inline bool level_capturable(const LevelJob &j, bool has_stream, bool graph_unusable, bool profiling, size_t n) {
  return !j.cb && has_stream && !graph_unusable && !profiling && n != 0;
}

}  // namespace wsapi
