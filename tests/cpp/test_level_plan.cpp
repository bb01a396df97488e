// The per-level driver's job and plan (csrc/ws_level_plan.hpp) on a CPU.
//   a. level_plan() over every combination of merging, lists, hook and history, with n_seeds just below, at and just above the
//      live-list threshold for thresholds of 0 and 2^20: mode, start state, the launches of a level in order, the tail and the
//      marker shift, against the table of modes written out below as data;
//   b. level_capturable() over all its inputs;
//   c. level_job_refusal(): the jobs the entry points build pass, the combinations nobody builds are refused.
#include "../../rustronomy-watershed_amd/csrc/ws_level_plan.hpp"

#include <cstdio>
#include <cstring>
#include <string>

using namespace wsapi;

namespace {

int failures = 0;
#define CHECK(cond, ...)                                                     \
  do {                                                                       \
    if (!(cond)) {                                                           \
      ++failures;                                                            \
      std::printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond);            \
      std::printf(__VA_ARGS__);                                              \
      std::printf("\n");                                                     \
    }                                                                        \
  } while (0)

const char *step_name(LevelStep s) {
  switch (s) {
    case LevelStep::UNION_STAMPED: return "union_stamped_ranged";
    case LevelStep::UNION_EMIT: return "union_emit";
    case LevelStep::UNION_EMIT_ALIVE: return "union_emit_alive";
    case LevelStep::EMIT_ALIVE_PREV: return "emit_alive(l-1)";
    case LevelStep::UNION_EDGES: return "union_edges_ranged";
    case LevelStep::FOLD_ADD: return "fold_and_add_ranged";
    case LevelStep::FOLD_ADD_SD: return "fold_and_add_sd";
    case LevelStep::EMIT_LAKES: return "emit_lakes";
    case LevelStep::HOOK: return "hook";
  }
  return "?";
}

std::string steps_of(const LevelPlan &p) {
  std::string s;
  for (int i = 0; i < p.n_steps; ++i) s += (i ? " " : "") + std::string(step_name(p.steps[i]));
  return s;
}

std::string start_of(const LevelPlan &p) {
  std::string s;
  if (p.ensure_hook) s += "uf_hook ";
  if (p.ensure_live) s += "uf_sd alive ";
  if (p.death_all_ones) s += "death=0xFF ";
  if (p.sd_init) s += "sd_init ";
  if (!s.empty()) s.pop_back();
  return s;
}

// The table of modes.  -1: any.  live: n_seeds >= live_list_min.  Every combination must match exactly one row.
struct Row {
  int history, merging, lists, hook, live;
  LevelMode mode;
  const char *start, *steps;      // start state; the launches of a level, in order
  bool hooked;                    // the unions note what they hook and the fold moves those areas
  LevelTail tail;
  uint32_t shift;                 // the group copy waits for the marker of group g + shift
};
const Row TABLE[] = {
    // history: nothing per level when segmenting, the stamping unions when merging
    {1, 0, -1, -1, -1, LevelMode::NONE, "", "", false, LevelTail::NONE, 0},
    {1, 1, -1, -1, -1, LevelMode::STAMPED, "uf_hook death=0xFF", "union_stamped_ranged", false, LevelTail::NONE, 0},
    // merging lists without a hook: the fused modes
    {0, 1, 1, 0, 0, LevelMode::FUSED, "death=0xFF", "union_emit fold_and_add_ranged", true, LevelTail::EMIT_LAKES_DEATH, 1},
    {0, 1, 1, 0, 1, LevelMode::FUSED_LIVE, "uf_sd alive sd_init", "union_emit_alive fold_and_add_sd", true, LevelTail::EMIT_ALIVE, 1},
    // everything else: plain.  union_edges_ranged if merging (hooked only when lists are wanted), fold_and_add_ranged if lists
    // (hooked only when merging), emit_lakes if lists, the hook if there is one
    {0, 0, 0, 0, -1, LevelMode::PLAIN, "", "", false, LevelTail::NONE, 0},
    {0, 0, 0, 1, -1, LevelMode::PLAIN, "", "hook", false, LevelTail::NONE, 0},
    {0, 0, 1, 0, -1, LevelMode::PLAIN, "", "fold_and_add_ranged emit_lakes", false, LevelTail::NONE, 0},
    {0, 0, 1, 1, -1, LevelMode::PLAIN, "", "fold_and_add_ranged emit_lakes hook", false, LevelTail::NONE, 0},
    {0, 1, 0, 0, -1, LevelMode::PLAIN, "", "union_edges_ranged", false, LevelTail::NONE, 0},
    {0, 1, 0, 1, -1, LevelMode::PLAIN, "", "union_edges_ranged hook", false, LevelTail::NONE, 0},
    {0, 1, 1, 1, -1, LevelMode::PLAIN, "", "union_edges_ranged fold_and_add_ranged emit_lakes hook", true, LevelTail::NONE, 0},
};

void a_hook(void *, uint8_t, uint8_t, const uint8_t *, const uint64_t *, size_t, size_t) {}

size_t n_lakes_word;
uint64_t words[4];
ws_lake lake_recs[1];

LevelJob job_of(bool merging, bool lists, bool hook, bool history, size_t n_seeds) {
  LevelJob j;
  j.merging = merging;
  j.n_seeds = n_seeds;
  j.history = history;
  if (lists) { j.n_lakes = &n_lakes_word; j.offsets = words; j.uncoloured = words + 2; j.cap = 1; j.lakes = lake_recs; }
  if (hook) j.cb = a_hook;
  return j;
}

void test_plan_table() {
  const size_t mins[] = {0, (size_t)1 << 20};
  int combos = 0;
  for (size_t live_min : mins)
    for (int d = -1; d <= 1; ++d)
      for (int bits = 0; bits < 16; ++bits) {
        const bool merging = bits & 1, lists = bits & 2, hook = bits & 4, history = bits & 8;
        const size_t n_seeds = live_min + (size_t)d;      // (threshold 0, d = -1: the largest size_t, above every threshold)
        const bool live = n_seeds >= live_min;
        const LevelJob j = job_of(merging, lists, hook, history, n_seeds);
        const Row *row = nullptr;
        int matches = 0;
        for (const Row &r : TABLE) {
          const auto m = [](int want, bool got) { return want < 0 || (want != 0) == got; };
          if (m(r.history, history) && m(r.merging, merging) && m(r.lists, lists) && m(r.hook, hook) && m(r.live, live)) { row = &r; ++matches; }
        }
        CHECK(matches == 1, "bits %d live %d: %d rows", bits, (int)live, matches);
        if (matches != 1) continue;
        for (int split = 0; split < 2; ++split) {
          const LevelPlan p = level_plan(j, live_min, split != 0);
          std::string steps = row->steps;
          if (split && row->mode == LevelMode::FUSED_LIVE) steps = "union_emit_alive emit_alive(l-1) fold_and_add_sd";      // WS_TOLIST_SPLIT
          CHECK(p.mode == row->mode, "bits %d n_seeds %zu min %zu: mode %d, want %d", bits, n_seeds, live_min, (int)p.mode, (int)row->mode);
          CHECK(start_of(p) == row->start, "bits %d: start '%s', want '%s'", bits, start_of(p).c_str(), row->start);
          CHECK(steps_of(p) == steps, "bits %d: steps '%s', want '%s'", bits, steps_of(p).c_str(), steps.c_str());
          CHECK(p.hooked_list == row->hooked, "bits %d: hooked %d", bits, (int)p.hooked_list);
          CHECK(p.tail == row->tail, "bits %d: tail %d, want %d", bits, (int)p.tail, (int)row->tail);
          CHECK(p.marker_shift == row->shift, "bits %d: marker shift %u, want %u", bits, p.marker_shift, row->shift);
          CHECK(p.split_emit == (split && row->mode == LevelMode::FUSED_LIVE), "bits %d: split_emit %d", bits, (int)p.split_emit);
          CHECK(p.n_steps <= LEVEL_MAX_STEPS, "bits %d: %d steps", bits, p.n_steps);
          // a marker behind the tail exists exactly when the group copies wait for the next group's
          CHECK((p.tail != LevelTail::NONE) == (p.marker_shift == 1), "bits %d: tail and marker shift disagree", bits);
        }
        // the job check: history with a hook or lists is refused, everything else of this enumeration passes
        const char *why = level_job_refusal(j);
        CHECK((why != nullptr) == (history && (hook || lists)), "bits %d: refusal '%s'", bits, why ? why : "(none)");
        if (why) CHECK(std::strncmp(why, "internal: ", 10) == 0, "'%s'", why);
        ++combos;
      }
  CHECK(combos == 2 * 3 * 16, "%d combinations", combos);
}

void test_capturable() {
  for (int bits = 0; bits < 32; ++bits) {
    const bool hook = bits & 1, stream = bits & 2, unusable = bits & 4, profiling = bits & 8;
    const size_t n = bits & 16 ? 3072 : 0;
    for (int lists = 0; lists < 2; ++lists) {
      const LevelJob j = job_of(true, lists != 0, hook, false, 7);
      const bool want = !hook && stream && !unusable && !profiling && n != 0;
      CHECK(level_capturable(j, stream, unusable, profiling, n) == want, "bits %d", bits);
    }
  }
}

bool refused(const LevelJob &j, const char *needle) {
  const char *why = level_job_refusal(j);
  return why && std::strncmp(why, "internal: ", 10) == 0 && std::strstr(why, needle);
}

void test_job_check() {
  static const uint8_t px[4] = {};
  static const uint64_t seeds64[2] = {};
  static const uint32_t words32[4] = {};
  static ws_options opt{};
  // what the entry points build
  const LevelJob host = LevelJob::from_host(true, px, 2, 2, 2, seeds64, 1, &opt);
  const LevelJob dev = LevelJob::from_device(false, px, 2, 2, 2, words32, 1, &opt);
  const LevelJob arr = LevelJob::from_arrival(false, words32, words32, 2, 2, 1, &opt);
  CHECK(host.source == LevelSource::HOST && dev.source == LevelSource::DEVICE && arr.source == LevelSource::ARRIVAL && arr.stride == 2, "the named sources");
  const auto with_lists = [](const LevelJob &j) { return j.with_lists(lake_recs, 1, &n_lakes_word, words, words + 2); };
  const auto with_history = [](const LevelJob &j) { return j.with_history(); };
  CHECK(with_lists(host).lakes == lake_recs && !with_lists(host).d_lakes && with_lists(dev).d_lakes == lake_recs && !with_lists(dev).lakes,
        "records on the source's side of the bus");
  LevelJob hooked = host;
  hooked.cb = a_hook; hooked.out_labels = words;
  LevelJob stack = arr;
  stack.slice_h = 1; stack.d_slice_base = words32;
  LevelJob empty_dev;      // an empty image, device form: no pointer at all
  empty_dev.source = LevelSource::DEVICE; empty_dev.opt = &opt;
  const LevelJob good[] = {with_history(host), with_history(dev), with_history(stack), with_history(empty_dev), with_lists(host), with_lists(dev),
                           with_lists(arr), with_lists(stack), with_lists(empty_dev), hooked};
  for (const LevelJob &j : good) CHECK(level_job_refusal(j) == nullptr, "'%s'", level_job_refusal(j));
  {      // lists that are counted only (cap 0, no record buffer) pass too
    LevelJob j = with_lists(dev);
    j.d_lakes = nullptr; j.cap = 0;
    CHECK(level_job_refusal(j) == nullptr, "'%s'", level_job_refusal(j));
  }

  // history together with a hook, lists or labels
  { LevelJob j = with_history(host); j.cb = a_hook; CHECK(refused(j, "history"), "history + hook"); }
  { LevelJob j = with_history(host); j.out_labels = words; CHECK(refused(j, "history"), "history + labels"); }
  CHECK(refused(with_history(with_lists(host)), "history"), "history + lists, host");
  CHECK(refused(with_history(with_lists(dev)), "history"), "history + lists, device");
  CHECK(refused(with_history(with_lists(stack)), "history"), "history + lists, stack");

  // two sources at once: a member of another source than the one named
  { LevelJob j = host; j.d_img = px; CHECK(refused(j, "two sources"), "host + d_img"); }
  { LevelJob j = host; j.d_seeds_rc = words32; CHECK(refused(j, "two sources"), "host + d_seeds_rc"); }
  { LevelJob j = host; j.d_keys = words32; CHECK(refused(j, "two sources"), "host + d_keys"); }
  { LevelJob j = dev; j.img = px; CHECK(refused(j, "two sources"), "device + img"); }
  { LevelJob j = dev; j.seeds_rc = seeds64; CHECK(refused(j, "two sources"), "device + seeds_rc"); }
  { LevelJob j = dev; j.d_seg = words32; CHECK(refused(j, "two sources"), "device + d_seg"); }
  { LevelJob j = dev; j.slice_h = 4; CHECK(refused(j, "two sources"), "device + slice_h"); }
  { LevelJob j = dev; j.d_slice_base = words32; CHECK(refused(j, "two sources"), "device + d_slice_base"); }
  { LevelJob j = arr; j.d_img = px; CHECK(refused(j, "two sources"), "arrival + d_img"); }
  { LevelJob j = arr; j.img = px; CHECK(refused(j, "two sources"), "arrival + img"); }
  { LevelJob j = dev; j.source = LevelSource::HOST; CHECK(refused(j, "two sources"), "device members, host named"); }

  // lists without all three of n_lakes, offsets and uncoloured
  for (int bits = 0; bits < 7; ++bits)
    for (const LevelJob &base : {host, dev, arr}) {
      LevelJob j = with_lists(base);
      if (!(bits & 1)) j.n_lakes = nullptr;
      if (!(bits & 2)) j.offsets = nullptr;
      if (!(bits & 4)) j.uncoloured = nullptr;
      CHECK(refused(j, "without n_lakes, offsets and uncoloured"), "lists with outputs %d", bits);
    }
  { LevelJob j = host; j.cap = 5; CHECK(refused(j, "without n_lakes"), "a cap and no lists"); }
  // ... and records on the wrong side of the bus
  { LevelJob j = with_lists(host); j.lakes = nullptr; j.d_lakes = lake_recs; CHECK(refused(j, "other side"), "host + d_lakes"); }
  { LevelJob j = with_lists(dev); j.d_lakes = nullptr; j.lakes = lake_recs; CHECK(refused(j, "other side"), "device + lakes"); }
}

}  // namespace

int main() {
  test_plan_table();
  test_capturable();
  test_job_check();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("level plan ok\n");
  return 0;
}
