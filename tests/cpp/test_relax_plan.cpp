// The relaxation's schedule (csrc/ws_relax_plan.hpp) on a CPU.
//   a. relax_plan() against tests/relax_plan_cases.txt: what relax_pass launched, kernel by kernel and argument by argument,
//      at the commit before the schedule was split out of it -- the plan of every (plane, pass) of the table, printed as
//      that commit's launches were, must be that line;
//   b. what consecutive passes of one transform have to agree on, for every plane of the table over passes 0 .. 11.
// usage: test_relax_plan tests/relax_plan_cases.txt
#include "../../rustronomy-watershed_amd/csrc/ws_relax_plan.hpp"

#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <string>
#include <vector>

using namespace wsk;

namespace {

struct Case {
  std::string label;
  RelaxGeom g;
  RelaxKnobs k;
  size_t stride = 0;
};

bool parse(const std::string &label, Case &c) {
  int seeds = 0, align = 0, list = 0, pad = 0;
  unsigned mi = 0;
  char knobs[200];
  if (sscanf(label.c_str(), "w=%d h=%d slice=%d pad=%d seeds=%d smp=%zu align=%d stride=%zu list=%d pm=%d mi=%u knobs=%199s", &c.g.w, &c.g.h, &c.g.slice_h, &pad,
             &seeds, &c.g.seam_min_px, &align, &c.stride, &list, &c.g.persist_mode, &mi, knobs) != 12)
    return false;
  c.label = label;
  c.g.padded = pad != 0;
  c.g.has_seeds = seeds != 0;
  c.g.seed_bits = seeds == 1;
  c.g.aligned4 = align != 0 && (c.stride & 3) == 0;
  c.g.stride32 = c.stride <= 0xFFFFFFFFull;
  c.g.has_list = list != 0;
  c.g.max_iters = mi;
  const std::string kn = knobs;
  if (kn == "-") return true;
  if (kn == "seam_band:4") c.k.seam_band = 4;
  else if (kn == "seam_band:8") c.k.seam_band = 8;
  else if (kn == "no_tall") c.k.no_tall = true;
  else if (kn == "no_tall_strips") c.k.no_tall_strips = true;
  else if (kn == "no_split") c.k.no_split = true;
  else if (kn == "no_append") c.k.no_append = true;
  else if (kn == "queue_from:5") c.k.queue_from = 5;
  else return false;
  return true;
}

// The tile list's layout (ws_relax.hip: RL_HDR, PQ_HDR, PQ_B, pq_base, pq_words_per_bucket), for the sizes of the queue's clears.
constexpr size_t RL_HDR = 192, PQ_HDR = 32, PQ_B = 31;
size_t pq_base(size_t cap) { return (RL_HDR + 3 * cap + 64 + 31) & ~(size_t)31; }
size_t pq_words_per_bucket(size_t tiles) { return ((tiles + 31) / 32 + 255) & ~(size_t)255; }

std::string num(long long v) { return std::to_string(v); }
std::string join(const std::vector<std::string> &v) {
  std::string s;
  for (size_t i = 0; i < v.size(); ++i) s += (i ? "," : "") + v[i];
  return s;
}

bool is_relax(RelaxStep::Kind k) {      // an instantiation of k_relax
  switch (k) {
    case RelaxStep::BANDS: case RelaxStep::STRIPS: case RelaxStep::FULL: case RelaxStep::FULL_LITE: case RelaxStep::CHUNKED: case RelaxStep::CHUNKED_SCAN:
    case RelaxStep::LISTED: case RelaxStep::LISTED_SPLIT: case RelaxStep::QUEUE_FIRST_COME: case RelaxStep::QUEUE_FLOOD_ORDER: return true;
    default: return false;
  }
}
bool is_queue(RelaxStep::Kind k) { return k == RelaxStep::QUEUE_FIRST_COME || k == RelaxStep::QUEUE_FLOOD_ORDER; }
bool is_list_build(RelaxStep::Kind k) { return k == RelaxStep::LIST_BUILD || k == RelaxStep::LIST_BUILD_SPLIT || k == RelaxStep::LIST_REGRID; }
bool is_clear(RelaxStep::Kind k) { return k == RelaxStep::CLEAR_RING || k == RelaxStep::CLEAR_COUNTERS || k == RelaxStep::CLEAR_BUCKETS; }
// the launches that run tiles: what launches_relax counts
bool runs_tiles(RelaxStep::Kind k) { return is_relax(k) || k == RelaxStep::TALL_PASS0 || k == RelaxStep::STRIPS_TALL; }

// A step as the launch it stands for, in the table's spelling.
std::string spell(const Case &c, const RelaxStep &st) {
  const RelaxGeom &g = c.g;
  const std::string h = num(g.h), w = num(g.w), sh = num(g.slice_h > 0 ? g.slice_h : g.h), pad = num(g.padded ? 1 : 0), list = g.has_list ? "p" : "0";
  const size_t cap = relax_plan_tiles(g.h, g.w);
  const std::string at = "[" + num(st.grid) + "," + num(st.block) + "]";
  const std::string seeds = st.seeds && g.has_seeds ? "p" : "0", bits = num(st.seeds && g.has_seeds && g.seed_bits ? 1 : 0);
  if (is_relax(st.kind)) {
    std::vector<long> t;
    switch (st.kind) {
      case RelaxStep::BANDS: t = {st.nw, 0, 0, 0, 0, 1, 0, st.seam_pitch}; break;
      case RelaxStep::STRIPS: t = {RX_NW, 0, 0, 0, 0, 2, 0, 32}; break;
      case RelaxStep::FULL: t = {RX_NW, 0, 0, 0, 0, 0, 0, 32}; break;
      case RelaxStep::FULL_LITE: t = {RX_NW, 0, 0, 1, 0, 0, 0, 32}; break;
      case RelaxStep::CHUNKED: t = {RX_NW, 1, 0, 1, 0, 0, 0, 32}; break;
      case RelaxStep::CHUNKED_SCAN: case RelaxStep::LISTED: t = {RX_NW, 1, 1, 1, 0, 0, 0, 32}; break;
      case RelaxStep::LISTED_SPLIT: t = {RX_SNW, 1, 1, 1, 1, 0, 0, 32}; break;
      case RelaxStep::QUEUE_FIRST_COME: t = {RX_SNW, 1, 1, 1, 1, 0, 1, 32}; break;
      default: t = {RX_QNW, 1, 1, 1, 1, 0, 2, 32}; break;
    }
    std::vector<std::string> ts;
    for (long v : t) ts.push_back(num(v));
    return "k_relax<" + join(ts) + ">" + at + "(" +
           join({"p", num((long long)c.stride), "p", h, w, num(st.tilesX), num(st.tilesY), num(st.otherX), num(st.otherY), num(st.shifted), num(st.chunk), "254",
                 num(st.pass), "p", "p", "pf", num(st.max_iters), seeds, bits, sh, "1", pad, list, num(st.use_list), num(st.read_same), num(st.write_same),
                 num((long long)cap), num(st.append_next)}) + ")";
  }
  const std::string stride32 = num((long long)(uint32_t)c.stride);
  switch (st.kind) {
    case RelaxStep::TALL_PASS0:
      return "k_relax0_tall" + at + "(" + join({"p", stride32, "p", h, w, num(st.tilesX), num(st.tilesX), num(st.otherX), "254", "p", "p", "pf", num(st.max_iters),
                                               g.has_seeds ? "p" : "0", sh, "1", list}) + ")";
    case RelaxStep::STRIPS_TALL:
      return "k_relax_strips_tall" + at + "(" + join({"p", stride32, "p", h, w, num(st.tilesX), num(st.otherX), "254", num(st.pass), "p", "pf", num(st.max_iters), sh, "1", list}) + ")";
    case RelaxStep::LIST_BUILD: case RelaxStep::LIST_BUILD_SPLIT:
      return std::string("k_relax_list<") + (st.kind == RelaxStep::LIST_BUILD ? num(RX_TW) + "," + num(RX_NW * RX_P) : num(RX_STW) + "," + num(RX_STH)) + ">" + at + "(" +
             join({h, w, num(st.tilesX), num(st.tilesY), num(st.otherX), num(st.otherY), num(st.shifted), num(st.pass), "p", list, num(st.read_same), num((long long)cap)}) + ")";
    case RelaxStep::LIST_REGRID:
      return "k_relax_list_regrid<" + join({num(RX_STW), num(st.regrid == 2 ? RX_QTH : RX_STH), num(RX_TW), num(RX_NW * RX_P)}) + ">" + at + "(" +
             join({h, w, num(st.tilesX), num(st.tilesY), num(st.otherX), num(st.otherY), num(st.pass), "p", list, num((long long)cap), num(st.regrid)}) + ")";
    case RelaxStep::LIST_ALL:
      return "k_relax_list_all<" + num(RX_STW) + "," + num(RX_STH) + ">" + at + "(" + join({h, w, num(st.tilesX), num(st.tilesY), num(st.pass), list, num((long long)cap)}) + ")";
    case RelaxStep::CLEAR_RING: return "memset(list+" + num(RL_HDR) + ",0," + num((long long)(2 * cap * 4)) + ")";
    case RelaxStep::CLEAR_COUNTERS: return "memset(list+8,0," + num((RL_HDR - 8) * 4) + ")";
    case RelaxStep::CLEAR_BUCKETS: return "memset(list+" + num((long long)pq_base(cap)) + ",0," + num((long long)((PQ_HDR + PQ_B * pq_words_per_bucket(cap)) * 4)) + ")";
    default: return "?";
  }
}

int failures = 0;
void fail(const Case &c, uint32_t pass, const std::string &what) {
  if (++failures <= 20) std::cerr << "FAIL " << c.label << " pass " << pass << ": " << what << "\n";
}

// b. What the passes of one transform must agree on.
void check_invariants(const Case &c) {
  constexpr uint32_t PASSES = 12;
  RelaxPlan plan[PASSES];
  for (uint32_t p = 0; p < PASSES; ++p) plan[p] = relax_plan(c.g, p, c.k);
  const int ax = (c.g.w + RX_TW - 1) / RX_TW, ay = (c.g.h + RX_NW * RX_P - 1) / (RX_NW * RX_P);
  auto has = [](const RelaxPlan &pl, auto pred) {
    for (int i = 0; i < pl.n; ++i)
      if (pred(pl.steps[i])) return true;
    return false;
  };
  // the step whose read_same / write_same / tiles stand for the pass: the last launch that runs tiles
  auto main_step = [](const RelaxPlan &pl) -> const RelaxStep & {
    int m = 0;
    for (int i = 0; i < pl.n; ++i)
      if (runs_tiles(pl.steps[i].kind)) m = i;
    return pl.steps[m];
  };
  if (plan[0].tall0 != plan[1].tall0) fail(c, 0, "passes 0 and 1 disagree on tall0");
  const bool tall_ran = plan[0].n == 1 && plan[0].steps[0].kind == RelaxStep::TALL_PASS0;
  const bool bands64 = has(plan[1], [](const RelaxStep &s) { return s.kind == RelaxStep::BANDS && s.seam_pitch == RX0_TH; });
  if (tall_ran != bands64) fail(c, 1, "bands of pitch 64 without the tall pass 0, or the reverse");
  for (uint32_t p = 0; p < PASSES; ++p) {
    const RelaxPlan &pl = plan[p];
    if (pl.n < 1 || pl.n > RELAX_MAX_STEPS) { fail(c, p, "step count"); continue; }
    if (pl.seam_flow != plan[0].seam_flow || pl.tall0 != plan[0].tall0) fail(c, p, "the flags change between passes");
    const bool seam_pass = has(pl, [](const RelaxStep &s) { return s.kind == RelaxStep::BANDS; });
    if (seam_pass != (pl.seam_flow && p == 1)) fail(c, p, "bands outside pass 1 of the seam flow");
    int tile_launches = 0;
    for (int i = 0; i < pl.n; ++i) {
      const RelaxStep &s = pl.steps[i];
      if (runs_tiles(s.kind)) ++tile_launches;
      if (is_clear(s.kind)) continue;
      if (s.grid < 1) fail(c, p, "empty grid");
      if (s.block % 64 != 0 || s.block < 64 || s.block > 1024) fail(c, p, "block is not 64 x NW <= 1024");
      if (runs_tiles(s.kind) && s.max_iters < 1 && c.g.max_iters != 0) fail(c, p, "no rounds");
      if (is_queue(s.kind)) {
        const bool followed = i + 1 < pl.n && pl.steps[i + 1].kind == RelaxStep::LIST_ALL && pl.steps[i + 1].pass == p + 1 && i + 2 == pl.n;
        if (!followed) fail(c, p, "queue step without list-all for the next pass behind it");
      }
    }
    // launches_relax (run_fused_form) counts passes + 1 in the seam flow
    if (tile_launches != (seam_pass ? 2 : 1)) fail(c, p, "launches that run tiles: " + num(tile_launches));
    if (p == 0) continue;
    const RelaxPlan &before = plan[p - 1];
    const RelaxStep &m = main_step(pl), &mb = main_step(before);
    if (m.read_same != mb.write_same) fail(c, p, "read_same differs from the write_same of the pass before");
    const bool before_seam = has(before, [](const RelaxStep &s) { return s.kind == RelaxStep::BANDS; });
    // Who reads the flags of the pass before: the list build of this pass, or its tiles themselves when they run without a list.
    const RelaxStep *reader = nullptr;
    for (int i = 0; i < pl.n && !reader; ++i)
      if (is_list_build(pl.steps[i].kind)) reader = &pl.steps[i];
    if (!reader && m.use_list == 0 && !seam_pass) reader = &m;
    if (reader) {
      // (bands and strips raise their flags in the shifted grid's words -- one more tile row and column than the anchored grid,
      // their own otherX / otherY -- whatever tiles they run on themselves)
      const int wx = before_seam ? ax + 1 : mb.tilesX, wy = before_seam ? ay + 1 : mb.tilesY;
      if (before_seam && (mb.otherX != wx || mb.otherY != wy)) fail(c, p, "the seam pass does not flag the shifted grid");
      if (reader->otherX != wx || reader->otherY != wy) fail(c, p, "reads the flags of a grid that the pass before did not write");
    } else if (!seam_pass) {
      // tiles from a list that no step of this pass builds: the pass before left it
      const bool left = mb.append_next != 0 || before.steps[before.n - 1].kind == RelaxStep::LIST_ALL;
      if (!left) fail(c, p, "a listed step without a list");
    }
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) { std::cerr << "cannot read " << argv[1] << "\n"; return 2; }
  std::string line, last_label;
  size_t lines = 0, planes = 0;
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    const size_t at = line.find(" pass="), colon = line.find(" : ");
    if (at == std::string::npos || colon == std::string::npos) { std::cerr << "bad line: " << line << "\n"; return 2; }
    Case c;
    if (!parse(line.substr(0, at), c)) { std::cerr << "bad label: " << line << "\n"; return 2; }
    const uint32_t pass = (uint32_t)std::stoul(line.substr(at + 6, colon - at - 6));
    const RelaxPlan plan = relax_plan(c.g, pass, c.k);
    std::string mine;
    for (int i = 0; i < plan.n; ++i) mine += (i ? " ; " : "") + spell(c, plan.steps[i]);
    ++lines;
    if (mine != line.substr(colon + 3)) fail(c, pass, "the plan is\n  " + mine + "\nthe table has\n  " + line.substr(colon + 3));
    if (c.label != last_label) { check_invariants(c); last_label = c.label; ++planes; }
  }
  if (lines < 300 || failures) { std::cerr << failures << " failures, " << lines << " lines\n"; return 1; }
  std::cout << "relax plan ok: " << lines << " lines, " << planes << " planes\n";
  return 0;
}
