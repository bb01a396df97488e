// ws_watershed.hpp -- header-only C++ mirror of the reference's public interface for the
// watershed path, over the C ABI in ws_hip.h.
//
// The reference (smups/rustronomy-watershed v0.4.1) is Rust and this image has no Rust
// toolchain, so the host side above the C ABI is written in C++ with the reference's own
// names, argument meaning and error behaviour ("lib.rs:N" = src/lib.rs line N):
//
//   TransformBuilder<T>      lib.rs:908-1047      BuildErr               lib.rs:1051-1065
//   HookCtx                  lib.rs:844-862       WatershedUtils         lib.rs:1069-1198
//   Watershed<T> (4 methods) lib.rs:1206-1238     Segmenting/MergingWatershed  lib.rs:1297-1849
//
// Rust panics (out-of-bounds seed, lib.rs:1366/1676) surface as std::out_of_range; Result<_,
// BuildErr> as a thrown BuildErr.  Documented deviations from the reference: see ws_hip.h.
#pragma once

#include <algorithm>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ws_hip.h"

namespace rustronomy_watershed {

constexpr std::size_t UNCOLOURED = 0;      // lib.rs:138
constexpr std::uint8_t NORMAL_MAX = 254;   // lib.rs:139
constexpr std::uint8_t ALWAYS_FILL = 0;    // lib.rs:140
constexpr std::uint8_t NEVER_FILL = 255;   // lib.rs:141

using usize = std::uint64_t;
using Seed = std::pair<usize, usize>;      // (row, col)

struct BuildErr : std::runtime_error {     // lib.rs:1051-1065
  enum Kind { MaxToHigh, MaxToLow } kind;
  std::uint8_t value;
  BuildErr(Kind k, std::uint8_t v)
      : std::runtime_error(k == MaxToHigh
                               ? "Maximum water level set to " + std::to_string(v) + ", which is higher than the maximum allowed value 254"
                               : "Maximum water level set to " + std::to_string(v) + ", which is lower than the minimum allowed value 255"),
        kind(k), value(v) {}
};

struct WatershedError : std::runtime_error {
  int status;
  WatershedError(int s, const std::string &detail) : std::runtime_error(std::string(ws_strerror(s)) + ": " + detail), status(s) {}
};

template <class T>
struct Array2 {                            // owned, standard layout (ndarray::Array2<T>)
  std::size_t rows = 0, cols = 0;
  std::vector<T> data;
  Array2() = default;
  Array2(std::size_t r, std::size_t c) : rows(r), cols(c), data(r * c) {}
  T &operator()(std::size_t r, std::size_t c) { return data[r * cols + c]; }
  const T &operator()(std::size_t r, std::size_t c) const { return data[r * cols + c]; }
};

template <class T>
struct ArrayView2 {                        // borrowed view with a row stride in elements
  const T *ptr = nullptr;
  std::size_t rows = 0, cols = 0, row_stride = 0;
  ArrayView2() = default;
  ArrayView2(const T *p, std::size_t r, std::size_t c, std::size_t s) : ptr(p), rows(r), cols(c), row_stride(s) {}
  ArrayView2(const Array2<T> &a) : ptr(a.data.data()), rows(a.rows), cols(a.cols), row_stride(a.cols) {}
  const T &operator()(std::size_t r, std::size_t c) const { return ptr[r * row_stride + c]; }
};

struct HookCtx {                           // lib.rs:844-862
  std::uint8_t water_level, max_water_level;
  ArrayView2<std::uint8_t> image;
  ArrayView2<usize> colours;
  const std::vector<std::pair<usize, Seed>> *seeds;    // (colour, (row, col)), lib.rs:1671-1672
};

// One ws_ctx per object; not thread safe (make one per thread: the reference's structs are Send + Sync).
class Context {
 public:
  explicit Context(int device = 0) {
    int rc = ws_ctx_create(device, &ctx_);
    if (rc != WS_OK) throw WatershedError(rc, "ws_ctx_create");
  }
  ~Context() { ws_ctx_destroy(ctx_); }
  Context(const Context &) = delete;
  Context &operator=(const Context &) = delete;
  ws_ctx *get() const { return ctx_; }
  void check(int rc) const {
    if (rc == WS_OK) return;
    if (rc == WS_ERR_SEED_OOB) throw std::out_of_range(ws_last_error(ctx_));
    throw WatershedError(rc, ws_last_error(ctx_));
  }

 private:
  ws_ctx *ctx_ = nullptr;
};

namespace detail {
template <class T>
struct HookBox {
  std::function<T(const HookCtx &)> fn;
  std::vector<T> out;
  const std::vector<std::pair<usize, Seed>> *seeds;
  static void thunk(void *user, std::uint8_t lvl, std::uint8_t mx, const std::uint8_t *img, const std::uint64_t *lab,
                    std::size_t h, std::size_t w) {
    auto *self = static_cast<HookBox *>(user);
    HookCtx ctx{lvl, mx, ArrayView2<std::uint8_t>(img, h, w, w), ArrayView2<usize>(lab, h, w, w), self->seeds};
    self->out.push_back(self->fn(ctx));
  }
};
inline std::vector<std::uint64_t> pack(const std::vector<Seed> &seeds) {
  std::vector<std::uint64_t> p(2 * seeds.size());
  for (std::size_t i = 0; i < seeds.size(); ++i) { p[2 * i] = seeds[i].first; p[2 * i + 1] = seeds[i].second; }
  return p;
}
}  // namespace detail

template <class E> struct dtype_of;
template <> struct dtype_of<float> { static constexpr int value = WS_F32; };
template <> struct dtype_of<double> { static constexpr int value = WS_F64; };
template <> struct dtype_of<std::int32_t> { static constexpr int value = WS_I32; };
template <> struct dtype_of<std::uint16_t> { static constexpr int value = WS_U16; };
template <> struct dtype_of<std::int16_t> { static constexpr int value = WS_I16; };
template <> struct dtype_of<std::uint8_t> { static constexpr int value = WS_U8; };

class WatershedUtils {                     // lib.rs:1069-1198
 public:
  // lib.rs:1134-1173: pre_processor_with_max::<MAX, T, D>; any dimension, passed as a flat span
  template <std::uint8_t MAX, class E>
  std::vector<std::uint8_t> pre_processor_with_max(const E *data, std::size_t n) const {
    static_assert(MAX < NEVER_FILL && MAX > ALWAYS_FILL, "lib.rs:1143-1144");
    std::vector<std::uint8_t> out(n);
    ctx_->check(ws_pre_processor(ctx_->get(), data, dtype_of<E>::value, n, MAX, out.data()));
    return out;
  }
  template <class E>
  std::vector<std::uint8_t> pre_processor(const E *data, std::size_t n) const {   // lib.rs:1081-1087
    return pre_processor_with_max<NORMAL_MAX, E>(data, n);
  }

  std::vector<Seed> find_local_minima(ArrayView2<std::uint8_t> img) const {
    const std::size_t cap = ((img.rows ? img.rows - 1 : 0) / 2 + 1) * ((img.cols ? img.cols - 1 : 0) / 2 + 1);
    std::vector<std::uint64_t> rc(2 * cap);
    std::size_t n = 0;
    ctx_->check(ws_find_local_minima(ctx_->get(), img.ptr, img.rows, img.cols, img.row_stride, rc.data(), cap, &n));
    std::vector<Seed> out(n);
    for (std::size_t i = 0; i < n; ++i) out[i] = {rc[2 * i], rc[2 * i + 1]};
    return out;
  }

  // not in the reference: pre_processor_with_max::<MAX> of every slice of a cube as one call (tests/integration.rs:267-290 normalise
  // one slice of a FITS cube after the other).  Element (k, r, c) of the view sits at data + k * slice_stride + r * row_stride +
  // c * col_stride (elements; a channel-last cube has slice_stride 1); the result is the contiguous (n_slices, h, w) u8 cube the
  // *_cube methods take.  minmax (nullable) receives every slice's zero-seeded (min, max).
  template <std::uint8_t MAX, class E>
  std::vector<std::uint8_t> pre_processor_cube_with_max(const E *data, std::size_t n_slices, std::size_t h, std::size_t w, std::size_t slice_stride,
                                                        std::size_t row_stride, std::size_t col_stride,
                                                        std::vector<std::pair<double, double>> *minmax = nullptr) const {
    static_assert(MAX < NEVER_FILL && MAX > ALWAYS_FILL, "lib.rs:1143-1144");
    std::vector<std::uint8_t> out(n_slices * h * w);
    std::vector<double> mm(minmax ? 2 * n_slices : 0);
    std::size_t failed = 0;
    const int rc = ws_pre_processor_batch(ctx_->get(), data, dtype_of<E>::value, n_slices, h, w, slice_stride, row_stride, col_stride, MAX,
                                          out.data(), minmax ? mm.data() : nullptr, &failed);
    if (rc == WS_ERR_UNSUPPORTED)      // a WS_F64 slice whose range is not finite: name it, as the other shims do
      throw WatershedError(rc, "slice " + std::to_string(failed) + ": " + ws_last_error(ctx_->get()));
    ctx_->check(rc);
    if (minmax) {
      minmax->resize(n_slices);
      for (std::size_t k = 0; k < n_slices; ++k) (*minmax)[k] = {mm[2 * k], mm[2 * k + 1]};
    }
    return out;
  }
  template <class E>
  std::vector<std::uint8_t> pre_processor_cube(const E *data, std::size_t n_slices, std::size_t h, std::size_t w, std::size_t slice_stride,
                                               std::size_t row_stride, std::size_t col_stride) const {
    return pre_processor_cube_with_max<NORMAL_MAX, E>(data, n_slices, h, w, slice_stride, row_stride, col_stride);
  }

  // not in the reference: find_local_minima of every slice of a u8 cube as one call.  Returns the slices' lists back to back;
  // offsets (n_slices + 1 entries): slice k's seeds are [offsets[k], offsets[k + 1]).
  std::vector<Seed> find_local_minima_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t h, std::size_t w, std::size_t row_stride,
                                           std::size_t slice_stride, std::vector<std::size_t> &offsets) const {
    const std::size_t cap = ((h ? h - 1 : 0) / 2 + 1) * ((w ? w - 1 : 0) / 2 + 1) * n_slices;
    std::vector<std::uint64_t> rc(2 * cap + 2);
    offsets.assign(n_slices + 1, 0);
    std::size_t n = 0;
    ctx_->check(ws_find_local_minima_batch(ctx_->get(), cube, n_slices, h, w, row_stride, slice_stride, rc.data(), cap, offsets.data(), &n));
    std::vector<Seed> out(n);
    for (std::size_t i = 0; i < n; ++i) out[i] = {rc[2 * i], rc[2 * i + 1]};
    return out;
  }

 protected:
  explicit WatershedUtils(std::shared_ptr<Context> c) : ctx_(std::move(c)) {}
  std::shared_ptr<Context> ctx_;
};

template <class T>
class Watershed : public WatershedUtils {  // lib.rs:1206-1238
 public:
  using Hook = std::function<T(const HookCtx &)>;
  std::uint8_t max_water_level() const { return opt_.max_water_level; }
  bool edge_correction() const { return opt_.edge_correction != 0; }

  std::vector<T> transform_with_hook(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds) const {
    if (!hook_) { run<int>(input, seeds, nullptr, nullptr); return {}; }   // lib.rs:1796-1807: work done, empty Vec
    return run<T>(input, seeds, &hook_, nullptr);
  }
  std::vector<std::pair<std::uint8_t, Array2<usize>>> transform_history(ArrayView2<std::uint8_t> input,
                                                                          const std::vector<Seed> &seeds) const {
    using R = std::pair<std::uint8_t, Array2<usize>>;
    std::function<R(const HookCtx &)> h = [](const HookCtx &c) {           // lib.rs:1545 / 1831
      Array2<usize> a(c.colours.rows, c.colours.cols);
      for (std::size_t r = 0; r < a.rows; ++r)
        for (std::size_t q = 0; q < a.cols; ++q) a(r, q) = c.colours(r, q);
      return R{c.water_level, std::move(a)};
    };
    return run<R>(input, seeds, &h, nullptr);
  }
  // not in the reference: transform_history for the water levels in `levels` only (any order, repeats allowed, at most 256) as
  // one call of the library (ws_transform_history: no per-level hook); entry k is levels[k]'s.  With every level 0..=max in
  // order it equals transform_history.
  std::vector<std::pair<std::uint8_t, Array2<usize>>> transform_history_levels(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds,
                                                                               const std::vector<std::uint8_t> &levels) const {
    const std::size_t e = opt_.edge_correction ? 2 : 0, rows = input.rows + e, cols = input.cols + e, npx = rows * cols;
    auto packed = detail::pack(seeds);
    std::vector<usize> flat(levels.size() * npx);
    ctx_->check(ws_transform_history(ctx_->get(), merging_, input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(),
                                     &opt_, levels.data(), levels.size(), flat.data()));
    std::vector<std::pair<std::uint8_t, Array2<usize>>> out;
    for (std::size_t k = 0; k < levels.size(); ++k) {
      Array2<usize> a(rows, cols);
      std::copy(flat.begin() + k * npx, flat.begin() + (k + 1) * npx, a.data.begin());
      out.emplace_back(levels[k], std::move(a));
    }
    return out;
  }
  // lib.rs:1220-1224: Vec<(u8, Vec<usize>)>, each inner Vec of length pixels+1 (lib.rs:630)
  std::vector<std::pair<std::uint8_t, std::vector<usize>>> transform_to_list(ArrayView2<std::uint8_t> input,
                                                                              const std::vector<Seed> &seeds) const {
    const std::size_t e = opt_.edge_correction ? 2 : 0, npx = (input.rows + e) * (input.cols + e);
    const std::size_t levels = std::size_t(opt_.max_water_level) + 1;
    std::vector<std::uint64_t> offsets(levels + 1), unc(levels);
    auto packed = detail::pack(seeds);
    // one record per live lake and level, at most seeds * levels; half of that covers a random field.  A too
    // small guess costs a second transform, not a wrong answer.
    std::size_t cap = std::min<std::size_t>(seeds.size() * levels / 2 + 1024, std::size_t(1) << 26), n = 0;
    std::vector<ws_lake> lakes;
    for (;;) {
      lakes.resize(cap);
      int rc = ws_transform_to_list(ctx_->get(), merging_, input.ptr, input.rows, input.cols, input.row_stride, packed.data(),
                                    seeds.size(), &opt_, lakes.data(), cap, &n, offsets.data(), unc.data());
      if (rc == WS_ERR_CAPACITY && n > cap) { cap = n; continue; }
      ctx_->check(rc);
      break;
    }
    std::vector<std::pair<std::uint8_t, std::vector<usize>>> out;
    for (std::size_t l = 0; l < levels; ++l) {
      std::vector<usize> hist(npx + 1, 0);
      for (std::uint64_t i = offsets[l]; i < offsets[l + 1]; ++i) hist[lakes[i].colour] = lakes[i].area;
      hist[0] = unc[l];
      out.emplace_back(std::uint8_t(l), std::move(hist));
    }
    return out;
  }

  // not in the reference: transform_to_list(cube[k], find_local_minima(cube[k])) of every slice of a contiguous u8 cube
  // (n_slices x rows x cols) as one call (ws_transform_to_list_batch), sparse: per slice, per level the uncoloured count and the
  // (colour, area) of every lake with pixels, in no particular order.  n_seeds (nullable) receives the slices' minima counts.
  struct SparseLevel {
    std::uint8_t level;
    usize uncoloured;
    std::vector<ws_lake> lakes;
  };
  std::vector<std::vector<SparseLevel>> transform_to_list_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows,
                                                               std::size_t cols, std::vector<std::size_t> *n_seeds = nullptr) const {
    const std::size_t levels = std::size_t(opt_.max_water_level) + 1;
    std::vector<std::uint64_t> offsets(n_slices * levels + 1), unc(n_slices * levels);
    std::vector<std::size_t> counts(n_slices);
    // one record per pixel of the cube; a too small guess costs a second transform, not a wrong answer
    std::size_t cap = std::min<std::size_t>(n_slices * rows * cols + 1024, std::size_t(1) << 28), n = 0, failed = 0;
    std::vector<ws_lake> lakes;
    for (;;) {
      lakes.resize(cap);
      int rc = ws_transform_to_list_batch(ctx_->get(), merging_, cube, n_slices, rows, cols, cols, rows * cols, nullptr, nullptr, &opt_,
                                          lakes.data(), cap, &n, offsets.data(), unc.data(), counts.data(), &failed);
      if (rc == WS_ERR_CAPACITY && n > cap) { cap = n; continue; }
      ctx_->check(rc);
      break;
    }
    std::vector<std::vector<SparseLevel>> out(n_slices);
    for (std::size_t k = 0; k < n_slices; ++k)
      for (std::size_t l = 0; l < levels; ++l) {
        const std::size_t b = k * levels + l;
        out[k].push_back({std::uint8_t(l), (usize)unc[b], std::vector<ws_lake>(lakes.begin() + offsets[b], lakes.begin() + offsets[b + 1])});
      }
    if (n_seeds) *n_seeds = counts;
    return out;
  }
  // not in the reference: transform_history_levels(cube[k], find_local_minima(cube[k]), levels) of every slice of a contiguous u8
  // cube (n_slices x rows x cols) as one call (ws_transform_history_batch); entry [k][j] is slice k's plane for levels[j], in the
  // slice's own colours.  n_seeds (nullable) receives the slices' minima counts.
  std::vector<std::vector<std::pair<std::uint8_t, Array2<usize>>>> transform_history_cube(const std::uint8_t *cube, std::size_t n_slices,
                                                                                          std::size_t rows, std::size_t cols,
                                                                                          const std::vector<std::uint8_t> &levels,
                                                                                          std::vector<std::size_t> *n_seeds = nullptr) const {
    const std::size_t e = opt_.edge_correction ? 2 : 0, prow = rows + e, pcol = cols + e, npx = prow * pcol, nl = levels.size();
    std::vector<usize> flat(n_slices * nl * npx);
    std::vector<std::size_t> counts(n_slices);
    std::size_t failed = 0;
    ctx_->check(ws_transform_history_batch(ctx_->get(), merging_, cube, n_slices, rows, cols, cols, rows * cols, nullptr, nullptr, &opt_,
                                           levels.data(), nl, flat.data(), counts.data(), &failed));
    std::vector<std::vector<std::pair<std::uint8_t, Array2<usize>>>> out(n_slices);
    for (std::size_t k = 0; k < n_slices; ++k)
      for (std::size_t j = 0; j < nl; ++j) {
        Array2<usize> a(prow, pcol);
        const auto from = flat.begin() + (k * nl + j) * npx;
        std::copy(from, from + npx, a.data.begin());
        out[k].emplace_back(levels[j], std::move(a));
      }
    if (n_seeds) *n_seeds = counts;
    return out;
  }

 protected:
  Watershed(ws_options o, Hook h, std::shared_ptr<Context> c, int merging)
      : WatershedUtils(std::move(c)), opt_(o), hook_(std::move(h)), merging_(merging) {}

  template <class R>
  std::vector<R> run(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::function<R(const HookCtx &)> *hook,
                     Array2<usize> *final_labels) const {
    auto packed = detail::pack(seeds);
    std::vector<std::pair<usize, Seed>> seed_colours;
    detail::HookBox<R> box;
    if (hook) {
      for (std::size_t i = 0; i < seeds.size(); ++i) seed_colours.push_back({i + 1, seeds[i]});
      box.fn = *hook;
      box.seeds = &seed_colours;
    }
    auto fn = merging_ ? ws_merge_with_hook : ws_segment_with_hook;
    ctx_->check(fn(ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(), &opt_,
                   hook ? &detail::HookBox<R>::thunk : nullptr, hook ? &box : nullptr,
                   final_labels ? final_labels->data.data() : nullptr));
    return std::move(box.out);
  }

  ws_options opt_;
  Hook hook_;
  int merging_;
};

template <class T = int>
class SegmentingWatershed : public Watershed<T> {     // lib.rs:1609-1849
 public:
  // lib.rs:1810-1822, intended semantics (the reference's body panics): labels after the last level
  Array2<usize> transform(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0;
    Array2<usize> out(input.rows + e, input.cols + e);
    this->template run<int>(input, seeds, nullptr, &out);
    return out;
  }
  // Not in the reference: its README's call pair, transform(input, find_local_minima(input)) (lib.rs:73-86), as ONE call of the
  // library (ws_segment_minima).  `seeds_out` (optional) receives the list the labels are numbered by.
  Array2<usize> transform_from_minima(ArrayView2<std::uint8_t> input, std::vector<Seed> *seeds_out = nullptr) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0;
    Array2<usize> out(input.rows + e, input.cols + e);
    const std::size_t cap = seeds_out && input.rows >= 3 && input.cols >= 3 ? ((input.rows - 1) / 2 + 1) * ((input.cols - 1) / 2 + 1) : 0;
    std::vector<std::uint64_t> rc(2 * cap + 2);
    std::size_t n = 0;
    this->ctx_->check(ws_segment_minima(this->ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, &this->opt_,
                                        reinterpret_cast<std::uint64_t *>(out.data.data()), cap ? rc.data() : nullptr, cap, &n));
    if (seeds_out) {
      seeds_out->resize(n);
      for (std::size_t i = 0; i < n; ++i) (*seeds_out)[i] = {(usize)rc[2 * i], (usize)rc[2 * i + 1]};
    }
    return out;
  }
  // Not in the reference: what its integration tests loop over (tests/integration.rs:267,356 -- find_local_minima + transform for
  // one slice of a cube after the other) as ONE call of the library (ws_segment_batch: the slices' uploads, transforms and label
  // copies overlap).  `cube`: n_slices contiguous rows x cols slices; slice k of the result is transform_from_minima of slice k.
  std::vector<Array2<usize>> transform_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0, plane = (rows + e) * (cols + e);
    std::vector<std::uint64_t> flat(n_slices * plane + 1);
    std::size_t failed = 0;
    this->ctx_->check(ws_segment_batch(this->ctx_->get(), cube, n_slices, rows, cols, cols, rows * cols, nullptr, nullptr, &this->opt_, flat.data(),
                                       nullptr, &failed));
    std::vector<Array2<usize>> out(n_slices, Array2<usize>(rows + e, cols + e));
    for (std::size_t k = 0; k < n_slices; ++k)
      for (std::size_t i = 0; i < plane; ++i) out[k].data[i] = (usize)flat[k * plane + i];
    return out;
  }

 private:
  template <class U> friend class TransformBuilder;
  using Watershed<T>::Watershed;
};

template <class T = int>
class MergingWatershed : public Watershed<T> {        // lib.rs:1297-1562
 public:
  // lib.rs:1524-1536: a stub in the reference (zeros, interior 123, seeds ignored)
  Array2<usize> transform(ArrayView2<std::uint8_t> input, const std::vector<Seed> &) const {
    Array2<usize> out(input.rows, input.cols);
    int rc = ws_merge_transform_stub(input.rows, input.cols, out.data.data());
    if (rc != WS_OK) throw WatershedError(rc, "ws_merge_transform_stub");
    return out;
  }
  // not in the reference: merged labels after the last level (canonical ids)
  Array2<usize> transform_final(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0;
    Array2<usize> out(input.rows + e, input.cols + e);
    this->template run<int>(input, seeds, nullptr, &out);
    return out;
  }
  // not in the reference: the lake hierarchy of the merging transform, one record per seed colour (index 0 .. seeds.size()) from
  // one flood, no plane written (ws_merge_tree): which lake swallowed which, after what water level, how big each was
  struct MergeTree {
    static constexpr std::uint32_t ALIVE = WS_TREE_ALIVE;
    std::vector<ws_tree_node> nodes;
    Array2<usize> labels;      // the segmenting labels the colours refer to (0 x 0 unless asked for)
    // colour -> canonical id of its lake after water level `level`: follow `parent` while death_level <= level
    std::vector<std::uint32_t> roots_at(std::uint32_t level) const {
      std::vector<std::uint32_t> root(nodes.size());
      for (std::size_t c = 0; c < nodes.size(); ++c) {
        std::uint32_t x = std::uint32_t(c);
        while (nodes[x].death_level <= level) x = nodes[x].parent;
        root[c] = x;
      }
      return root;
    }
    // colour -> the first node of its parent chain that `cut` keeps: alive, or area >= min_area and n_leaves >= min_leaves
    std::vector<std::uint32_t> cut_table(const ws_tree_cut &cut) const {
      std::vector<std::uint32_t> node(nodes.size());
      for (std::size_t c = 0; c < nodes.size(); ++c) {
        std::uint32_t x = std::uint32_t(c);
        while (nodes[x].death_level != ALIVE && (nodes[x].area < cut.min_area || nodes[x].n_leaves < cut.min_leaves)) x = nodes[x].parent;
        node[c] = x;
      }
      return node;
    }
    // the same with catalogue thresholds (ws_lake_cut): `stats` is the catalogue of the tree's flood (merge_tree_stats); a node is
    // also kept only if its sum_w, w_max and depth -- death_level - w_min where that is positive, else 0 -- reach the cut's
    std::vector<std::uint32_t> cut_table(const ws_lake_cut &cut, const std::vector<ws_lake_stats> &stats) const {
      if (stats.size() != nodes.size()) throw std::invalid_argument("one catalogue record per tree record");
      auto kept = [&](std::uint32_t x) {
        const ws_tree_node &t = nodes[x];
        const ws_lake_stats &s = stats[x];
        if (t.death_level == ALIVE) return true;
        const std::uint32_t depth = t.death_level > s.w_min ? t.death_level - s.w_min : 0;
        return t.area >= cut.min_area && t.n_leaves >= cut.min_leaves && s.sum_w >= cut.min_sum_w && s.w_max >= cut.min_w_max &&
               depth >= cut.min_depth;
      };
      std::vector<std::uint32_t> node(nodes.size());
      for (std::size_t c = 0; c < nodes.size(); ++c) {
        std::uint32_t x = std::uint32_t(c);
        while (!kept(x)) x = nodes[x].parent;
        node[c] = x;
      }
      return node;
    }
  };
  // one cut of a merge tree (ws_tree_cut): thresholds on a swallowed lake's pixels and seed colours, the last level shown, the
  // last level whose merges are applied
  static ws_tree_cut cut(std::uint32_t min_area = 0, std::uint32_t min_leaves = 0, std::uint8_t show_level = 254, std::uint8_t merge_level = 0) {
    return ws_tree_cut{min_area, min_leaves, show_level, merge_level, {0, 0}};
  }
  // not in the reference: the label planes of the merge tree pruned by `cuts` (at most 32), the whole route in one call
  // (ws_merge_tree_cut): planes[k] shows every pixel the lake cuts[k] leaves it in, 0 where it is hidden; lakes[offsets[k] ..
  // offsets[k + 1]) are cut k's (colour, pixels) records in increasing colour and hidden[k] its pixels that show 0
  struct TreeCut {
    MergeTree tree;
    std::vector<Array2<usize>> planes;
    std::vector<ws_lake> lakes;
    std::vector<std::uint64_t> offsets, hidden;
  };
  TreeCut tree_cut(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_tree_cut> &cuts) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0, prow = input.rows + e, pcol = input.cols + e, k = cuts.size();
    TreeCut t{MergeTree{std::vector<ws_tree_node>(seeds.size() + 1), Array2<usize>(0, 0)}, {}, {}, std::vector<std::uint64_t>(k + 1, 0),
              std::vector<std::uint64_t>(k, 0)};
    if (k == 0) throw std::invalid_argument("tree_cut needs at least one cut");
    auto packed = detail::pack(seeds);
    std::vector<usize> flat(k * prow * pcol);
    std::size_t cap = std::max<std::size_t>(std::min(seeds.size(), prow * pcol), 1) * k, total = 0;      // a cut shows no more colours than there are, or pixels
    t.lakes.resize(cap);
    this->ctx_->check(ws_merge_tree_cut(this->ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(),
                                        &this->opt_, cuts.data(), k, t.tree.nodes.data(), flat.data(), t.lakes.data(), cap, &total,
                                        t.offsets.data(), t.hidden.data()));
    t.lakes.resize(total);
    for (std::size_t j = 0; j < k; ++j) {
      t.planes.emplace_back(prow, pcol);
      std::copy(flat.begin() + j * prow * pcol, flat.begin() + (j + 1) * prow * pcol, t.planes.back().data.begin());
    }
    return t;
  }
  // one cut by catalogue quantities as well (ws_lake_cut): the lake's weights summed to min_sum_w, its largest weight reached
  // min_w_max, and it died min_depth above its smallest weight
  static ws_lake_cut lake_cut(std::uint64_t min_sum_w = 0, std::uint32_t min_w_max = 0, std::uint32_t min_depth = 0, std::uint32_t min_area = 0,
                              std::uint32_t min_leaves = 0, std::uint8_t show_level = 254, std::uint8_t merge_level = 0) {
    return ws_lake_cut{min_sum_w, min_area, min_leaves, min_w_max, min_depth, show_level, merge_level, {0, 0, 0, 0, 0, 0}};
  }
  // tree_cut with the lake catalogue of the same flood (ws_merge_tree_stats_cut): the cuts may carry catalogue thresholds, and the
  // catalogue comes back with the tree.  Weights: a u8 or u16 plane of the image's shape; without one the image itself weighs.
  struct LakeCut : TreeCut {
    std::vector<ws_lake_stats> stats;
  };
  LakeCut tree_cut(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts) const {
    return lake_cut_run(input, seeds, cuts, nullptr, 0, 0);
  }
  LakeCut tree_cut(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts,
                   ArrayView2<std::uint8_t> weights) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return lake_cut_run(input, seeds, cuts, weights.ptr, WS_U8, weights.row_stride);
  }
  LakeCut tree_cut(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts,
                   ArrayView2<std::uint16_t> weights) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return lake_cut_run(input, seeds, cuts, weights.ptr, WS_U16, weights.row_stride);
  }
  // tree_cut with the regions the cuts show MEASURED in the same call (ws_merge_tree_cut_catalogue): region_stats[i] holds the
  // moments, the box, the extrema and the first peak pixel of the pixels lakes[i] counts -- the region of that colour in its cut, not
  // stats[colour], which measures the lake as it was when it died -- and hidden_stats[k] those of the pixels cut k shows as 0.
  struct CutCatalogue : LakeCut {
    std::vector<ws_lake_stats> region_stats, hidden_stats;
  };
  CutCatalogue tree_cut_catalogue(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts) const {
    return cut_catalogue_run(input, seeds, cuts, nullptr, 0, 0);
  }
  CutCatalogue tree_cut_catalogue(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts,
                                  ArrayView2<std::uint8_t> weights) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return cut_catalogue_run(input, seeds, cuts, weights.ptr, WS_U8, weights.row_stride);
  }
  CutCatalogue tree_cut_catalogue(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts,
                                  ArrayView2<std::uint16_t> weights) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return cut_catalogue_run(input, seeds, cuts, weights.ptr, WS_U16, weights.row_stride);
  }
  MergeTree merge_tree(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, bool want_labels = false) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0;
    MergeTree t{std::vector<ws_tree_node>(seeds.size() + 1), Array2<usize>(want_labels ? input.rows + e : 0, want_labels ? input.cols + e : 0)};
    auto packed = detail::pack(seeds);
    this->ctx_->check(ws_merge_tree(this->ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(),
                                    &this->opt_, t.nodes.data(), want_labels ? t.labels.data.data() : nullptr));
    return t;
  }
  // not in the reference: merge_tree and a catalogue of its lakes from the same flood (ws_merge_tree_stats): stats[c] holds the
  // weighted and plain first moments, the box, the extrema and the first peak pixel of the pixels nodes[c].area counts, stats[0]
  // those of the pixels never coloured; rows and columns are those of the padded plane.  Weights: a u8 or u16 plane of the image's
  // shape; without one the image itself weighs.
  struct LakeCatalogue {
    MergeTree tree;
    std::vector<ws_lake_stats> stats;
    std::vector<ws_lake_shape> shapes;      // merge_tree_shapes only: the second moments, exact 128-bit sums as (low, high)
    // the weighted centroid (row, col) of record c in the padded plane; false where the record weighs nothing
    bool centroid(std::size_t c, double *row, double *col) const {
      const ws_lake_stats &r = stats[c];
      if (r.sum_w == 0) return false;
      *row = double(r.sum_wr) / double(r.sum_w);
      *col = double(r.sum_wc) / double(r.sum_w);
      return true;
    }
  };
  LakeCatalogue merge_tree_stats(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, bool want_labels = false) const {
    return lake_catalogue(input, seeds, nullptr, 0, 0, want_labels);
  }
  LakeCatalogue merge_tree_stats(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, ArrayView2<std::uint8_t> weights,
                                 bool want_labels = false) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return lake_catalogue(input, seeds, weights.ptr, WS_U8, weights.row_stride, want_labels);
  }
  LakeCatalogue merge_tree_stats(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, ArrayView2<std::uint16_t> weights,
                                 bool want_labels = false) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return lake_catalogue(input, seeds, weights.ptr, WS_U16, weights.row_stride, want_labels);
  }
  // not in the reference: merge_tree_stats and the second moments of every lake from the same flood (ws_merge_tree_shapes):
  // shapes[c] holds the exact sums of v row^2, v col^2, v row col, row^2, col^2 and row col over the pixels nodes[c].area counts.
  LakeCatalogue merge_tree_shapes(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, bool want_labels = false) const {
    return lake_catalogue(input, seeds, nullptr, 0, 0, want_labels, true);
  }
  LakeCatalogue merge_tree_shapes(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, ArrayView2<std::uint8_t> weights,
                                  bool want_labels = false) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return lake_catalogue(input, seeds, weights.ptr, WS_U8, weights.row_stride, want_labels, true);
  }
  LakeCatalogue merge_tree_shapes(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, ArrayView2<std::uint16_t> weights,
                                  bool want_labels = false) const {
    if (weights.rows != input.rows || weights.cols != input.cols) throw std::invalid_argument("weights must have the image's shape");
    return lake_catalogue(input, seeds, weights.ptr, WS_U16, weights.row_stride, want_labels, true);
  }
  // not in the reference: merge_tree of every slice of a contiguous cube (n_slices x rows x cols) as ONE call of the library
  // (ws_merge_tree_batch: slices that stack share one flood, one set of per-level unions and one fold launch per level).
  // seeds: one list per slice, or nullptr for every slice's own find_local_minima (n_seeds, nullable, receives the counts).
  std::vector<MergeTree> merge_tree_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                         const std::vector<std::vector<Seed>> *seeds = nullptr, bool want_labels = false,
                                         std::vector<std::size_t> *n_seeds = nullptr) const {
    if (seeds && seeds->size() != n_slices) throw std::invalid_argument("one seed list per slice");
    const std::size_t e = this->opt_.edge_correction ? 2 : 0, prow = rows + e, pcol = cols + e, npx = prow * pcol;
    std::vector<std::uint64_t> packed;
    std::vector<std::size_t> offs(n_slices + 1, 0), counts(n_slices, 0);
    if (seeds)
      for (std::size_t k = 0; k < n_slices; ++k) {
        const auto one = detail::pack((*seeds)[k]);
        packed.insert(packed.end(), one.begin(), one.end());
        offs[k + 1] = offs[k] + (*seeds)[k].size();
      }
    // own minima: rarely denser than one pixel in eight; a too small guess is answered before any flood with the count
    std::size_t cap = seeds ? offs[n_slices] + n_slices : n_slices * (rows * cols / 8 + 1), total = 0, failed = 0;
    std::vector<ws_tree_node> flat(cap);
    std::vector<usize> labels(want_labels ? n_slices * npx : 0);
    for (int attempt = 0; attempt < 2; ++attempt) {
      const int rc = ws_merge_tree_batch(this->ctx_->get(), cube, n_slices, rows, cols, cols, rows * cols, seeds ? packed.data() : nullptr,
                                         seeds ? offs.data() : nullptr, &this->opt_, flat.data(), cap, &total,
                                         want_labels ? labels.data() : nullptr, counts.data(), &failed);
      if (rc == WS_ERR_CAPACITY && total > cap && attempt == 0) {
        cap = total;
        flat.resize(cap);
        continue;
      }
      this->ctx_->check(rc);
      break;
    }
    std::vector<MergeTree> out;
    std::size_t at = 0;
    for (std::size_t k = 0; k < n_slices; ++k) {
      const std::size_t n = counts[k] + 1;
      MergeTree t{std::vector<ws_tree_node>(flat.begin() + at, flat.begin() + at + n), Array2<usize>(want_labels ? prow : 0, want_labels ? pcol : 0)};
      if (want_labels) std::copy(labels.begin() + k * npx, labels.begin() + (k + 1) * npx, t.labels.data.begin());
      out.push_back(std::move(t));
      at += n;
    }
    if (n_seeds) *n_seeds = counts;
    return out;
  }
  // not in the reference: merge_tree_stats of every slice of a contiguous cube as ONE call of the library
  // (ws_merge_tree_stats_batch: slices that stack share one flood, one set of per-level unions and one fold launch per level of
  // the tree and of the statistics).  Every catalogue is what merge_tree_stats returns for the slice alone: the slice's own
  // colours, rows, columns and peak pixels.  weights: a contiguous u8 or u16 cube of the cube's shape; without one the cube itself
  // weighs.  seeds and n_seeds as merge_tree_cube.
  std::vector<LakeCatalogue> merge_tree_stats_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                   const std::vector<std::vector<Seed>> *seeds = nullptr, bool want_labels = false,
                                                   std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, nullptr, 0, seeds, want_labels, n_seeds);
  }
  // (a literal nullptr in the fifth place means "own minima, no weights", as it does for merge_tree_cube)
  std::vector<LakeCatalogue> merge_tree_stats_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                   std::nullptr_t, bool want_labels = false, std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, nullptr, 0, nullptr, want_labels, n_seeds);
  }
  std::vector<LakeCatalogue> merge_tree_stats_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                   const std::uint8_t *weights, const std::vector<std::vector<Seed>> *seeds = nullptr,
                                                   bool want_labels = false, std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, weights, WS_U8, seeds, want_labels, n_seeds);
  }
  std::vector<LakeCatalogue> merge_tree_stats_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                   const std::uint16_t *weights, const std::vector<std::vector<Seed>> *seeds = nullptr,
                                                   bool want_labels = false, std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, weights, WS_U16, seeds, want_labels, n_seeds);
  }
  // not in the reference: merge_tree_shapes of every slice of a contiguous cube as ONE call of the library
  // (ws_merge_tree_shapes_batch: slices that stack run the shape kernels once over the stack, after the tree's and the
  // statistics').  Every catalogue is what merge_tree_shapes returns for the slice alone, `shapes` filled: rows and columns are the
  // slice's own.  Arguments as merge_tree_stats_cube.
  std::vector<LakeCatalogue> merge_tree_shapes_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                    const std::vector<std::vector<Seed>> *seeds = nullptr, bool want_labels = false,
                                                    std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, nullptr, 0, seeds, want_labels, n_seeds, true);
  }
  std::vector<LakeCatalogue> merge_tree_shapes_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                    std::nullptr_t, bool want_labels = false, std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, nullptr, 0, nullptr, want_labels, n_seeds, true);
  }
  std::vector<LakeCatalogue> merge_tree_shapes_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                    const std::uint8_t *weights, const std::vector<std::vector<Seed>> *seeds = nullptr,
                                                    bool want_labels = false, std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, weights, WS_U8, seeds, want_labels, n_seeds, true);
  }
  std::vector<LakeCatalogue> merge_tree_shapes_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                    const std::uint16_t *weights, const std::vector<std::vector<Seed>> *seeds = nullptr,
                                                    bool want_labels = false, std::vector<std::size_t> *n_seeds = nullptr) const {
    return lake_catalogue_cube(cube, n_slices, rows, cols, weights, WS_U16, seeds, want_labels, n_seeds, true);
  }

  // not in the reference: tree_cut_catalogue of every slice of a contiguous cube as ONE call of the library
  // (ws_merge_tree_cut_catalogue_batch: slices that stack share one flood, and every stacked group is cut once, while its stamps
  // are on the device).  Every CutCatalogue is what tree_cut_catalogue returns for the slice alone: the slice's own colours, rows,
  // columns and peak pixels, offsets from 0.  weights, seeds and n_seeds as merge_tree_stats_cube.
  std::vector<CutCatalogue> merge_tree_cut_catalogue_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                          const std::vector<ws_lake_cut> &cuts, const std::vector<std::vector<Seed>> *seeds = nullptr,
                                                          std::vector<std::size_t> *n_seeds = nullptr) const {
    return cut_catalogue_cube(cube, n_slices, rows, cols, cuts, nullptr, 0, seeds, n_seeds);
  }
  std::vector<CutCatalogue> merge_tree_cut_catalogue_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                          const std::vector<ws_lake_cut> &cuts, const std::uint8_t *weights,
                                                          const std::vector<std::vector<Seed>> *seeds = nullptr,
                                                          std::vector<std::size_t> *n_seeds = nullptr) const {
    return cut_catalogue_cube(cube, n_slices, rows, cols, cuts, weights, WS_U8, seeds, n_seeds);
  }
  std::vector<CutCatalogue> merge_tree_cut_catalogue_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                          const std::vector<ws_lake_cut> &cuts, const std::uint16_t *weights,
                                                          const std::vector<std::vector<Seed>> *seeds = nullptr,
                                                          std::vector<std::size_t> *n_seeds = nullptr) const {
    return cut_catalogue_cube(cube, n_slices, rows, cols, cuts, weights, WS_U16, seeds, n_seeds);
  }

 private:
  std::vector<CutCatalogue> cut_catalogue_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                               const std::vector<ws_lake_cut> &cuts, const void *weights, int dtype,
                                               const std::vector<std::vector<Seed>> *seeds, std::vector<std::size_t> *n_seeds) const {
    if (seeds && seeds->size() != n_slices) throw std::invalid_argument("one seed list per slice");
    const std::size_t e = this->opt_.edge_correction ? 2 : 0, prow = rows + e, pcol = cols + e, npx = prow * pcol, k = cuts.size();
    if (k == 0) throw std::invalid_argument("merge_tree_cut_catalogue_cube needs at least one cut");
    std::vector<std::uint64_t> packed;
    std::vector<std::size_t> offs(n_slices + 1, 0), counts(n_slices, 0);
    if (seeds)
      for (std::size_t s = 0; s < n_slices; ++s) {
        const auto one = detail::pack((*seeds)[s]);
        packed.insert(packed.end(), one.begin(), one.end());
        offs[s + 1] = offs[s] + (*seeds)[s].size();
        counts[s] = (*seeds)[s].size();
      }
    // (as merge_tree_cube: a too small guess of the records is answered before any flood with the count; of the lists, with the need)
    std::size_t rec_cap = seeds ? offs[n_slices] + n_slices : n_slices * (rows * cols / 8 + 1), total = 0, failed = 0, got = 0;
    std::size_t cap = std::max<std::size_t>(std::min(rec_cap, n_slices * npx), 1) * k;
    std::vector<ws_tree_node> flat(rec_cap);
    std::vector<ws_lake_stats> records(rec_cap), region(cap), hidden_stats(n_slices * k);
    std::vector<ws_lake> lakes(cap);
    std::vector<usize> planes(n_slices * k * npx);
    std::vector<std::uint64_t> offsets(n_slices * k + 1, 0), hidden(n_slices * k, 0);
    for (int attempt = 0; attempt < 3; ++attempt) {
      const int rc = ws_merge_tree_cut_catalogue_batch(this->ctx_->get(), cube, n_slices, rows, cols, cols, rows * cols, seeds ? packed.data() : nullptr,
                                                       seeds ? offs.data() : nullptr, &this->opt_, weights, dtype, cols, rows * cols, cuts.data(), k,
                                                       flat.data(), records.data(), rec_cap, &total, planes.data(), lakes.data(), region.data(), cap,
                                                       &got, offsets.data(), hidden.data(), hidden_stats.data(), counts.data(), &failed);
      if (rc == WS_ERR_CAPACITY && total > rec_cap && attempt < 2) {
        rec_cap = total;
        flat.resize(rec_cap);
        records.resize(rec_cap);
        continue;
      }
      if (rc == WS_ERR_CAPACITY && got > cap && attempt < 2) {
        cap = got;
        lakes.resize(cap);
        region.resize(cap);
        continue;
      }
      this->ctx_->check(rc);
      break;
    }
    std::vector<CutCatalogue> out;
    std::size_t at = 0;
    for (std::size_t s = 0; s < n_slices; ++s) {
      const std::size_t n = counts[s] + 1, lo = offsets[s * k], hi = offsets[(s + 1) * k];
      CutCatalogue t;
      t.tree = MergeTree{std::vector<ws_tree_node>(flat.begin() + at, flat.begin() + at + n), Array2<usize>(0, 0)};
      t.stats.assign(records.begin() + at, records.begin() + at + n);
      t.lakes.assign(lakes.begin() + lo, lakes.begin() + hi);
      t.region_stats.assign(region.begin() + lo, region.begin() + hi);
      t.hidden.assign(hidden.begin() + s * k, hidden.begin() + (s + 1) * k);
      t.hidden_stats.assign(hidden_stats.begin() + s * k, hidden_stats.begin() + (s + 1) * k);
      for (std::size_t j = 0; j <= k; ++j) t.offsets.push_back(offsets[s * k + j] - lo);
      for (std::size_t j = 0; j < k; ++j) {
        t.planes.emplace_back(prow, pcol);
        std::copy(planes.begin() + (s * k + j) * npx, planes.begin() + (s * k + j + 1) * npx, t.planes.back().data.begin());
      }
      out.push_back(std::move(t));
      at += n;
    }
    if (n_seeds) *n_seeds = counts;
    return out;
  }
  std::vector<LakeCatalogue> lake_catalogue_cube(const std::uint8_t *cube, std::size_t n_slices, std::size_t rows, std::size_t cols,
                                                 const void *weights, int dtype, const std::vector<std::vector<Seed>> *seeds,
                                                 bool want_labels, std::vector<std::size_t> *n_seeds, bool with_shapes = false) const {
    if (seeds && seeds->size() != n_slices) throw std::invalid_argument("one seed list per slice");
    const std::size_t e = this->opt_.edge_correction ? 2 : 0, prow = rows + e, pcol = cols + e, npx = prow * pcol;
    std::vector<std::uint64_t> packed;
    std::vector<std::size_t> offs(n_slices + 1, 0), counts(n_slices, 0);
    if (seeds)
      for (std::size_t k = 0; k < n_slices; ++k) {
        const auto one = detail::pack((*seeds)[k]);
        packed.insert(packed.end(), one.begin(), one.end());
        offs[k + 1] = offs[k] + (*seeds)[k].size();
        counts[k] = (*seeds)[k].size();
      }
    // (as merge_tree_cube: a too small guess is answered before any flood with the count)
    std::size_t cap = seeds ? offs[n_slices] + n_slices : n_slices * (rows * cols / 8 + 1), total = 0, failed = 0;
    std::vector<ws_tree_node> flat(cap);
    std::vector<ws_lake_stats> records(cap);
    std::vector<ws_lake_shape> shapes(with_shapes ? cap : 0);
    std::vector<usize> labels(want_labels ? n_slices * npx : 0);
    for (int attempt = 0; attempt < 2; ++attempt) {
      const std::uint64_t *seeds_rc = seeds ? packed.data() : nullptr;
      const std::size_t *seed_offs = seeds ? offs.data() : nullptr;
      usize *labels_out = want_labels ? labels.data() : nullptr;
      const int rc = with_shapes ? ws_merge_tree_shapes_batch(this->ctx_->get(), cube, n_slices, rows, cols, cols, rows * cols, seeds_rc, seed_offs,
                                                              &this->opt_, weights, dtype, cols, rows * cols, flat.data(), records.data(),
                                                              shapes.data(), cap, &total, labels_out, counts.data(), &failed)
                                 : ws_merge_tree_stats_batch(this->ctx_->get(), cube, n_slices, rows, cols, cols, rows * cols, seeds_rc, seed_offs,
                                                             &this->opt_, weights, dtype, cols, rows * cols, flat.data(), records.data(), cap,
                                                             &total, labels_out, counts.data(), &failed);
      if (rc == WS_ERR_CAPACITY && total > cap && attempt == 0) {
        cap = total;
        flat.resize(cap);
        records.resize(cap);
        if (with_shapes) shapes.resize(cap);
        continue;
      }
      this->ctx_->check(rc);
      break;
    }
    std::vector<LakeCatalogue> out;
    std::size_t at = 0;
    for (std::size_t k = 0; k < n_slices; ++k) {
      const std::size_t n = counts[k] + 1;
      LakeCatalogue cat{MergeTree{std::vector<ws_tree_node>(flat.begin() + at, flat.begin() + at + n),
                                  Array2<usize>(want_labels ? prow : 0, want_labels ? pcol : 0)},
                        std::vector<ws_lake_stats>(records.begin() + at, records.begin() + at + n)};
      if (with_shapes) cat.shapes.assign(shapes.begin() + at, shapes.begin() + at + n);
      if (want_labels) std::copy(labels.begin() + k * npx, labels.begin() + (k + 1) * npx, cat.tree.labels.data.begin());
      out.push_back(std::move(cat));
      at += n;
    }
    if (n_seeds) *n_seeds = counts;
    return out;
  }
  LakeCut lake_cut_run(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts, const void *weights,
                       int dtype, std::size_t weight_stride) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0, prow = input.rows + e, pcol = input.cols + e, k = cuts.size();
    if (k == 0) throw std::invalid_argument("tree_cut needs at least one cut");
    LakeCut t;
    t.tree = MergeTree{std::vector<ws_tree_node>(seeds.size() + 1), Array2<usize>(0, 0)};
    t.offsets.assign(k + 1, 0);
    t.hidden.assign(k, 0);
    t.stats.resize(seeds.size() + 1);
    auto packed = detail::pack(seeds);
    std::vector<usize> flat(k * prow * pcol);
    std::size_t cap = std::max<std::size_t>(std::min(seeds.size(), prow * pcol), 1) * k, total = 0;      // a cut shows no more colours than there are, or pixels
    t.lakes.resize(cap);
    this->ctx_->check(ws_merge_tree_stats_cut(this->ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(),
                                              &this->opt_, weights, dtype, weight_stride, cuts.data(), k, t.tree.nodes.data(), t.stats.data(),
                                              flat.data(), t.lakes.data(), cap, &total, t.offsets.data(), t.hidden.data()));
    t.lakes.resize(total);
    for (std::size_t j = 0; j < k; ++j) {
      t.planes.emplace_back(prow, pcol);
      std::copy(flat.begin() + j * prow * pcol, flat.begin() + (j + 1) * prow * pcol, t.planes.back().data.begin());
    }
    return t;
  }
  CutCatalogue cut_catalogue_run(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const std::vector<ws_lake_cut> &cuts,
                                 const void *weights, int dtype, std::size_t weight_stride) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0, prow = input.rows + e, pcol = input.cols + e, k = cuts.size();
    if (k == 0) throw std::invalid_argument("tree_cut_catalogue needs at least one cut");
    CutCatalogue t;
    t.tree = MergeTree{std::vector<ws_tree_node>(seeds.size() + 1), Array2<usize>(0, 0)};
    t.offsets.assign(k + 1, 0);
    t.hidden.assign(k, 0);
    t.stats.resize(seeds.size() + 1);
    t.hidden_stats.resize(k);
    auto packed = detail::pack(seeds);
    std::vector<usize> flat(k * prow * pcol);
    std::size_t cap = std::max<std::size_t>(std::min(seeds.size(), prow * pcol), 1) * k, total = 0;      // a cut shows no more colours than there are, or pixels
    t.lakes.resize(cap);
    t.region_stats.resize(cap);
    this->ctx_->check(ws_merge_tree_cut_catalogue(this->ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(),
                                                  &this->opt_, weights, dtype, weight_stride, cuts.data(), k, t.tree.nodes.data(), t.stats.data(),
                                                  flat.data(), t.lakes.data(), t.region_stats.data(), cap, &total, t.offsets.data(), t.hidden.data(),
                                                  t.hidden_stats.data()));
    t.lakes.resize(total);
    t.region_stats.resize(total);
    for (std::size_t j = 0; j < k; ++j) {
      t.planes.emplace_back(prow, pcol);
      std::copy(flat.begin() + j * prow * pcol, flat.begin() + (j + 1) * prow * pcol, t.planes.back().data.begin());
    }
    return t;
  }
  LakeCatalogue lake_catalogue(ArrayView2<std::uint8_t> input, const std::vector<Seed> &seeds, const void *weights, int dtype,
                               std::size_t weight_stride, bool want_labels, bool want_shapes = false) const {
    const std::size_t e = this->opt_.edge_correction ? 2 : 0;
    LakeCatalogue cat{MergeTree{std::vector<ws_tree_node>(seeds.size() + 1),
                                Array2<usize>(want_labels ? input.rows + e : 0, want_labels ? input.cols + e : 0)},
                      std::vector<ws_lake_stats>(seeds.size() + 1), std::vector<ws_lake_shape>(want_shapes ? seeds.size() + 1 : 0)};
    auto packed = detail::pack(seeds);
    if (want_shapes) {
      this->ctx_->check(ws_merge_tree_shapes(this->ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(),
                                             &this->opt_, weights, dtype, weight_stride, cat.tree.nodes.data(), cat.stats.data(),
                                             cat.shapes.data(), want_labels ? cat.tree.labels.data.data() : nullptr));
      return cat;
    }
    this->ctx_->check(ws_merge_tree_stats(this->ctx_->get(), input.ptr, input.rows, input.cols, input.row_stride, packed.data(), seeds.size(),
                                          &this->opt_, weights, dtype, weight_stride, cat.tree.nodes.data(), cat.stats.data(),
                                          want_labels ? cat.tree.labels.data.data() : nullptr));
    return cat;
  }
  template <class U> friend class TransformBuilder;
  using Watershed<T>::Watershed;
};

template <class T = int>
class TransformBuilder {                   // lib.rs:908-1047
 public:
  TransformBuilder() { ws_options_default(&opt_); }                                  // lib.rs:936-946
  static TransformBuilder new_() { return TransformBuilder(); }
  TransformBuilder &set_max_water_lvl(std::uint8_t v) { opt_.max_water_level = v; return *this; }   // lib.rs:950
  TransformBuilder &enable_edge_correction() { opt_.edge_correction = 1; return *this; }             // lib.rs:958
  TransformBuilder &set_wlvl_hook(std::function<T(const HookCtx &)> h) { hook_ = std::move(h); return *this; }   // lib.rs:967
  TransformBuilder &set_engine(ws_engine e) { opt_.engine = std::uint8_t(e); return *this; }        // this implementation only
  TransformBuilder &set_context(std::shared_ptr<Context> c) { ctx_ = std::move(c); return *this; }
  // this implementation only (ws_options.seed_shift): with edge correction, seeds move by (+1, +1) onto their own pixel
  // instead of indexing the padded plane with the caller's coordinates (lib.rs:1675-1677)
  TransformBuilder &shift_seeds_into_padded_plane(bool on = true) { opt_.seed_shift = on ? 1 : 0; return *this; }

  SegmentingWatershed<T> build_segmenting() const {                                                  // lib.rs:1024-1046
    validate();
    return SegmentingWatershed<T>(opt_, hook_, ctx_ ? ctx_ : std::make_shared<Context>(0), 0);
  }
  MergingWatershed<T> build_merging() const {                                                        // lib.rs:998-1020
    validate();
    return MergingWatershed<T>(opt_, hook_, ctx_ ? ctx_ : std::make_shared<Context>(0), 1);
  }

 private:
  void validate() const {
    const int rc = ws_options_validate(&opt_);
    if (rc == WS_ERR_MAX_TOO_HIGH) throw BuildErr(BuildErr::MaxToHigh, opt_.max_water_level);     // lib.rs:1026-1027
    if (rc == WS_ERR_MAX_TOO_LOW) throw BuildErr(BuildErr::MaxToLow, opt_.max_water_level);       // lib.rs:1028-1029
    if (rc != WS_OK) throw WatershedError(rc, "ws_options_validate");
  }
  ws_options opt_;
  std::function<T(const HookCtx &)> hook_;
  std::shared_ptr<Context> ctx_;
};

}  // namespace rustronomy_watershed
