// ws_cube_plan.hpp -- the host arithmetic of the cube front end (ws_cube_input.hip), plain C++ so that it can be tested without a
// device (tests/cpp/test_cube_plan.cpp): the extent of a strided view, the runs of slices of the stacked minima, and how a run's
// 32-bit offsets become the call's size_t offsets.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace wsplan {

// *total = n_slices * h * w; *span = elements between the first and the last element of the view, both included (0 for an empty
// view).  false when either leaves size_t, or the span times 16 (the widest element and some slack) does.
inline bool cube_extent(size_t n_slices, size_t h, size_t w, size_t ss, size_t rs, size_t cs, size_t *total, size_t *span) {
  size_t hw = 0, t = 0, a = 0, b = 0, d = 0;
  *total = 0;
  *span = 0;
  if (__builtin_mul_overflow(h, w, &hw) || __builtin_mul_overflow(hw, n_slices, &t)) return false;
  *total = t;
  if (t == 0) return true;
  if (__builtin_mul_overflow(n_slices - 1, ss, &a) || __builtin_mul_overflow(h - 1, rs, &b) || __builtin_mul_overflow(w - 1, cs, &d) ||
      __builtin_add_overflow(a, b, &a) || __builtin_add_overflow(a, d, &a) || __builtin_add_overflow(a, (size_t)1, &a) || a > (~(size_t)0 >> 4))
    return false;
  *span = a;
  return true;
}

constexpr size_t MINIMA_STACK_ROWS_MAX = 0x7FFFFFFFull - 15;      // stacked rows of one run: 2^31 - 16
constexpr size_t MINIMA_RUN_NIBBLE_BYTES = (size_t)1 << 29;       // nibble plane of one run: narrow slices cost 256 B a row whatever their width

// slices per run of the stacked minima (h, w >= 3; h * w < 2^32): whole slices under max_px pixels, MINIMA_STACK_ROWS_MAX rows and
// MINIMA_RUN_NIBBLE_BYTES of nibble plane (row_nibbles bytes a row), at least one, at most n_slices
inline size_t minima_run_slices(size_t n_slices, size_t h, size_t w, size_t max_px, size_t row_nibbles) {
  size_t per = max_px / (h * w);
  const size_t by_rows = MINIMA_STACK_ROWS_MAX / h, by_bytes = MINIMA_RUN_NIBBLE_BYTES / (h * row_nibbles);
  if (by_rows < per) per = by_rows;
  if (by_bytes < per) per = by_bytes;
  if (per < 1) per = 1;
  return per < n_slices ? per : n_slices;
}

// a run's offsets (g + 1 words from the device: where each of its g slices begins within the run, and the run's total) added to the
// call's: seed_offsets[k0 .. k0 + g) are written, the new running total is returned
inline size_t minima_add_run(const uint32_t *run_offsets, size_t g, size_t k0, size_t total, size_t *seed_offsets) {
  for (size_t i = 0; i < g; ++i) seed_offsets[k0 + i] = total + run_offsets[i];
  return total + run_offsets[g];
}

}  // namespace wsplan
