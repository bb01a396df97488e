"""Device-resident entry points over PyTorch-ROCm tensors.

PyTorch is plumbing here (HBM allocations, the current HIP stream, torch.distributed);
all compute is the HIP engine behind include/ws_hip.h.  Tensors hold raw bits: label and
seed planes are int32 tensors carrying the uint32 values of the C ABI.
"""
import ctypes

import torch

from . import _ffi
from .api import Context, ENGINE_AUTO


class DeviceEngine:
    """One engine context on torch's CURRENT stream of the device.  Create it under a stream of your own
    (`torch.cuda.set_stream(torch.cuda.Stream(dev))`, as bench.py does) rather than on the legacy default stream: a repeated
    transform is replayed as one hipGraph, and HIP cannot capture on the legacy stream -- there every transform is its eleven
    stream operations (2048^2: 0.155 instead of 0.123 ms; results are the same)."""

    def __init__(self, device_index=0, engine=ENGINE_AUTO):
        if not torch.cuda.is_available():
            raise RuntimeError("DeviceEngine needs a HIP device (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.device("cuda", device_index)
        torch.cuda.set_device(self.device)
        # enqueue on torch's current stream so torch events bracket the engine's kernels
        self.stream = torch.cuda.current_stream(self.device)
        self.ctx = Context(device_index, stream=self.stream.cuda_stream)
        self.engine = engine

    def options(self, max_level=254, edge=False, engine=None, seed_shift=False):
        return _ffi.Options(max_level, int(edge), self.engine if engine is None else engine, 0, int(seed_shift))

    def random_field(self, h, w, seed):
        img = torch.empty((h, w), dtype=torch.uint8, device=self.device)
        self.ctx.check(_ffi.lib().ws_random_field_device(self.ctx.handle, img.data_ptr(), h, w, w, seed))
        return img

    def find_local_minima(self, img):
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        h, w = img.shape
        cap = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1)
        out = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=self.device)
        n = ctypes.c_size_t(0)
        self.ctx.check(_ffi.lib().ws_find_local_minima_device(self.ctx.handle, img.data_ptr(), h, w, w, out.data_ptr(),
                                                              cap, ctypes.byref(n)))
        return out[: n.value]

    _DTYPES = {torch.float32: 0, torch.float64: 1, torch.int32: 2, torch.int16: 4, torch.uint8: 5}
    if hasattr(torch, "uint16"):
        _DTYPES[torch.uint16] = 3

    def _max_value(self, max_value):
        if not 1 <= int(max_value) <= 254:
            raise AssertionError("MAX must be in 1..=254 (lib.rs:1143-1144)")      # the reference asserts
        return int(max_value)

    def pre_processor(self, data, max_value=254):
        """pre_processor_with_max of a device tensor of any shape (ws_pre_processor_device): one (min, max) over all of it.  Returns
        a uint8 tensor of the same shape.  float64 data waits for the stream once (the range check); other dtypes stay asynchronous."""
        assert data.is_cuda and data.dtype in self._DTYPES, "float32, float64, int32, int16, uint16 or uint8 on the device"
        data = data.contiguous()
        out = torch.empty(data.shape, dtype=torch.uint8, device=self.device)
        self.ctx.check(_ffi.lib().ws_pre_processor_device(self.ctx.handle, data.data_ptr(), self._DTYPES[data.dtype], data.numel(),
                                                          self._max_value(max_value), out.data_ptr()))
        return out

    def pre_processor_batch(self, data, axis=0, max_value=254, want_minmax=False):
        """pre_processor_with_max of every slice along `axis` of a 3-D device tensor (ws_pre_processor_batch_device), each with its
        own (min, max); the tensor's strides go to the engine as they are (a channel-last cube, axis=2, is not copied).  Returns the
        contiguous (n_slices, h, w) uint8 cube every *_batch method takes, with want_minmax also a float64 (n_slices, 2) tensor."""
        assert data.is_cuda and data.dim() == 3 and data.dtype in self._DTYPES
        view = data.movedim(axis, 0)
        if any(st < 0 for st in view.stride()):
            view = view.contiguous()
        n, h, w = view.shape
        ss, rs, cs = view.stride()
        out = torch.empty((n, h, w), dtype=torch.uint8, device=self.device)
        minmax = torch.empty((n, 2), dtype=torch.float64, device=self.device) if want_minmax else None
        failed = ctypes.c_size_t(0)
        rc = _ffi.lib().ws_pre_processor_batch_device(self.ctx.handle, view.data_ptr() if view.numel() else None, self._DTYPES[data.dtype],
                                                      n, h, w, ss, rs, cs, self._max_value(max_value), out.data_ptr() if out.numel() else None,
                                                      minmax.data_ptr() if want_minmax and n else None, ctypes.byref(failed))
        if rc == _ffi.WS_ERR_UNSUPPORTED:
            from .api import WatershedError
            raise WatershedError(rc, f"slice {failed.value}: " + _ffi.lib().ws_last_error(self.ctx.handle).decode())
        self.ctx.check(rc)
        return (out, minmax) if want_minmax else out

    def find_local_minima_batch(self, cube):
        """find_local_minima of every slice of a contiguous (S, H, W) uint8 device cube (ws_find_local_minima_batch_device).  Returns
        (seeds, seed_offsets): int32 (n, 2) device tensor of slice-local (row, col) pairs, back to back, and S + 1 host integers
        (numpy) -- the pair every *_batch method takes."""
        import numpy as np
        assert cube.dtype == torch.uint8 and cube.dim() == 3 and cube.is_contiguous() and cube.is_cuda
        s, h, w = cube.shape
        cap = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1) * s
        out = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=self.device)
        offsets = np.zeros(s + 1, dtype=np.uintp)
        n = ctypes.c_size_t(0)
        self.ctx.check(_ffi.lib().ws_find_local_minima_batch_device(self.ctx.handle, cube.data_ptr() if cube.numel() else None, s, h, w, w, h * w,
                                                                    out.data_ptr(), cap, offsets.ctypes.data_as(_ffi.szp), ctypes.byref(n)))
        return out[: n.value], offsets

    def _plane(self, img, edge):
        e = 2 if edge else 0
        return img.shape[0] + e, img.shape[1] + e

    def segment(self, img, seeds, max_level=254, edge=False, engine=None, out=None, seed_shift=False):
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        h, w = img.shape
        if out is None:
            out = torch.empty(self._plane(img, edge), dtype=torch.int32, device=self.device)
        opt = self.options(max_level, edge, engine, seed_shift)
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        self.ctx.check(_ffi.lib().ws_segment_device(self.ctx.handle, img.data_ptr(), h, w, w,
                                                    seeds.data_ptr() if ns else None, ns, ctypes.byref(opt),
                                                    out.data_ptr()))
        return out

    def segment_minima(self, img, max_level=254, edge=False, engine=None, out=None, want_seeds=False):
        """find_local_minima + segment as one call (ws_segment_minima_device): labels, n_seeds[, seeds]."""
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        h, w = img.shape
        if out is None:
            out = torch.empty(self._plane(img, edge), dtype=torch.int32, device=self.device)
        opt = self.options(max_level, edge, engine, False)
        cap = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1) if want_seeds else 0
        seeds = torch.empty((max(cap, 1), 2), dtype=torch.int32, device=self.device) if want_seeds else None
        n = ctypes.c_size_t(0)
        self.ctx.check(_ffi.lib().ws_segment_minima_device(self.ctx.handle, img.data_ptr(), h, w, w, ctypes.byref(opt), out.data_ptr(),
                                                           seeds.data_ptr() if want_seeds else None, cap, ctypes.byref(n)))
        return (out, n.value, seeds[: n.value]) if want_seeds else (out, n.value)

    def segment_begin(self, img, seeds, out, max_level=254, edge=False, seed_shift=False):
        """First half of segment() (ws_segment_device_begin): queues the transform and returns.  The engine is busy until
        segment_end(); img, seeds and out must stay alive and unchanged until then.  Two engines taking turns keep the
        GPU fed between transforms."""
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        assert out.dtype == torch.int32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == self._plane(img, edge)
        h, w = img.shape
        opt = self.options(max_level, edge, None, seed_shift)
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        self._pending = (img, seeds, out)
        self.ctx.check(_ffi.lib().ws_segment_device_begin(self.ctx.handle, img.data_ptr(), h, w, w,
                                                          seeds.data_ptr() if ns else None, ns, ctypes.byref(opt),
                                                          out.data_ptr()))
        return out

    def segment_end(self):
        """Second half: waits for the transform begun with segment_begin() and raises if it failed."""
        pending, self._pending = getattr(self, "_pending", None), None
        self.ctx.check(_ffi.lib().ws_segment_device_end(self.ctx.handle))
        return pending[2] if pending else None

    def segment_batch(self, cube, seeds, seed_offsets, max_level=254, edge=False, out=None, seed_shift=False):
        """A stack of independent slices (config C4).  cube: (S, H, W) uint8; seeds: all slices' (row, col) pairs
        concatenated, int32 (n, 2); seed_offsets: S + 1 host integers.  Returns (S, H', W') int32 labels."""
        assert cube.dtype == torch.uint8 and cube.dim() == 3 and cube.is_contiguous() and cube.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        s, h, w = cube.shape
        assert len(seed_offsets) == s + 1
        e = 2 if edge else 0
        if out is None:
            out = torch.empty((s, h + e, w + e), dtype=torch.int32, device=self.device)
        opt = self.options(max_level, edge, None, seed_shift)
        offs = (ctypes.c_size_t * (s + 1))(*[int(x) for x in seed_offsets])
        failed = ctypes.c_size_t(0)
        self.ctx.check(_ffi.lib().ws_segment_batch_device(self.ctx.handle, cube.data_ptr(), s, h, w, w, h * w,
                                                          seeds.data_ptr() if seeds.numel() else None, offs,
                                                          ctypes.byref(opt), out.data_ptr(), ctypes.byref(failed)))
        return out

    def merge(self, img, seeds, max_level=254, edge=False, out=None, seed_shift=False):
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        h, w = img.shape
        if out is None:
            out = torch.empty(self._plane(img, edge), dtype=torch.int32, device=self.device)
        opt = self.options(max_level, edge, None, seed_shift)
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        self.ctx.check(_ffi.lib().ws_merge_device(self.ctx.handle, img.data_ptr(), h, w, w,
                                                  seeds.data_ptr() if ns else None, ns, ctypes.byref(opt),
                                                  out.data_ptr()))
        return out

    def merge_begin(self, img, seeds, out, max_level=254, edge=False, seed_shift=False):
        """First half of merge() (ws_merge_device_begin); rules as segment_begin()."""
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        assert out.dtype == torch.int32 and out.is_cuda and out.is_contiguous() and tuple(out.shape) == self._plane(img, edge)
        h, w = img.shape
        opt = self.options(max_level, edge, None, seed_shift)
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        self._pending = (img, seeds, out)
        self.ctx.check(_ffi.lib().ws_merge_device_begin(self.ctx.handle, img.data_ptr(), h, w, w,
                                                        seeds.data_ptr() if ns else None, ns, ctypes.byref(opt),
                                                        out.data_ptr()))
        return out

    def merge_end(self):
        pending, self._pending = getattr(self, "_pending", None), None
        self.ctx.check(_ffi.lib().ws_merge_device_end(self.ctx.handle))
        return pending[2] if pending else None

    def last_arrival(self):
        """Arrival stamps (level << 24 | ring) of the last fused-engine call, as a tensor copy."""
        p = ctypes.c_void_p()
        h = ctypes.c_size_t()
        w = ctypes.c_size_t()
        self.ctx.check(_ffi.lib().ws_last_arrival_device(self.ctx.handle, ctypes.byref(p), ctypes.byref(h), ctypes.byref(w)))
        out = torch.empty((h.value, w.value), dtype=torch.int32, device=self.device)
        self.ctx.check(_ffi.lib().ws_copy_last_arrival_device(self.ctx.handle, out.data_ptr(), out.numel()))
        return out

    def transform_to_list(self, img, seeds, merging=True, max_level=254, edge=False, lakes=None):
        """transform_to_list with the records left in HBM: returns (lakes (n, 2) int64 tensor of (colour, area) on the device,
        offsets numpy (levels + 1), uncoloured numpy (levels)).  `lakes`: a reusable (cap, 2) int64 device buffer."""
        import numpy as np
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        h, w = img.shape
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        levels = max_level + 1
        opt = self.options(max_level, edge)
        offsets = np.zeros(levels + 1, dtype=np.uint64)
        unc = np.zeros(levels, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        cap = int(lakes.shape[0]) if lakes is not None else max(ns, 1) * levels // 2 + 1024
        while True:
            if lakes is None or lakes.shape[0] < cap:
                lakes = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
            rc = _ffi.lib().ws_transform_to_list_device(self.ctx.handle, int(merging), img.data_ptr(), h, w, w,
                                                        seeds.data_ptr() if ns else None, ns, ctypes.byref(opt), lakes.data_ptr(), cap,
                                                        ctypes.byref(n), offsets.ctypes.data, unc.ctypes.data)
            if rc == _ffi.WS_ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            self.ctx.check(rc)
            break
        return lakes[: n.value], offsets, unc

    @staticmethod
    def _batch_args(cube, seeds, seed_offsets):
        if cube.dim() != 3:
            raise ValueError("cube must be 3-D: (slices, rows, columns)")
        if len(seed_offsets) != cube.shape[0] + 1:
            raise ValueError("seed_offsets needs one entry per slice and one more")
        assert cube.dtype == torch.uint8 and cube.is_contiguous() and cube.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        s = cube.shape[0]
        return (ctypes.c_size_t * (s + 1))(*[int(x) for x in seed_offsets])

    def transform_to_list_batch(self, cube, seeds, seed_offsets, merging=True, max_level=254, edge=False, lakes=None):
        """transform_to_list of every slice of a cube (ws_transform_to_list_batch_device), records left in HBM.  cube: (S, H, W)
        uint8; seeds: all slices' (row, col) pairs concatenated, int32 (n, 2); seed_offsets: S + 1 host integers.  Returns (lakes
        (n, 2) int64 device tensor of (colour, area), offsets numpy (S * levels + 1), uncoloured numpy (S * levels)): slice k's
        records at level l are lakes[offsets[k * levels + l] : offsets[k * levels + l + 1]], in the slice's own colours."""
        import numpy as np
        offs = self._batch_args(cube, seeds, seed_offsets)
        s, h, w = cube.shape
        levels = max_level + 1
        opt = self.options(max_level, edge)
        offsets = np.zeros(s * levels + 1, dtype=np.uint64)
        unc = np.zeros(max(s * levels, 1), dtype=np.uint64)
        n = ctypes.c_size_t(0)
        failed = ctypes.c_size_t(0)
        ns = int(seed_offsets[-1]) - int(seed_offsets[0])
        cap = int(lakes.shape[0]) if lakes is not None else max(ns, 1) * levels // 2 + 1024
        while True:
            if lakes is None or lakes.shape[0] < cap:
                lakes = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
            rc = _ffi.lib().ws_transform_to_list_batch_device(self.ctx.handle, int(merging), cube.data_ptr(), s, h, w, w, h * w,
                                                              seeds.data_ptr() if seeds.numel() else None, offs, ctypes.byref(opt),
                                                              lakes.data_ptr(), cap, ctypes.byref(n), offsets.ctypes.data,
                                                              unc.ctypes.data, ctypes.byref(failed))
            if rc == _ffi.WS_ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            self.ctx.check(rc)
            break
        return lakes[: n.value], offsets, unc[: s * levels]

    def merge_batch(self, cube, seeds, seed_offsets, max_level=254, edge=False, out=None, seed_shift=False):
        """The merging transform's final labels of every slice of a cube (ws_merge_batch_device); arguments as segment_batch.
        Returns (S, H', W') int32 labels, slice k as merge(cube[k], its seeds)."""
        offs = self._batch_args(cube, seeds, seed_offsets)
        s, h, w = cube.shape
        e = 2 if edge else 0
        if out is None:
            out = torch.empty((s, h + e, w + e), dtype=torch.int32, device=self.device)
        opt = self.options(max_level, edge, None, seed_shift)
        failed = ctypes.c_size_t(0)
        self.ctx.check(_ffi.lib().ws_merge_batch_device(self.ctx.handle, cube.data_ptr(), s, h, w, w, h * w,
                                                        seeds.data_ptr() if seeds.numel() else None, offs,
                                                        ctypes.byref(opt), out.data_ptr(), ctypes.byref(failed)))
        return out

    def level_snapshot(self, labels, water_level, out=None):
        """The segmenting label plane after `water_level` (transform_history's entry for that level), on the device."""
        if out is None:
            out = torch.empty_like(labels)
        self.ctx.check(_ffi.lib().ws_level_snapshot_device(self.ctx.handle, labels.data_ptr(), int(water_level), out.data_ptr()))
        return out

    def transform_history(self, img, seeds, levels=None, merging=False, max_level=254, edge=False, out=None):
        """transform_history for the water levels in `levels` (any order, repeats allowed, at most 256; None: 0..=max_level) with
        everything in HBM (ws_transform_history_device): a (K, H', W') int32 tensor whose plane k is the label plane the reference's
        hook sees after levels[k] -- merging: canonical lake ids.  `out`: a reusable (K, H', W') int32 device tensor."""
        from .api import _history_levels
        lv = _history_levels(levels, max_level)
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        h, w = img.shape
        ph, pw = self._plane(img, edge)
        if out is None:
            out = torch.empty((lv.size, ph, pw), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (lv.size, ph, pw):
            raise ValueError(f"out must be a contiguous int32 tensor of shape {(lv.size, ph, pw)}")
        if lv.size == 0:
            return out
        opt = self.options(max_level, edge)
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        self.ctx.check(_ffi.lib().ws_transform_history_device(self.ctx.handle, int(merging), img.data_ptr(), h, w, w,
                                                              seeds.data_ptr() if ns else None, ns, ctypes.byref(opt),
                                                              lv.ctypes.data, lv.size, out.data_ptr(), ph * pw))
        return out

    def transform_history_batch(self, cube, seeds, seed_offsets, levels=None, merging=False, max_level=254, edge=False, out=None):
        """transform_history of every slice of a cube for the water levels in `levels` (any order, repeats allowed, at most 256;
        None: 0..=max_level) with everything in HBM (ws_transform_history_batch_device); cube, seeds and seed_offsets as
        transform_to_list_batch.  Returns an (S, K, H', W') int32 tensor: out[k, j] is transform_history(cube[k], its seeds,
        levels)[j], in the slice's own colours.  `out`: a reusable (S, K, H', W') int32 device tensor."""
        from .api import _history_levels
        lv = _history_levels(levels, max_level)
        offs = self._batch_args(cube, seeds, seed_offsets)
        s, h, w = cube.shape
        e = 2 if edge else 0
        shape = (s, lv.size, h + e, w + e)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError(f"out must be a contiguous int32 tensor of shape {shape}")
        if lv.size == 0 or s == 0:
            return out
        opt = self.options(max_level, edge)
        failed = ctypes.c_size_t(0)
        self.ctx.check(_ffi.lib().ws_transform_history_batch_device(self.ctx.handle, int(merging), cube.data_ptr(), s, h, w, w, h * w,
                                                                    seeds.data_ptr() if seeds.numel() else None, offs, ctypes.byref(opt),
                                                                    lv.ctypes.data, lv.size, out.data_ptr(), (h + e) * (w + e),
                                                                    ctypes.byref(failed)))
        return out

    def merge_tree(self, img, seeds, max_level=254, edge=False, seed_shift=False, want_labels=False, out=None):
        """The merging transform's lake hierarchy with everything in HBM (ws_merge_tree_device): an (n_seeds + 1, 4) int32 tensor
        whose row c is colour c's (parent, death_level, area, n_leaves) -- uint32 bits, death_level -1 = never died.  With
        want_labels also the segmenting (H', W') int32 label plane the colours refer to: returns (tree, labels).  `out`: a
        reusable contiguous (n_seeds + 1, 4) int32 device tensor."""
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        h, w = img.shape
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        if out is None:
            out = torch.empty((ns + 1, 4), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (ns + 1, 4):
            raise ValueError(f"out must be a contiguous int32 tensor of shape {(ns + 1, 4)}")
        labels = torch.empty(self._plane(img, edge), dtype=torch.int32, device=self.device) if want_labels else None
        opt = self.options(max_level, edge, None, seed_shift)
        self.ctx.check(_ffi.lib().ws_merge_tree_device(self.ctx.handle, img.data_ptr(), h, w, w, seeds.data_ptr() if ns else None, ns,
                                                       ctypes.byref(opt), out.data_ptr(), labels.data_ptr() if want_labels else None))
        return (out, labels) if want_labels else out

    def merge_tree_stats(self, img, seeds, weights=None, max_level=254, edge=False, seed_shift=False, want_labels=False, out=None,
                         out_stats=None):
        """merge_tree and a catalogue of its lakes from the same flood with everything in HBM (ws_merge_tree_stats_device): the
        tree tensor of merge_tree and an (n_seeds + 1, 9) int64 tensor of raw ws_lake_stats records -- row c, the bits of colour
        c's 72 bytes: sum_w, sum_wr, sum_wc, sum_r, sum_c (uint64 bits), then r_min | r_max << 32, c_min | c_max << 32,
        w_min | w_max << 32, peak_pixel | reserved << 32.  weights: a 2-D uint8 or int16 / uint16 (taken as u16 bits) device
        tensor of the image's shape whose rows are contiguous (a row stride in elements is honoured), None: the image itself.
        With want_labels returns (tree, stats, labels).  `out`, `out_stats`: reusable contiguous tensors of those shapes."""
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        h, w = img.shape
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        dtype, wstride = 0, 0
        if weights is not None:
            u16 = {torch.int16, getattr(torch, "uint16", torch.int16)}
            if weights.dtype != torch.uint8 and weights.dtype not in u16:
                raise TypeError("weights must be a uint8, uint16 or int16 (u16 bits) tensor")
            if not weights.is_cuda or weights.dim() != 2 or tuple(weights.shape) != (h, w) or (w > 1 and weights.stride(1) != 1):
                raise ValueError(f"weights must be a device tensor of shape {(h, w)} with contiguous rows")
            dtype = _ffi.WS_DTYPES["uint8" if weights.dtype == torch.uint8 else "uint16"]
            wstride = weights.stride(0) if h > 1 else w
        if out is None:
            out = torch.empty((ns + 1, 4), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (ns + 1, 4):
            raise ValueError(f"out must be a contiguous int32 tensor of shape {(ns + 1, 4)}")
        if out_stats is None:
            out_stats = torch.empty((ns + 1, 9), dtype=torch.int64, device=self.device)
        elif out_stats.dtype != torch.int64 or not out_stats.is_contiguous() or tuple(out_stats.shape) != (ns + 1, 9):
            raise ValueError(f"out_stats must be a contiguous int64 tensor of shape {(ns + 1, 9)}")
        labels = torch.empty(self._plane(img, edge), dtype=torch.int32, device=self.device) if want_labels else None
        opt = self.options(max_level, edge, None, seed_shift)
        self.ctx.check(_ffi.lib().ws_merge_tree_stats_device(self.ctx.handle, img.data_ptr(), h, w, w, seeds.data_ptr() if ns else None, ns,
                                                             ctypes.byref(opt), weights.data_ptr() if weights is not None else None, dtype,
                                                             wstride, out.data_ptr(), out_stats.data_ptr(),
                                                             labels.data_ptr() if want_labels else None))
        return (out, out_stats, labels) if want_labels else (out, out_stats)

    def merge_tree_from_arrival(self, keys, labels, n_seeds, max_level=254, weights=None, want_stats=False):
        """merge_tree -- with want_stats, merge_tree_stats -- of a segmenting transform that has already run, without a second
        flood (ws_merge_tree_from_arrival_device): keys = its arrival stamps (last_arrival()), labels = its labels, both 2-D int32
        device tensors of the (padded) plane's shape, contiguous (views into larger buffers are fine); n_seeds = the number of
        colours.  Returns the tree tensor of merge_tree, or (tree, stats) as merge_tree_stats.  weights (needed with want_stats:
        this form has no image): a uint8 or int16 / uint16 device tensor of the PLANE's shape with contiguous rows."""
        if keys.dim() != 2 or tuple(keys.shape) != tuple(labels.shape):
            raise ValueError("keys and labels must be 2-D tensors of the same shape")
        assert keys.dtype == torch.int32 and labels.dtype == torch.int32 and keys.is_cuda and labels.is_cuda
        assert keys.numel() == 0 or (keys.is_contiguous() and labels.is_contiguous())
        h, w = keys.shape
        ns = int(n_seeds)
        dtype, wstride = 0, 0
        if want_stats:
            if weights is None:
                raise ValueError("merge_tree_from_arrival has no image: the catalogue needs weights")
            u16 = {torch.int16, getattr(torch, "uint16", torch.int16)}
            if weights.dtype != torch.uint8 and weights.dtype not in u16:
                raise TypeError("weights must be a uint8, uint16 or int16 (u16 bits) tensor")
            if not weights.is_cuda or weights.dim() != 2 or tuple(weights.shape) != (h, w) or (w > 1 and weights.stride(1) != 1):
                raise ValueError(f"weights must be a device tensor of shape {(h, w)} with contiguous rows")
            dtype = _ffi.WS_DTYPES["uint8" if weights.dtype == torch.uint8 else "uint16"]
            wstride = weights.stride(0) if h > 1 else w
        out = torch.empty((ns + 1, 4), dtype=torch.int32, device=self.device)
        out_stats = torch.empty((ns + 1, 9), dtype=torch.int64, device=self.device) if want_stats else None
        opt = self.options(max_level, False)
        self.ctx.check(_ffi.lib().ws_merge_tree_from_arrival_device(self.ctx.handle, keys.data_ptr() if h * w else None,
                                                                    labels.data_ptr() if h * w else None, h, w, ns, ctypes.byref(opt),
                                                                    weights.data_ptr() if want_stats else None, dtype, wstride,
                                                                    out.data_ptr(), out_stats.data_ptr() if want_stats else None))
        return (out, out_stats) if want_stats else out

    @staticmethod
    def _weight_plane(weights, h, w):
        """(ws dtype, row stride in elements) of a 2-D device weight tensor of shape (h, w) with contiguous rows."""
        u16 = {torch.int16, getattr(torch, "uint16", torch.int16)}
        if weights.dtype != torch.uint8 and weights.dtype not in u16:
            raise TypeError("weights must be a uint8, uint16 or int16 (u16 bits) tensor")
        if not weights.is_cuda or weights.dim() != 2 or tuple(weights.shape) != (h, w) or (w > 1 and weights.stride(1) != 1):
            raise ValueError(f"weights must be a device tensor of shape {(h, w)} with contiguous rows")
        return _ffi.WS_DTYPES["uint8" if weights.dtype == torch.uint8 else "uint16"], (weights.stride(0) if h > 1 else w)

    def _records(self, out, shape, dtype, name):
        if out is None:
            return torch.empty(shape, dtype=dtype, device=self.device)
        if out.dtype != dtype or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape {shape}")
        return out

    def merge_tree_shapes(self, img, seeds, weights=None, max_level=254, edge=False, seed_shift=False, want_labels=False, out=None,
                          out_stats=None, out_shapes=None):
        """merge_tree_stats and the second moments of every lake from the same flood with everything in HBM
        (ws_merge_tree_shapes_device): the tree and stats tensors of merge_tree_stats and an (n_seeds + 1, 12) int64 tensor of raw
        ws_lake_shape words -- row c, the bits of colour c's 96 bytes: sum_wrr, sum_wcc, sum_wrc, sum_rr, sum_cc, sum_rc, each
        exact in 128 bits as (low, high) uint64 bits.  Arguments as merge_tree_stats; `out_shapes`: a reusable contiguous tensor
        of that shape (a view at an 8-byte offset is fine).  With want_labels returns (tree, stats, shapes, labels)."""
        assert img.dtype == torch.uint8 and img.dim() == 2 and img.is_contiguous() and img.is_cuda
        assert seeds.dtype == torch.int32 and seeds.is_cuda and (seeds.numel() == 0 or seeds.is_contiguous())
        h, w = img.shape
        ns = seeds.shape[0] if seeds.dim() == 2 else 0
        dtype, wstride = self._weight_plane(weights, h, w) if weights is not None else (0, 0)
        out = self._records(out, (ns + 1, 4), torch.int32, "out")
        out_stats = self._records(out_stats, (ns + 1, 9), torch.int64, "out_stats")
        out_shapes = self._records(out_shapes, (ns + 1, 12), torch.int64, "out_shapes")
        labels = torch.empty(self._plane(img, edge), dtype=torch.int32, device=self.device) if want_labels else None
        opt = self.options(max_level, edge, None, seed_shift)
        self.ctx.check(_ffi.lib().ws_merge_tree_shapes_device(self.ctx.handle, img.data_ptr(), h, w, w, seeds.data_ptr() if ns else None, ns,
                                                              ctypes.byref(opt), weights.data_ptr() if weights is not None else None, dtype,
                                                              wstride, out.data_ptr(), out_stats.data_ptr(), out_shapes.data_ptr(),
                                                              labels.data_ptr() if want_labels else None))
        return (out, out_stats, out_shapes, labels) if want_labels else (out, out_stats, out_shapes)

    def merge_tree_shapes_from_arrival(self, keys, labels, n_seeds, weights, max_level=254, out=None, out_stats=None, out_shapes=None):
        """merge_tree_shapes of a segmenting transform that has already run, without a second flood
        (ws_merge_tree_shapes_from_arrival_device): keys, labels, n_seeds and weights (required: this form has no image) as
        merge_tree_from_arrival with want_stats.  Returns (tree, stats, shapes) as merge_tree_shapes."""
        if keys.dim() != 2 or tuple(keys.shape) != tuple(labels.shape):
            raise ValueError("keys and labels must be 2-D tensors of the same shape")
        assert keys.dtype == torch.int32 and labels.dtype == torch.int32 and keys.is_cuda and labels.is_cuda
        assert keys.numel() == 0 or (keys.is_contiguous() and labels.is_contiguous())
        if weights is None:
            raise ValueError("merge_tree_shapes_from_arrival has no image: the moments need weights")
        h, w = keys.shape
        ns = int(n_seeds)
        dtype, wstride = self._weight_plane(weights, h, w)
        out = self._records(out, (ns + 1, 4), torch.int32, "out")
        out_stats = self._records(out_stats, (ns + 1, 9), torch.int64, "out_stats")
        out_shapes = self._records(out_shapes, (ns + 1, 12), torch.int64, "out_shapes")
        opt = self.options(max_level, False)
        self.ctx.check(_ffi.lib().ws_merge_tree_shapes_from_arrival_device(self.ctx.handle, keys.data_ptr() if h * w else None,
                                                                           labels.data_ptr() if h * w else None, h, w, ns,
                                                                           ctypes.byref(opt), weights.data_ptr(), dtype, wstride,
                                                                           out.data_ptr(), out_stats.data_ptr(), out_shapes.data_ptr()))
        return out, out_stats, out_shapes

    def tree_cut(self, tree, keys, labels, cuts, out=None, want_lakes=False, stats=None):
        """The label planes -- with want_lakes, also the lake lists -- of a merge tree pruned by `cuts` (an api.Cut or up to 32),
        everything in HBM (ws_tree_cut_device): tree = the (n_seeds + 1, 4) int32 tensor of merge_tree, keys = the arrival stamps
        (last_arrival()) and labels = the segmenting labels (merge_tree(want_labels=True)) of the same flood, 2-D int32 device
        tensors of one shape, contiguous (views into larger buffers are fine).  Returns a (K, H', W') int32 tensor whose plane k
        shows every pixel the lake cuts[k] leaves it in, 0 where it is hidden; with want_lakes (planes, lakes, offsets, hidden):
        lakes an (n, 2) int64 device tensor, lakes[offsets[k] : offsets[k + 1]] cut k's (colour, pixels) records in increasing
        colour, hidden[k] its pixels that show 0 (numpy).  `out`: a reusable contiguous (K, H', W') int32 device tensor.
        stats: the (n_seeds + 1, 9) int64 catalogue tensor of merge_tree_stats of the same flood (views into larger buffers are
        fine); with it the cuts may carry catalogue thresholds (min_sum_w, min_w_max, min_depth: ws_tree_cut_stats_device).  Such
        a cut without stats is a ValueError before any device work."""
        import numpy as np
        from .api import _as_cuts, _as_lake_cuts, _cut_list
        lst = _cut_list(cuts)
        if stats is None:
            if any(c.catalogue for c in lst):
                raise ValueError("a cut has a catalogue threshold: pass stats, the catalogue of merge_tree_stats")
            arr, k = _as_cuts(lst)
        else:
            arr, k = _as_lake_cuts(lst)
            if stats.dim() != 2 or tuple(stats.shape) != (tree.shape[0], 9):
                raise ValueError("stats must be an (n_seeds + 1, 9) tensor, one row per row of tree")
            assert stats.dtype == torch.int64 and stats.is_cuda and stats.is_contiguous()
        if keys.dim() != 2 or tuple(keys.shape) != tuple(labels.shape):
            raise ValueError("keys and labels must be 2-D tensors of the same shape")
        if tree.dim() != 2 or tree.shape[0] < 1 or tree.shape[1] != 4:
            raise ValueError("tree must be an (n_seeds + 1, 4) tensor")
        assert tree.dtype == torch.int32 and tree.is_cuda and tree.is_contiguous()
        assert keys.dtype == torch.int32 and labels.dtype == torch.int32 and keys.is_cuda and labels.is_cuda
        assert keys.numel() == 0 or (keys.is_contiguous() and labels.is_contiguous())
        h, w = keys.shape
        ns = tree.shape[0] - 1
        if out is None:
            out = torch.empty((k, h, w), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (k, h, w):
            raise ValueError(f"out must be a contiguous int32 tensor of shape {(k, h, w)}")
        offsets = np.zeros(k + 1, dtype=np.uint64)
        hidden = np.zeros(max(k, 1), dtype=np.uint64)
        n = ctypes.c_size_t(0)
        lakes = None
        cap = max(min(ns, h * w), 1) * max(k, 1) if want_lakes else 0      # a cut shows no more colours than there are, or pixels
        if want_lakes:
            lakes = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
        if k and h * w and stats is None:      # (no cut or no pixel: nothing to run, no plane word to write, empty lists)
            self.ctx.check(_ffi.lib().ws_tree_cut_device(self.ctx.handle, tree.data_ptr(), ns, keys.data_ptr(), labels.data_ptr(), h, w,
                                                         arr, k, out.data_ptr(), h * w, lakes.data_ptr() if want_lakes else None, cap,
                                                         ctypes.byref(n), offsets.ctypes.data, hidden.ctypes.data))
        elif k and h * w:
            self.ctx.check(_ffi.lib().ws_tree_cut_stats_device(self.ctx.handle, tree.data_ptr(), stats.data_ptr(), ns, keys.data_ptr(),
                                                               labels.data_ptr(), h, w, arr, k, out.data_ptr(), h * w,
                                                               lakes.data_ptr() if want_lakes else None, cap, ctypes.byref(n),
                                                               offsets.ctypes.data, hidden.ctypes.data))
        return (out, lakes[: n.value], offsets, hidden[:k]) if want_lakes else out

    def tree_cut_catalogue(self, tree, keys, labels, cuts, weights, stats=None, out=None, want_planes=True):
        """tree_cut(want_lakes=True) with the regions the cuts show measured in the same call, everything in HBM
        (ws_tree_cut_catalogue_device): returns (planes | None, lakes, region_stats, offsets, hidden, hidden_stats).  tree, keys,
        labels, cuts, stats and out as tree_cut, with the same checks; planes, lakes, offsets and hidden as it returns them
        (want_planes=False: no plane is rendered).  region_stats: an (n, 9) int64 device tensor of raw ws_lake_stats records as
        merge_tree_stats returns them, row i measured over the pixels lakes[i] counts -- the region of colour lakes[i, 0] in
        its cut, not the catalogue's record of that colour.  hidden_stats: a (K, 9) int64 numpy array, row k the same over the
        pixels cut k shows as 0.  weights: a 2-D uint8 or int16 / uint16 (taken as u16 bits) device tensor of the PLANE's shape
        (keys.shape: a padded plane comes with padded weights) whose rows are contiguous (a row stride in elements is honoured)."""
        import numpy as np
        from .api import _as_lake_cuts, _cut_list
        lst = _cut_list(cuts)
        if stats is None and any(c.catalogue for c in lst):
            raise ValueError("a cut has a catalogue threshold: pass stats, the catalogue of merge_tree_stats")
        arr, k = _as_lake_cuts(lst)
        if keys.dim() != 2 or tuple(keys.shape) != tuple(labels.shape):
            raise ValueError("keys and labels must be 2-D tensors of the same shape")
        if tree.dim() != 2 or tree.shape[0] < 1 or tree.shape[1] != 4:
            raise ValueError("tree must be an (n_seeds + 1, 4) tensor")
        if stats is not None:
            if stats.dim() != 2 or tuple(stats.shape) != (tree.shape[0], 9):
                raise ValueError("stats must be an (n_seeds + 1, 9) tensor, one row per row of tree")
            assert stats.dtype == torch.int64 and stats.is_cuda and stats.is_contiguous()
        assert tree.dtype == torch.int32 and tree.is_cuda and tree.is_contiguous()
        assert keys.dtype == torch.int32 and labels.dtype == torch.int32 and keys.is_cuda and labels.is_cuda
        assert keys.numel() == 0 or (keys.is_contiguous() and labels.is_contiguous())
        h, w = keys.shape
        ns = tree.shape[0] - 1
        u16 = {torch.int16, getattr(torch, "uint16", torch.int16)}
        if weights is None:
            raise ValueError("tree_cut_catalogue has no image: the records need weights")
        if weights.dtype != torch.uint8 and weights.dtype not in u16:
            raise TypeError("weights must be a uint8, uint16 or int16 (u16 bits) tensor")
        if not weights.is_cuda or weights.dim() != 2 or tuple(weights.shape) != (h, w) or (w > 1 and weights.stride(1) != 1):
            raise ValueError(f"weights must be a device tensor of shape {(h, w)} with contiguous rows")
        dtype = _ffi.WS_DTYPES["uint8" if weights.dtype == torch.uint8 else "uint16"]
        wstride = weights.stride(0) if h > 1 else w
        if not want_planes:
            out = None
        elif out is None:
            out = torch.empty((k, h, w), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (k, h, w):
            raise ValueError(f"out must be a contiguous int32 tensor of shape {(k, h, w)}")
        offsets = np.zeros(k + 1, dtype=np.uint64)
        hidden = np.zeros(max(k, 1), dtype=np.uint64)
        hidden_stats = np.zeros((max(k, 1), 9), dtype=np.int64)
        n = ctypes.c_size_t(0)
        cap = max(min(ns, h * w), 1) * max(k, 1)      # a cut shows no more colours than there are, or pixels
        lakes = torch.empty((cap, 2), dtype=torch.int64, device=self.device)
        region = torch.empty((cap, 9), dtype=torch.int64, device=self.device)
        if h * w == 0:      # (no pixel: nothing to run, empty lists, every hidden record the identity of the fold)
            hidden_stats[:] = (0, 0, 0, 0, 0, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
        elif k:
            self.ctx.check(_ffi.lib().ws_tree_cut_catalogue_device(self.ctx.handle, tree.data_ptr(), stats.data_ptr() if stats is not None else None,
                                                                   ns, keys.data_ptr(), labels.data_ptr(), h, w,
                                                                   weights.data_ptr(), dtype, wstride, arr, k, out.data_ptr() if want_planes else None,
                                                                   h * w, lakes.data_ptr(), region.data_ptr(), cap, ctypes.byref(n),
                                                                   offsets.ctypes.data, hidden.ctypes.data, hidden_stats.ctypes.data))
        return out, lakes[: n.value], region[: n.value], offsets, hidden[:k], hidden_stats[:k]

    def merge_tree_batch(self, cube, seeds, seed_offsets, max_level=254, edge=False, seed_shift=False, want_labels=False, out=None):
        """merge_tree of every slice of a cube with everything in HBM (ws_merge_tree_batch_device); cube, seeds and seed_offsets as
        transform_to_list_batch.  Returns an (n_seeds_total + S, 4) int32 tensor: slice k's n_k + 1 rows start at
        (seed_offsets[k] - seed_offsets[0]) + k, row c of them colour c of the slice's own colours as merge_tree's.  With
        want_labels also the segmenting (S, H', W') int32 labels: returns (tree, labels).  `out`: a reusable contiguous int32
        device tensor of that shape."""
        offs = self._batch_args(cube, seeds, seed_offsets)
        s, h, w = cube.shape
        e = 2 if edge else 0
        shape = (int(seed_offsets[-1]) - int(seed_offsets[0]) + s, 4)
        if out is None:
            out = torch.empty(shape, dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError(f"out must be a contiguous int32 tensor of shape {shape}")
        labels = torch.empty((s, h + e, w + e), dtype=torch.int32, device=self.device) if want_labels else None
        if s:
            opt = self.options(max_level, edge, None, seed_shift)
            failed = ctypes.c_size_t(0)
            self.ctx.check(_ffi.lib().ws_merge_tree_batch_device(self.ctx.handle, cube.data_ptr(), s, h, w, w, h * w,
                                                                 seeds.data_ptr() if seeds.numel() else None, offs, ctypes.byref(opt),
                                                                 out.data_ptr(), labels.data_ptr() if want_labels else None,
                                                                 ctypes.byref(failed)))
        return (out, labels) if want_labels else out

    def merge_tree_stats_batch(self, cube, seeds, seed_offsets, weights=None, max_level=254, edge=False, seed_shift=False,
                               want_labels=False, out=None, out_stats=None):
        """merge_tree_stats of every slice of a cube with everything in HBM (ws_merge_tree_stats_batch_device); cube, seeds and
        seed_offsets as merge_tree_batch.  Returns (tree, stats): the (n_seeds_total + S, 4) int32 tensor of merge_tree_batch and
        an (n_seeds_total + S, 9) int64 tensor of raw ws_lake_stats records as merge_tree_stats's, in the same slice-major layout
        -- every slice's records are those of merge_tree_stats on the slice alone.  weights: a 3-D uint8 or int16 / uint16 (taken
        as u16 bits) device tensor of the cube's shape whose rows are contiguous (row and slice strides in elements are
        honoured), None: the cube itself.  With want_labels returns (tree, stats, labels).  `out`, `out_stats`: reusable
        contiguous tensors of those shapes."""
        offs = self._batch_args(cube, seeds, seed_offsets)
        s, h, w = cube.shape
        e = 2 if edge else 0
        dtype, wrow, wslice = 0, 0, 0
        if weights is not None:
            u16 = {torch.int16, getattr(torch, "uint16", torch.int16)}
            if weights.dtype != torch.uint8 and weights.dtype not in u16:
                raise TypeError("weights must be a uint8, uint16 or int16 (u16 bits) tensor")
            if not weights.is_cuda or weights.dim() != 3 or tuple(weights.shape) != (s, h, w) or (w > 1 and weights.stride(2) != 1):
                raise ValueError(f"weights must be a device tensor of shape {(s, h, w)} with contiguous rows")
            dtype = _ffi.WS_DTYPES["uint8" if weights.dtype == torch.uint8 else "uint16"]
            wrow = weights.stride(1) if h > 1 else w
            wslice = weights.stride(0) if s > 1 else h * wrow
        total = int(seed_offsets[-1]) - int(seed_offsets[0]) + s
        if out is None:
            out = torch.empty((total, 4), dtype=torch.int32, device=self.device)
        elif out.dtype != torch.int32 or not out.is_contiguous() or tuple(out.shape) != (total, 4):
            raise ValueError(f"out must be a contiguous int32 tensor of shape {(total, 4)}")
        if out_stats is None:
            out_stats = torch.empty((total, 9), dtype=torch.int64, device=self.device)
        elif out_stats.dtype != torch.int64 or not out_stats.is_contiguous() or tuple(out_stats.shape) != (total, 9):
            raise ValueError(f"out_stats must be a contiguous int64 tensor of shape {(total, 9)}")
        labels = torch.empty((s, h + e, w + e), dtype=torch.int32, device=self.device) if want_labels else None
        if s:
            opt = self.options(max_level, edge, None, seed_shift)
            failed = ctypes.c_size_t(0)
            self.ctx.check(_ffi.lib().ws_merge_tree_stats_batch_device(self.ctx.handle, cube.data_ptr(), s, h, w, w, h * w,
                                                                       seeds.data_ptr() if seeds.numel() else None, offs, ctypes.byref(opt),
                                                                       weights.data_ptr() if weights is not None else None, dtype, wrow, wslice,
                                                                       out.data_ptr(), out_stats.data_ptr(),
                                                                       labels.data_ptr() if want_labels else None, ctypes.byref(failed)))
        return (out, out_stats, labels) if want_labels else (out, out_stats)

    def merge_tree_shapes_batch(self, cube, seeds, seed_offsets, weights=None, max_level=254, edge=False, seed_shift=False,
                                want_labels=False, out=None, out_stats=None, out_shapes=None):
        """merge_tree_shapes of every slice of a cube with everything in HBM (ws_merge_tree_shapes_batch_device); every argument
        as merge_tree_stats_batch.  Returns (tree, stats, shapes): the two tensors of merge_tree_stats_batch and an
        (n_seeds_total + S, 12) int64 tensor of raw ws_lake_shape words as merge_tree_shapes's, in the same slice-major layout --
        every slice's records are those of merge_tree_shapes on the slice alone.  With want_labels returns (tree, stats, shapes,
        labels).  `out`, `out_stats`, `out_shapes`: reusable contiguous tensors of those shapes."""
        offs = self._batch_args(cube, seeds, seed_offsets)
        s, h, w = cube.shape
        e = 2 if edge else 0
        wptr, dtype, wrow, wslice = self._cube_weights(weights, (s, h, w)) if weights is not None else (None, 0, 0, 0)
        total = int(seed_offsets[-1]) - int(seed_offsets[0]) + s
        out = self._records(out, (total, 4), torch.int32, "out")
        out_stats = self._records(out_stats, (total, 9), torch.int64, "out_stats")
        out_shapes = self._records(out_shapes, (total, 12), torch.int64, "out_shapes")
        labels = torch.empty((s, h + e, w + e), dtype=torch.int32, device=self.device) if want_labels else None
        if s:
            opt = self.options(max_level, edge, None, seed_shift)
            failed = ctypes.c_size_t(0)
            self.ctx.check(_ffi.lib().ws_merge_tree_shapes_batch_device(self.ctx.handle, cube.data_ptr(), s, h, w, w, h * w,
                                                                        seeds.data_ptr() if seeds.numel() else None, offs, ctypes.byref(opt),
                                                                        wptr, dtype, wrow, wslice, out.data_ptr(), out_stats.data_ptr(),
                                                                        out_shapes.data_ptr(), labels.data_ptr() if want_labels else None,
                                                                        ctypes.byref(failed)))
        return (out, out_stats, out_shapes, labels) if want_labels else (out, out_stats, out_shapes)

    @staticmethod
    def _cube_weights(weights, shape):
        """(pointer, dtype, row stride, slice stride) of a 3-D weight tensor of `shape` with contiguous rows."""
        s, h, w = shape
        u16 = {torch.int16, getattr(torch, "uint16", torch.int16)}
        if weights.dtype != torch.uint8 and weights.dtype not in u16:
            raise TypeError("weights must be a uint8, uint16 or int16 (u16 bits) tensor")
        if not weights.is_cuda or weights.dim() != 3 or tuple(weights.shape) != (s, h, w) or (w > 1 and weights.stride(2) != 1):
            raise ValueError(f"weights must be a device tensor of shape {(s, h, w)} with contiguous rows")
        wrow = weights.stride(1) if h > 1 else w
        return weights.data_ptr(), _ffi.WS_DTYPES["uint8" if weights.dtype == torch.uint8 else "uint16"], wrow, weights.stride(0) if s > 1 else h * wrow

    def tree_cut_catalogue_batch(self, tree, keys, labels, seed_offsets, cuts, weights=None, stats=None, want_planes=True, want_lakes=True,
                                 measure=True, cap=None):
        """tree_cut_catalogue of every slice of a cube in one call, from records and planes in HBM
        (ws_tree_cut_catalogue_batch_device).  tree (and stats, optional) in the slice-major layout of merge_tree(_stats)_batch;
        keys and labels: (S, H', W') int32 device tensors, contiguous; seed_offsets: S + 1 host integers; weights: an (S, H', W')
        uint8 or int16 / uint16 device tensor with contiguous rows (needed when measure).  Returns (planes | None, lakes,
        region_stats, offsets, hidden, hidden_stats): planes (S, K, H', W') int32; lakes (n, 2) int64 and region_stats (n, 9)
        int64 device tensors, list (k, j) at offsets[k * K + j] : offsets[k * K + j + 1] in slice k's own colours; offsets
        (S * K + 1), hidden (S * K) and hidden_stats (S * K, 9) numpy.  measure=False: no region or hidden records (None)."""
        import numpy as np
        from .api import _as_lake_cuts, _cut_list
        lst = _cut_list(cuts)
        if stats is None and any(c.catalogue for c in lst):
            raise ValueError("a cut has a catalogue threshold: pass stats, the catalogue of merge_tree_stats_batch")
        arr, k = _as_lake_cuts(lst)
        if keys.dim() != 3 or tuple(keys.shape) != tuple(labels.shape):
            raise ValueError("keys and labels must be 3-D tensors of the same shape")
        s, h, w = keys.shape
        offs = np.ascontiguousarray(np.asarray(seed_offsets, dtype=np.uint64))
        if offs.shape != (s + 1,):
            raise ValueError("seed_offsets must hold one entry per slice and one more")
        total = int(offs[-1]) - int(offs[0]) + s
        if tree.dim() != 2 or tuple(tree.shape) != (total, 4):
            raise ValueError(f"tree must be a {(total, 4)} tensor")
        assert tree.dtype == torch.int32 and tree.is_cuda and tree.is_contiguous()
        if stats is not None:
            if tuple(stats.shape) != (total, 9):
                raise ValueError(f"stats must be a {(total, 9)} tensor")
            assert stats.dtype == torch.int64 and stats.is_cuda and stats.is_contiguous()
        assert keys.dtype == torch.int32 and labels.dtype == torch.int32 and keys.is_cuda and labels.is_cuda
        assert keys.numel() == 0 or (keys.is_contiguous() and labels.is_contiguous())
        if not want_planes and not want_lakes:
            raise ValueError("nothing asked for: want_planes and want_lakes are both False")
        if measure and weights is None:
            raise ValueError("tree_cut_catalogue_batch has no image: the records need weights")
        wptr, dtype, wrow, wslice = self._cube_weights(weights, (s, h, w)) if measure else (None, 0, 0, 0)
        out = torch.empty((s, k, h, w), dtype=torch.int32, device=self.device) if want_planes else None
        offsets = np.zeros(s * k + 1, dtype=np.uint64)
        hidden = np.zeros(max(s * k, 1), dtype=np.uint64)
        hidden_stats = np.zeros((max(s * k, 1), 9), dtype=np.int64) if measure else None
        n = ctypes.c_size_t(0)
        if cap is None:
            cap = max(min(total - s, s * h * w), 1) * max(k, 1)
        lakes = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=self.device) if want_lakes else None
        region = torch.empty((max(cap, 1), 9), dtype=torch.int64, device=self.device) if want_lakes and measure else None
        self.ctx.check(_ffi.lib().ws_tree_cut_catalogue_batch_device(
            self.ctx.handle, tree.data_ptr(), stats.data_ptr() if stats is not None else None, s,
            offs.ctypes.data_as(ctypes.POINTER(ctypes.c_size_t)), keys.data_ptr(), labels.data_ptr(), h, w, wptr, dtype, wrow, wslice, arr, k,
            out.data_ptr() if want_planes else None, h * w, lakes.data_ptr() if want_lakes else None,
            region.data_ptr() if region is not None else None, cap if want_lakes else 0, ctypes.byref(n), offsets.ctypes.data, hidden.ctypes.data,
            hidden_stats.ctypes.data if measure else None))
        return (out, lakes[: n.value] if want_lakes else None, region[: n.value] if region is not None else None, offsets, hidden[: s * k],
                hidden_stats[: s * k] if measure else None)

    def merge_tree_cut_catalogue_batch(self, cube, seeds, seed_offsets, cuts, weights=None, max_level=254, edge=False, seed_shift=False,
                                       want_stats=True, want_labels=False, want_keys=False, want_planes=True, want_lakes=True, measure=True,
                                       cap=None):
        """Cube in, everything out (ws_merge_tree_cut_catalogue_batch_device): the trees (and with want_stats the catalogues) of
        merge_tree_stats_batch and the cut catalogue of every slice in one call, each stacked group cut while its stamps are on
        the device.  cube, seeds, seed_offsets and weights (None: the cube itself) as merge_tree_stats_batch; cuts as
        tree_cut_catalogue_batch.  Returns a dict: tree, stats (None without want_stats), labels and keys ((S, H', W') int32, when
        asked: what tree_cut_catalogue_batch needs to cut the same flood again), planes ((S, K, H', W') | None), lakes,
        region_stats, offsets, hidden, hidden_stats, and `slices`: per slice a tuple (planes, lakes, region_stats, offsets,
        hidden, hidden_stats) of views, offsets from 0, as tree_cut_catalogue returns them."""
        import numpy as np
        from .api import _as_lake_cuts, _cut_list
        lst = _cut_list(cuts)
        if not want_stats and any(c.catalogue for c in lst):
            raise ValueError("a cut has a catalogue threshold: the catalogue is needed (want_stats)")
        arr, k = _as_lake_cuts(lst)
        offs = self._batch_args(cube, seeds, seed_offsets)
        s, h, w = cube.shape
        e = 2 if edge else 0
        ph, pw = h + e, w + e
        if not want_planes and not want_lakes:
            raise ValueError("nothing asked for: want_planes and want_lakes are both False")
        wptr, dtype, wrow, wslice = self._cube_weights(weights, (s, h, w)) if weights is not None else (None, 0, 0, 0)
        total = int(seed_offsets[-1]) - int(seed_offsets[0]) + s
        tree = torch.empty((total, 4), dtype=torch.int32, device=self.device)
        stats = torch.empty((total, 9), dtype=torch.int64, device=self.device) if want_stats else None
        labels = torch.empty((s, ph, pw), dtype=torch.int32, device=self.device) if want_labels else None
        keys = torch.empty((s, ph, pw), dtype=torch.int32, device=self.device) if want_keys else None
        out = torch.empty((s, k, ph, pw), dtype=torch.int32, device=self.device) if want_planes else None
        offsets = np.zeros(s * k + 1, dtype=np.uint64)
        hidden = np.zeros(max(s * k, 1), dtype=np.uint64)
        hidden_stats = np.zeros((max(s * k, 1), 9), dtype=np.int64) if measure else None
        n = ctypes.c_size_t(0)
        if cap is None:
            cap = max(min(total - s, s * ph * pw), 1) * max(k, 1)
        lakes = torch.empty((max(cap, 1), 2), dtype=torch.int64, device=self.device) if want_lakes else None
        region = torch.empty((max(cap, 1), 9), dtype=torch.int64, device=self.device) if want_lakes and measure else None
        opt = self.options(max_level, edge, None, seed_shift)
        failed = ctypes.c_size_t(0)
        self.ctx.check(_ffi.lib().ws_merge_tree_cut_catalogue_batch_device(
            self.ctx.handle, cube.data_ptr(), s, h, w, w, h * w, seeds.data_ptr() if seeds.numel() else None, offs, ctypes.byref(opt),
            wptr, dtype, wrow, wslice, arr, k, tree.data_ptr(), stats.data_ptr() if want_stats else None,
            labels.data_ptr() if want_labels else None, keys.data_ptr() if want_keys else None, out.data_ptr() if want_planes else None, ph * pw,
            lakes.data_ptr() if want_lakes else None, region.data_ptr() if region is not None else None, cap if want_lakes else 0, ctypes.byref(n),
            offsets.ctypes.data, hidden.ctypes.data, hidden_stats.ctypes.data if measure else None, ctypes.byref(failed)))
        res = dict(tree=tree, stats=stats, labels=labels, keys=keys, planes=out, lakes=lakes[: n.value] if want_lakes else None,
                   region_stats=region[: n.value] if region is not None else None, offsets=offsets, hidden=hidden[: s * k],
                   hidden_stats=hidden_stats[: s * k] if measure else None)
        per = []
        for i in range(s):
            lo, hi = int(offsets[i * k]), int(offsets[(i + 1) * k])
            per.append((out[i] if want_planes else None, res["lakes"][lo:hi] if want_lakes else None,
                        res["region_stats"][lo:hi] if region is not None else None, offsets[i * k: (i + 1) * k + 1] - offsets[i * k],
                        hidden[i * k: (i + 1) * k], hidden_stats[i * k: (i + 1) * k] if measure else None))
        res["slices"] = per
        return res

    def stats(self):
        return self.ctx.stats()
