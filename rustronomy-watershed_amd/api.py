"""Host-side mirror of the reference's public interface for the watershed path.

Same names, argument meaning and error behaviour as rustronomy-watershed v0.4.1
(`TransformBuilder`, `BuildErr`, `HookCtx`, `Watershed` trait methods, `WatershedUtils::
find_local_minima`; "lib.rs:N" = src/lib.rs line N of the reference), implemented over the
C-ABI in include/ws_hip.h.  All compute happens in the HIP engine; this file only moves
numpy arrays across the boundary.

Documented deviations:
  * tie-break where lakes meet: first coloured neighbour in down,right,left,up order (the
    reference picks at random among them, lib.rs:249-253);
  * `SegmentingWatershed.transform` returns the labels after the last level (the reference
    panics at lib.rs:1821);
  * merged-lake ids are canonical (smallest seed colour in the lake) where the reference's are
    arbitrary.
"""
import ctypes

import numpy as np

from . import _ffi

UNCOLOURED = 0          # lib.rs:138
NORMAL_MAX = 254        # lib.rs:139
ALWAYS_FILL = 0         # lib.rs:140
NEVER_FILL = 255        # lib.rs:141

ENGINE_AUTO, ENGINE_FUSED, ENGINE_SWEEP = _ffi.WS_ENGINE_AUTO, _ffi.WS_ENGINE_FUSED, _ffi.WS_ENGINE_SWEEP


class WatershedError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = _ffi.lib().ws_strerror(status).decode()
        super().__init__(f"{msg} ({status})" + (f": {detail}" if detail else ""))


class BuildErr(ValueError):
    """lib.rs:1051-1065"""


class MaxToHigh(BuildErr):
    def __init__(self, v):
        self.value = v
        super().__init__(f"Maximum water level set to {v}, which is higher than the maximum allowed value {NORMAL_MAX}")


class MaxToLow(BuildErr):
    def __init__(self, v):
        self.value = v
        # the reference's message names NEVER_FILL here (lib.rs:1062); kept verbatim in meaning
        super().__init__(f"Maximum water level set to {v}, which is lower than the minimum allowed value {NEVER_FILL}")


class SeedOutOfBounds(IndexError):
    """the reference panics with an ndarray index error (lib.rs:1366 / 1676)"""


class HookCtx:
    """lib.rs:844-862"""
    __slots__ = ("water_level", "max_water_level", "image", "colours", "seeds")

    def __init__(self, water_level, max_water_level, image, colours, seeds):
        self.water_level = water_level
        self.max_water_level = max_water_level
        self.image = image
        self.colours = colours
        self.seeds = seeds


class Context:
    """One ws_ctx: a HIP stream plus reusable device workspaces.  Not thread safe."""

    def __init__(self, device=0, stream=None):
        self._h = ctypes.c_void_p()
        L = _ffi.lib()
        rc = (L.ws_ctx_create(device, ctypes.byref(self._h)) if stream is None
              else L.ws_ctx_create_on_stream(device, ctypes.c_void_p(stream), ctypes.byref(self._h)))
        if rc != _ffi.WS_OK:
            self._h = ctypes.c_void_p()
            raise WatershedError(rc, "ws_ctx_create")
        self.device = device

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            _ffi.lib().ws_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc == _ffi.WS_OK:
            return
        detail = _ffi.lib().ws_last_error(self._h).decode()
        if rc == _ffi.WS_ERR_SEED_OOB:
            raise SeedOutOfBounds(detail)
        raise WatershedError(rc, detail)

    def set_profiling(self, on):
        self.check(_ffi.lib().ws_ctx_set_profiling(self._h, int(on)))

    def stats(self):
        st = _ffi.Stats()
        self.check(_ffi.lib().ws_ctx_get_stats(self._h, ctypes.byref(st)))
        return st.as_dict()

    def synchronize(self):
        self.check(_ffi.lib().ws_ctx_synchronize(self._h))

    def set_batch_pixel_limit(self, max_px):
        self.check(_ffi.lib().ws_ctx_set_batch_pixel_limit(self._h, int(max_px)))

    def set_seam_repair_min_pixels(self, min_px):
        self.check(_ffi.lib().ws_ctx_set_seam_repair_min_pixels(self._h, int(min_px)))


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


def _as_image(img):
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise TypeError("input must be a 2-D uint8 array (ndarray::ArrayView2<u8>)")
    if a.strides[1] != 1 or (a.shape[0] > 1 and a.strides[0] < a.shape[1]):
        a = np.ascontiguousarray(a)          # the Rust shim calls as_standard_layout() likewise
    stride = a.strides[0] if a.shape[0] > 1 else max(a.shape[1], 1)
    return a, int(stride)


def _as_seeds(seeds):
    s = np.ascontiguousarray(np.asarray(seeds, dtype=np.uint64).reshape(-1, 2))
    return s, int(s.shape[0])


def _history_levels(levels, max_level):
    """The level list of a transform_history for chosen levels (ws_transform_history(_device)) as u8, checked before any device
    work: None = every level 0..=max_level; otherwise at most 256 integers in 0..=max_level, any order, repeats allowed."""
    if levels is None:
        return np.arange(int(max_level) + 1, dtype=np.uint8)
    lv = np.asarray(levels).reshape(-1)
    if lv.size == 0:
        return np.zeros(0, dtype=np.uint8)
    if not np.issubdtype(lv.dtype, np.integer):
        raise ValueError("water levels must be integers")
    if lv.size > 256:
        raise ValueError(f"at most 256 water levels per call, not {lv.size}")
    if int(lv.min()) < 0 or int(lv.max()) > int(max_level):
        raise ValueError(f"water levels must lie in 0..={int(max_level)} (max_water_level)")
    return np.ascontiguousarray(lv, dtype=np.uint8)


LAKE_STATS_DTYPE = np.dtype([("sum_w", "<u8"), ("sum_wr", "<u8"), ("sum_wc", "<u8"), ("sum_r", "<u8"), ("sum_c", "<u8"),
                             ("r_min", "<u4"), ("r_max", "<u4"), ("c_min", "<u4"), ("c_max", "<u4"), ("w_min", "<u4"), ("w_max", "<u4"),
                             ("peak_pixel", "<u4"), ("reserved", "<u4")])      # ws_lake_stats, 72 bytes


def _as_weights(weights, shape):
    """(array or None, ws_dtype, row stride in elements) of a weight plane for ws_merge_tree_stats: u8 or u16, the image's shape."""
    if weights is None:
        return None, 0, 0
    a = np.asarray(weights)
    if a.dtype not in (np.uint8, np.uint16) or a.ndim != 2:
        raise TypeError("weights must be a 2-D uint8 or uint16 array (quantise float data first: pre_processor_with_max)")
    if a.shape != tuple(shape):
        raise ValueError(f"weights must have the image's shape {tuple(shape)}, not {a.shape}")
    item = a.dtype.itemsize
    if a.size and (a.strides[1] != item or a.strides[0] % item or a.strides[0] < a.shape[1] * item):
        a = np.ascontiguousarray(a)
    return a, _ffi.WS_DTYPES[a.dtype.name], (a.strides[0] // item if a.size else a.shape[1])


LAKE_SHAPE_DTYPE = np.dtype([("sum_wrr", "<u8", (2,)), ("sum_wcc", "<u8", (2,)), ("sum_wrc", "<u8", (2,)), ("sum_rr", "<u8", (2,)),
                             ("sum_cc", "<u8", (2,)), ("sum_rc", "<u8", (2,))])      # ws_lake_shape, 96 bytes: (low, high) of six 128-bit sums


def _wide(words):
    """An (n, 2) array of (low, high) u64 words as an object array of Python ints."""
    w = np.asarray(words)
    return np.array([int(lo) | int(hi) << 64 for lo, hi in w.reshape(-1, 2)], dtype=object)


def ellipses(stats, shapes, weighted=True, area=None):
    """(var_r, var_c, cov_rc, major_sigma, minor_sigma, angle) float64 arrays: the second central moments of every record of
    merge_tree_shapes about its own centroid, the sigmas of its ellipse and the direction of its major axis, in the coordinates
    of the padded plane.  Weighted, with S = sum_w: var_r = (S sum_wrr - sum_wr^2) / S^2, cov_rc = (S sum_wrc - sum_wr sum_wc) /
    S^2.  weighted=False: the same of the plain sums with S = `area` (MergeTree.area, the pixels the record counts; needed then).
    Numerator and denominator are exact Python integers divided once, so each moment is the correctly rounded value.  With a =
    var_r, c = var_c, b = cov_rc: lambda+- = (a + c) / 2 +- sqrt(((a - c) / 2)^2 + b^2), sigma = sqrt(lambda+-), angle =
    atan2(2 b, a - c) / 2 -- the major axis measured from the row axis towards the column axis, in (-pi/2, pi/2].  nan where
    S == 0."""
    n = len(shapes)
    if weighted:
        s0 = [int(x) for x in stats["sum_w"]]
        s_r, s_c = [int(x) for x in stats["sum_wr"]], [int(x) for x in stats["sum_wc"]]
        rr, cc, rc = _wide(shapes["sum_wrr"]), _wide(shapes["sum_wcc"]), _wide(shapes["sum_wrc"])
    else:
        if area is None:
            raise ValueError("weighted=False needs area: the pixels every record counts (MergeTree.area)")
        s0 = [int(x) for x in area]
        s_r, s_c = [int(x) for x in stats["sum_r"]], [int(x) for x in stats["sum_c"]]
        rr, cc, rc = _wide(shapes["sum_rr"]), _wide(shapes["sum_cc"]), _wide(shapes["sum_rc"])
    if not (len(s0) == n == len(stats)):
        raise ValueError("stats, shapes and area must have one record per colour")
    var_r, var_c, cov = np.full(n, np.nan), np.full(n, np.nan), np.full(n, np.nan)
    for i in range(n):
        S = s0[i]
        if S == 0:
            continue
        den = S * S
        var_r[i] = (S * rr[i] - s_r[i] * s_r[i]) / den      # (int / int rounds once)
        var_c[i] = (S * cc[i] - s_c[i] * s_c[i]) / den
        cov[i] = (S * rc[i] - s_r[i] * s_c[i]) / den
    root = np.hypot((var_r - var_c) / 2, cov)
    mid = (var_r + var_c) / 2
    major = np.sqrt(mid + root)
    minor = np.sqrt(np.maximum(mid - root, 0.0))      # (rounding may leave a line's minor axis a hair below 0; nan stays nan)
    angle = 0.5 * np.arctan2(2 * cov, var_r - var_c)
    return var_r, var_c, cov, major, minor, angle


def centroids(stats):
    """(row, col) float64 arrays: the weighted centroid sum_wr / sum_w, sum_wc / sum_w of every record of merge_tree_stats, in the
    coordinates of the padded plane; nan where sum_w == 0."""
    sw = stats["sum_w"].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        row = np.where(sw > 0, stats["sum_wr"].astype(np.float64) / sw, np.nan)
        col = np.where(sw > 0, stats["sum_wc"].astype(np.float64) / sw, np.nan)
    return row, col


class Cut:
    """One cut of a merge tree (ws_tree_cut): a swallowed lake stands on its own iff it had reached `min_area` pixels and
    `min_leaves` seed colours; pixels that arrive after `show_level` are 0; every merge up to `merge_level` is applied.
    Checked here, before any device work.  Cut(show_level=L, merge_level=L) is the merging history plane of level L.
    With a lake catalogue (ws_lake_cut) three more thresholds: the lake's weights summed to `min_sum_w` (64 bits), its largest
    weight reached `min_w_max`, and it died `min_depth` above its smallest weight."""
    __slots__ = ("min_area", "min_leaves", "show_level", "merge_level", "min_sum_w", "min_w_max", "min_depth")

    def __init__(self, min_area=0, min_leaves=0, show_level=254, merge_level=0, min_sum_w=0, min_w_max=0, min_depth=0):
        for name, v, top in (("min_area", min_area, 0xFFFFFFFF), ("min_leaves", min_leaves, 0xFFFFFFFF),
                             ("show_level", show_level, 254), ("merge_level", merge_level, 254),
                             ("min_sum_w", min_sum_w, 0xFFFFFFFFFFFFFFFF), ("min_w_max", min_w_max, 0xFFFFFFFF),
                             ("min_depth", min_depth, 0xFFFFFFFF)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise TypeError(f"{name} must be an integer")
            if not 0 <= int(v) <= top:
                raise ValueError(f"{name} must lie in 0..={top}, not {v}")
            object.__setattr__(self, name, int(v))

    def __setattr__(self, name, value):
        raise AttributeError("a Cut is immutable")

    @property
    def catalogue(self):
        """Whether the cut has a threshold on a catalogue quantity (and so needs the lake statistics)."""
        return bool(self.min_sum_w or self.min_w_max or self.min_depth)

    def __repr__(self):
        more = f", min_sum_w={self.min_sum_w}, min_w_max={self.min_w_max}, min_depth={self.min_depth}" if self.catalogue else ""
        return f"Cut(min_area={self.min_area}, min_leaves={self.min_leaves}, show_level={self.show_level}, merge_level={self.merge_level}{more})"

    def __eq__(self, other):
        return isinstance(other, Cut) and all(getattr(self, k) == getattr(other, k) for k in self.__slots__)

    def __hash__(self):
        return hash(tuple(getattr(self, k) for k in self.__slots__))


def _cut_list(cuts):
    """The Cut values of a Cut or a sequence of at most 32 of them, checked before any device work."""
    lst = [cuts] if isinstance(cuts, Cut) else list(cuts)
    if len(lst) > 32:
        raise ValueError(f"at most 32 cuts per call, not {len(lst)}")
    for c in lst:
        if not isinstance(c, Cut):
            raise TypeError("cuts must be Cut values")
    return lst


def _as_cuts(cuts):
    """(ctypes array of ws_tree_cut, n) of a Cut or a sequence of at most 32 of them, none with a catalogue threshold."""
    lst = _cut_list(cuts)
    if any(c.catalogue for c in lst):
        raise ValueError("a cut has a catalogue threshold: this call takes none")
    arr = (_ffi.TreeCut * max(len(lst), 1))()
    for k, c in enumerate(lst):
        arr[k].min_area, arr[k].min_leaves, arr[k].show_level, arr[k].merge_level = c.min_area, c.min_leaves, c.show_level, c.merge_level
    return arr, len(lst)


def _as_lake_cuts(cuts):
    """(ctypes array of ws_lake_cut, n) of a Cut or a sequence of at most 32 of them."""
    lst = _cut_list(cuts)
    arr = (_ffi.LakeCut * max(len(lst), 1))()
    for k, c in enumerate(lst):
        arr[k].min_area, arr[k].min_leaves, arr[k].show_level, arr[k].merge_level = c.min_area, c.min_leaves, c.show_level, c.merge_level
        arr[k].min_sum_w, arr[k].min_w_max, arr[k].min_depth = c.min_sum_w, c.min_w_max, c.min_depth
    return arr, len(lst)


class MergeTree:
    """The merging transform's lake hierarchy (ws_merge_tree): numpy arrays indexed by seed colour, 0 .. n_seeds.
    `parent`: canonical id of the lake that swallowed the colour (0: none); `death_level`: the first water level after which the
    colour is no lake of its own (ALIVE: none); `area`, `n_leaves`: pixels and seed colours of the lake while it was last its
    own.  `labels`: the segmenting label plane the colours refer to, when it was asked for."""
    ALIVE = _ffi.WS_TREE_ALIVE
    __slots__ = ("parent", "death_level", "area", "n_leaves", "labels")

    def __init__(self, parent, death_level, area, n_leaves, labels=None):
        self.parent = np.asarray(parent, dtype=np.uint32)
        self.death_level = np.asarray(death_level, dtype=np.uint32)
        self.area = np.asarray(area, dtype=np.uint32)
        self.n_leaves = np.asarray(n_leaves, dtype=np.uint32)
        self.labels = labels

    def roots_at(self, level):
        """colour -> canonical id of its lake after water level `level`: follow `parent` while death_level <= level.
        roots_at(L)[labels] is the merging label plane of level L wherever that plane is coloured."""
        root = np.arange(self.parent.size, dtype=np.uint32)
        dead = self.death_level[root] <= level
        while dead.any():          # parents die strictly later: at most one step per level
            root[dead] = self.parent[root[dead]]
            dead = self.death_level[root] <= level
        return root

    def cut_table(self, cut, stats=None):
        """colour -> the first node of its parent chain that `cut` keeps: alive, or area >= min_area and n_leaves >= min_leaves
        -- and, for a cut with catalogue thresholds, stats (the records of merge_tree_stats) with sum_w >= min_sum_w, w_max >=
        min_w_max and depth >= min_depth, depth = death_level - w_min where that is positive, else 0.
        A pixel of colour c that arrived at level t then shows the end of the walk from cut_table(cut)[c] along `parent` while
        death_level <= max(t, cut.merge_level) (ws_tree_cut_device, ws_tree_cut_stats_device)."""
        if cut.catalogue and stats is None:
            raise ValueError("a cut with a catalogue threshold needs the lake statistics")
        node = np.arange(self.parent.size, dtype=np.uint32)
        keep = (self.death_level == self.ALIVE) | ((self.area >= cut.min_area) & (self.n_leaves >= cut.min_leaves))
        if cut.catalogue:
            death, w_min = self.death_level.astype(np.int64), stats["w_min"].astype(np.int64)
            depth = np.where((self.death_level != self.ALIVE) & (death > w_min), death - w_min, 0)
            keep &= (self.death_level == self.ALIVE) | ((stats["sum_w"] >= np.uint64(cut.min_sum_w)) & (stats["w_max"] >= cut.min_w_max) &
                                                         (depth >= cut.min_depth))
        gone = ~keep[node]
        while gone.any():          # the chain ends alive: at most one step per level
            node[gone] = self.parent[node[gone]]
            gone = ~keep[node]
        return node

    def children(self):
        """{colour: sorted array of the colours it swallowed}, for the colours that swallowed any."""
        dying = np.flatnonzero(self.death_level != self.ALIVE)
        order = dying[np.argsort(self.parent[dying], kind="stable")]
        keys, first = np.unique(self.parent[order], return_index=True)
        return {int(k): part for k, part in zip(keys, np.split(order, first[1:]))}


class TransformBuilder:
    """lib.rs:908-1047.  `TransformBuilder()` is both `new()` and `default()`."""

    def __init__(self):
        self.max_water_level = NORMAL_MAX     # lib.rs:942
        self.edge_correction = False          # lib.rs:943
        self.wlvl_hook = None                 # lib.rs:944
        self.engine = ENGINE_AUTO
        self.context = None
        self.seed_shift = False               # lib.rs:1675-1677: seeds are NOT moved into the padded plane

    @classmethod
    def new(cls):
        return cls()

    @classmethod
    def default(cls):
        return cls()

    def set_max_water_lvl(self, max_water_lvl):          # lib.rs:950
        if not 0 <= int(max_water_lvl) <= 255:
            raise OverflowError("max_water_lvl must fit a u8")
        self.max_water_level = int(max_water_lvl)
        return self

    def enable_edge_correction(self):                    # lib.rs:958
        self.edge_correction = True
        return self

    def set_wlvl_hook(self, hook):                       # lib.rs:967
        self.wlvl_hook = hook
        return self

    # not in the reference: engine / context selection of this implementation
    def set_engine(self, engine):
        self.engine = engine
        return self

    def set_context(self, ctx):
        self.context = ctx
        return self

    def shift_seeds_into_padded_plane(self, on=True):
        """Not in the reference (ws_options.seed_shift): with edge correction, move every seed by (+1, +1) onto the
        pixel it was found at, instead of indexing the padded plane with the caller's coordinates (lib.rs:1675-1677)."""
        self.seed_shift = bool(on)
        return self

    def _validate(self):
        opt = _ffi.Options(self.max_water_level, int(self.edge_correction), self.engine, 0, int(self.seed_shift))
        rc = _ffi.lib().ws_options_validate(ctypes.byref(opt))
        if rc == _ffi.WS_ERR_MAX_TOO_HIGH:
            raise MaxToHigh(self.max_water_level)         # lib.rs:1026-1027
        if rc == _ffi.WS_ERR_MAX_TOO_LOW:
            raise MaxToLow(self.max_water_level)          # lib.rs:1028-1029
        if rc != _ffi.WS_OK:
            raise WatershedError(rc, "ws_options_validate")
        return opt

    def build_segmenting(self):                           # lib.rs:1024-1046
        return SegmentingWatershed(self._validate(), self.wlvl_hook, self.context)

    def build_merging(self):                              # lib.rs:998-1020
        return MergingWatershed(self._validate(), self.wlvl_hook, self.context)


class WatershedUtils:
    """lib.rs:1069-1198"""

    def pre_processor(self, img):
        """lib.rs:1081-1087: any numeric array -> u8 in [0, NORMAL_MAX]; NaN / -inf / subnormals / exact 0 ->
        NEVER_FILL, +inf -> ALWAYS_FILL (as the code does, whatever its comments say)."""
        return self.pre_processor_with_max(img, NORMAL_MAX)

    def pre_processor_with_max(self, img, max_value):
        """lib.rs:1134-1173 (`pre_processor_with_max::<MAX, _, _>`); any dimension."""
        a = np.ascontiguousarray(img)
        if a.dtype.name not in _ffi.WS_DTYPES:
            raise TypeError(f"unsupported dtype {a.dtype} (supported: {sorted(_ffi.WS_DTYPES)})")
        if not 0 <= int(max_value) <= 255:
            raise OverflowError("MAX must fit a u8")
        if int(max_value) >= NEVER_FILL or int(max_value) <= ALWAYS_FILL:
            raise AssertionError("MAX must be in 1..=254 (lib.rs:1143-1144)")      # the reference asserts
        ctx = self._ctx()
        out = np.empty(a.shape, dtype=np.uint8)
        rc = _ffi.lib().ws_pre_processor(ctx.handle, a.ctypes.data, _ffi.WS_DTYPES[a.dtype.name], a.size, int(max_value),
                                         out.ctypes.data)
        ctx.check(rc)
        return out

    def find_local_minima(self, img):
        """Strict 8-neighbour local MAXIMA of the interior, row-major (lib.rs:1178-1197).
        Returns an (n, 2) uint64 array of (row, col)."""
        a, stride = _as_image(img)
        h, w = a.shape
        ctx = self._ctx()
        cap = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1)
        out = np.empty((max(cap, 1), 2), dtype=np.uint64)
        n = ctypes.c_size_t(0)
        rc = _ffi.lib().ws_find_local_minima(ctx.handle, a.ctypes.data, h, w, stride, out.ctypes.data, cap,
                                             ctypes.byref(n))
        ctx.check(rc)
        return out[: n.value].copy()

    def pre_processor_cube(self, cube, axis=0):
        """pre_processor of every slice `cube.take(k, axis)` of a 3-D cube as one call (ws_pre_processor_batch): each slice is
        normalised with its OWN zero-seeded (min, max).  Returns the contiguous (n_slices, h, w) uint8 cube the *_cube methods take."""
        return self.pre_processor_with_max_cube(cube, NORMAL_MAX, axis)

    def pre_processor_with_max_cube(self, cube, max_value, axis=0):
        """pre_processor_with_max of every slice along `axis` (tests/integration.rs:267-290 slice a FITS cube along its LAST axis:
        axis=2).  Any numpy strides that are non-negative multiples of the item size go to the engine as they are -- a channel-last
        cube is not copied into planes first; anything else is copied contiguous."""
        a = np.asarray(cube)
        if a.ndim != 3:
            raise ValueError("cube must be 3-D")
        if a.dtype.name not in _ffi.WS_DTYPES:
            raise TypeError(f"unsupported dtype {a.dtype} (supported: {sorted(_ffi.WS_DTYPES)})")
        if not 0 <= int(max_value) <= 255:
            raise OverflowError("MAX must fit a u8")
        if int(max_value) >= NEVER_FILL or int(max_value) <= ALWAYS_FILL:
            raise AssertionError("MAX must be in 1..=254 (lib.rs:1143-1144)")      # the reference asserts
        a = np.moveaxis(a, axis, 0)
        item = a.dtype.itemsize
        if any(st < 0 or st % item for st in a.strides):
            a = np.ascontiguousarray(a)
        n, h, w = a.shape
        ss, rs, cs = (st // item for st in a.strides)
        ctx = self._ctx()
        out = np.empty((n, h, w), dtype=np.uint8)
        failed = ctypes.c_size_t(0)
        rc = _ffi.lib().ws_pre_processor_batch(ctx.handle, a.ctypes.data, _ffi.WS_DTYPES[a.dtype.name], n, h, w, ss, rs, cs, int(max_value),
                                               out.ctypes.data, None, ctypes.byref(failed))
        if rc == _ffi.WS_ERR_UNSUPPORTED:
            raise WatershedError(rc, f"slice {failed.value}: " + _ffi.lib().ws_last_error(ctx.handle).decode())
        ctx.check(rc)
        return out

    def find_local_minima_cube(self, cube):
        """find_local_minima of every slice of a (n_slices, h, w) uint8 cube as one call (ws_find_local_minima_batch).  Returns
        (seeds, offsets): the slices' (row, col) pairs back to back as an (n, 2) uint64 array, coordinates local to the slice,
        and n_slices + 1 offsets -- slice k's seeds are seeds[offsets[k]:offsets[k + 1]], what the *_cube methods take."""
        a = np.asarray(cube)
        if a.dtype != np.uint8 or a.ndim != 3:
            raise TypeError("cube must be a 3-D uint8 array")
        a = np.ascontiguousarray(a)
        n, h, w = a.shape
        ctx = self._ctx()
        cap = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1) * n
        out = np.empty((max(cap, 1), 2), dtype=np.uint64)
        offsets = np.zeros(n + 1, dtype=np.uintp)
        found = ctypes.c_size_t(0)
        rc = _ffi.lib().ws_find_local_minima_batch(ctx.handle, a.ctypes.data, n, h, w, w, h * w, out.ctypes.data, cap,
                                                   offsets.ctypes.data_as(_ffi.szp), ctypes.byref(found))
        ctx.check(rc)
        return out[: found.value].copy(), offsets.astype(np.uint64)


class _Transform(WatershedUtils):
    _merging = False

    def __init__(self, opt, hook, ctx):
        self._opt = opt
        self.max_water_level = opt.max_water_level
        self.edge_correction = bool(opt.edge_correction)
        self.wlvl_hook = hook
        self._context = ctx

    def _ctx(self):
        return self._context if self._context is not None else default_context()

    def _shape(self, a):
        e = 2 if self.edge_correction else 0
        return a.shape[0] + e, a.shape[1] + e

    def _run_with_hook(self, img, seeds, hook, want_final):
        a, stride = _as_image(img)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        ph, pw = self._shape(a)
        ctx = self._ctx()
        results = []
        seed_colours = None
        cb = None
        if hook is not None:
            seed_colours = [(i + 1, (int(r), int(c))) for i, (r, c) in enumerate(s)]   # lib.rs:1671-1672

            def _cb(_user, lvl, mx, pimg, plab, hh, ww):
                image = np.ctypeslib.as_array(pimg, shape=(hh, ww))
                colours = np.ctypeslib.as_array(plab, shape=(hh, ww))
                results.append(hook(HookCtx(lvl, mx, image, colours, seed_colours)))
            cb = _ffi.LEVEL_CB(_cb)
        out = np.empty((ph, pw), dtype=np.uint64) if want_final else None
        fn = _ffi.lib().ws_merge_with_hook if self._merging else _ffi.lib().ws_segment_with_hook
        rc = fn(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                ctypes.cast(cb, ctypes.c_void_p) if cb else None, None, out.ctypes.data if want_final else None)
        ctx.check(rc)
        return results, out

    def transform_with_hook(self, input, seeds):          # lib.rs:1214
        if self.wlvl_hook is None:
            # the reference still runs the whole transform and returns an empty Vec (lib.rs:1796-1807)
            self._run_with_hook(input, seeds, None, False)
            return []
        return self._run_with_hook(input, seeds, self.wlvl_hook, False)[0]

    def transform_history(self, input, seeds):            # lib.rs:1233-1237, 1538-1549, 1824-1835
        return self._run_with_hook(input, seeds, lambda ctx: (ctx.water_level, ctx.colours.copy()), False)[0]

    def transform_history_levels(self, input, seeds, levels=None, out=None):
        """transform_history for the water levels in `levels` only -- any order, repeats allowed, at most 256; None: every level
        -- as ONE call of the library (ws_transform_history: no per-level hook, the planes rendered on the device in one pass).
        Returns [(level, u64 plane)] in the order of `levels`; with levels=None exactly what transform_history returns.  Not a
        method of the reference.  `out`: a reusable C-contiguous (K, H', W') uint64 array the planes are written into (the
        planes returned are views of it)."""
        lv = _history_levels(levels, self.max_water_level)
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        ph, pw = self._shape(a)
        if out is None:
            out = np.empty((lv.size, ph, pw), dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags.c_contiguous or out.shape != (lv.size, ph, pw):
            raise ValueError(f"out must be a C-contiguous uint64 array of shape {(lv.size, ph, pw)}")
        if lv.size:
            ctx = self._ctx()
            rc = _ffi.lib().ws_transform_history(ctx.handle, int(self._merging), a.ctypes.data, h, w, stride, s.ctypes.data, ns,
                                                 ctypes.byref(self._opt), lv.ctypes.data, lv.size, out.ctypes.data)
            ctx.check(rc)
        return [(int(lvl), out[k]) for k, lvl in enumerate(lv)]

    def transform_to_list(self, input, seeds):            # lib.rs:1220-1224, 1551-1561, 1837-1847
        """[(level, lake_sizes)] with lake_sizes a uint64 vector of length pixels+1 (lib.rs:630)."""
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        ph, pw = self._shape(a)
        ctx = self._ctx()
        levels = self.max_water_level + 1
        offsets = np.zeros(levels + 1, dtype=np.uint64)
        unc = np.zeros(levels, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        # one record per live lake and level, at most ns * levels; half of that covers a random field (83 per seed
        # at 1024^2).  A too small guess costs a second transform, not a wrong answer.
        cap = min(max(ns, 1) * (self.max_water_level + 1) // 2 + 1024, 1 << 26)
        while True:
            lakes = np.empty((cap, 2), dtype=np.uint64)
            rc = _ffi.lib().ws_transform_to_list(ctx.handle, int(self._merging), a.ctypes.data, h, w, stride,
                                                 s.ctypes.data, ns, ctypes.byref(self._opt), lakes.ctypes.data, cap,
                                                 ctypes.byref(n), offsets.ctypes.data, unc.ctypes.data)
            if rc == _ffi.WS_ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            ctx.check(rc)
            break
        out = []
        for lvl in range(levels):
            hist = np.zeros(ph * pw + 1, dtype=np.uint64)
            lo, hi = int(offsets[lvl]), int(offsets[lvl + 1])
            hist[lakes[lo:hi, 0].astype(np.int64)] = lakes[lo:hi, 1]
            hist[0] = unc[lvl]
            out.append((lvl, hist))
        return out

    def transform_to_list_sparse(self, input, seeds):
        """Same content as transform_to_list without the dense h*w+1 vectors:
        [(level, uncoloured, colours[], areas[])]."""
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        ctx = self._ctx()
        levels = self.max_water_level + 1
        offsets = np.zeros(levels + 1, dtype=np.uint64)
        unc = np.zeros(levels, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        # one record per live lake and level, at most ns * levels; half of that covers a random field (83 per seed
        # at 1024^2).  A too small guess costs a second transform, not a wrong answer.
        cap = min(max(ns, 1) * (self.max_water_level + 1) // 2 + 1024, 1 << 26)
        while True:
            lakes = np.empty((cap, 2), dtype=np.uint64)
            rc = _ffi.lib().ws_transform_to_list(ctx.handle, int(self._merging), a.ctypes.data, h, w, stride,
                                                 s.ctypes.data, ns, ctypes.byref(self._opt), lakes.ctypes.data, cap,
                                                 ctypes.byref(n), offsets.ctypes.data, unc.ctypes.data)
            if rc == _ffi.WS_ERR_CAPACITY and n.value > cap:
                cap = n.value
                continue
            ctx.check(rc)
            break
        # views into one record array (no per-level copies: 155 MB of them at 1024^2)
        off = offsets.astype(np.int64)
        return [(lvl, int(unc[lvl]), lakes[off[lvl]:off[lvl + 1], 0], lakes[off[lvl]:off[lvl + 1], 1]) for lvl in range(levels)]


    def transform_to_list_cube(self, cube, seeds=None):
        """transform_to_list_sparse of every slice cube[k] of a 3-D u8 array with seeds[k] -- or, with seeds None, the slice's own
        find_local_minima -- in ONE call of the library (ws_transform_to_list_batch: slices that stack run one set of per-level
        launches for the whole cube).  Returns, per slice, [(level, uncoloured, colours[], areas[])] in the slice's own colours
        (and, with seeds None, the number of minima of every slice).  Not a method of the reference."""
        c = np.asarray(cube)
        if c.ndim != 3:
            raise ValueError("cube must be 3-D: (slices, rows, columns)")
        c = np.ascontiguousarray(c, dtype=np.uint8)
        n, h, w = c.shape
        if seeds is None:
            flat, offs = None, None
        else:
            if len(seeds) != n:
                raise ValueError("one seed list per slice")
            lists = [np.asarray(s, dtype=np.uint64).reshape(-1, 2) for s in seeds]
            offs = np.zeros(n + 1, dtype=np.uintp)
            offs[1:] = np.cumsum([len(l) for l in lists])
            flat = np.ascontiguousarray(np.concatenate(lists, axis=0) if lists else np.zeros((0, 2), dtype=np.uint64))
            if flat.shape[0] == 0:
                flat = np.zeros((1, 2), dtype=np.uint64)
        ctx = self._ctx()
        levels = self.max_water_level + 1
        offsets = np.zeros(n * levels + 1, dtype=np.uint64)
        unc = np.zeros(max(n * levels, 1), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uintp)
        total = ctypes.c_size_t(0)
        failed = ctypes.c_size_t(0)
        # one record per pixel of the cube (a random field needs ~10, a smooth map far fewer); a too small guess costs a second
        # transform, not a wrong answer
        cap = min(n * h * w + 1024, 1 << 28)
        while True:
            lakes = np.empty((cap, 2), dtype=np.uint64)
            rc = _ffi.lib().ws_transform_to_list_batch(ctx.handle, int(self._merging), c.ctypes.data, n, h, w, w, h * w,
                                                       flat.ctypes.data if flat is not None else None,
                                                       offs.ctypes.data_as(_ffi.szp) if offs is not None else None,
                                                       ctypes.byref(self._opt), lakes.ctypes.data, cap, ctypes.byref(total),
                                                       offsets.ctypes.data, unc.ctypes.data, counts.ctypes.data_as(_ffi.szp),
                                                       ctypes.byref(failed))
            if rc == _ffi.WS_ERR_CAPACITY and total.value > cap:
                cap = total.value
                continue
            ctx.check(rc)
            break
        off = offsets.astype(np.int64)
        out = []
        for k in range(n):      # views into one record array
            b = k * levels
            out.append([(lvl, int(unc[b + lvl]), lakes[off[b + lvl]:off[b + lvl + 1], 0], lakes[off[b + lvl]:off[b + lvl + 1], 1])
                        for lvl in range(levels)])
        return out if seeds is not None else (out, counts[:n].astype(np.int64))

    def transform_history_cube(self, cube, seeds=None, levels=None, out=None):
        """transform_history_levels of every slice cube[k] of a 3-D u8 array with seeds[k] -- or, with seeds None, the slice's own
        find_local_minima -- for the water levels in `levels` (any order, repeats allowed, at most 256; None: every level), in ONE
        call of the library (ws_transform_history_batch: slices that stack run one flood and one set of per-level launches for
        the whole cube).  Returns, per slice, [(level, u64 plane)] in the order of `levels`, the planes views of one (S, K, H', W')
        array in the slice's own colours (and, with seeds None, the number of minima of every slice).  `out`: a reusable
        C-contiguous (S, K, H', W') uint64 array.  Not a method of the reference."""
        c = np.asarray(cube)
        if c.ndim != 3:
            raise ValueError("cube must be 3-D: (slices, rows, columns)")
        n = c.shape[0]
        if seeds is not None and len(seeds) != n:
            raise ValueError("one seed list per slice")
        lv = _history_levels(levels, self.max_water_level)
        c = np.ascontiguousarray(c, dtype=np.uint8)
        _, h, w = c.shape
        e = 2 if self.edge_correction else 0
        ph, pw = h + e, w + e
        shape = (n, lv.size, ph, pw)
        if out is None:
            out = np.empty(shape, dtype=np.uint64)
        elif out.dtype != np.uint64 or not out.flags.c_contiguous or out.shape != shape:
            raise ValueError(f"out must be a C-contiguous uint64 array of shape {shape}")
        if seeds is None:
            flat, offs = None, None
        else:
            lists = [np.asarray(s, dtype=np.uint64).reshape(-1, 2) for s in seeds]
            offs = np.zeros(n + 1, dtype=np.uintp)
            offs[1:] = np.cumsum([len(l) for l in lists])
            flat = np.ascontiguousarray(np.concatenate(lists, axis=0) if lists else np.zeros((0, 2), dtype=np.uint64))
            if flat.shape[0] == 0:
                flat = np.zeros((1, 2), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uintp)
        if lv.size and n:
            ctx = self._ctx()
            failed = ctypes.c_size_t(0)
            rc = _ffi.lib().ws_transform_history_batch(ctx.handle, int(self._merging), c.ctypes.data, n, h, w, w, h * w,
                                                       flat.ctypes.data if flat is not None else None,
                                                       offs.ctypes.data_as(_ffi.szp) if offs is not None else None,
                                                       ctypes.byref(self._opt), lv.ctypes.data, lv.size, out.ctypes.data,
                                                       counts.ctypes.data_as(_ffi.szp), ctypes.byref(failed))
            ctx.check(rc)
        res = [[(int(lvl), out[k, j]) for j, lvl in enumerate(lv)] for k in range(n)]
        return res if seeds is not None else (res, counts[:n].astype(np.int64))


class SegmentingWatershed(_Transform):
    """lib.rs:1609-1849"""
    _merging = False

    def transform(self, input, seeds):                    # lib.rs:1810-1822 (intended semantics)
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        ctx = self._ctx()
        out = np.empty(self._shape(a), dtype=np.uint64)
        rc = _ffi.lib().ws_segment(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                                   out.ctypes.data)
        ctx.check(rc)
        return out

    def transform_from_minima(self, input, want_seeds=False, labels_u32=False):
        """`self.transform(input, &self.find_local_minima(input))` -- the README's call pair, lib.rs:73-86 -- as ONE call of the
        library (ws_segment_minima): the seed list never crosses PCIe unless want_seeds.  Not a method of the reference."""
        a, stride = _as_image(input)
        h, w = a.shape
        ctx = self._ctx()
        out = np.empty(self._shape(a), dtype=np.uint32 if labels_u32 else np.uint64)
        cap = ((max(h, 1) - 1) // 2 + 1) * ((max(w, 1) - 1) // 2 + 1) if want_seeds else 0
        seeds = np.empty((max(cap, 1), 2), dtype=np.uint64) if want_seeds else None
        n = ctypes.c_size_t(0)
        fn = _ffi.lib().ws_segment_minima_u32 if labels_u32 else _ffi.lib().ws_segment_minima
        ctx.check(fn(ctx.handle, a.ctypes.data, h, w, stride, ctypes.byref(self._opt), out.ctypes.data,
                     seeds.ctypes.data if want_seeds else None, cap, ctypes.byref(n)))
        return (out, seeds[: n.value].copy()) if want_seeds else out

    def transform_cube(self, cube, seeds=None):
        """The slices cube[k] of a 3-D u8 array, each as `transform(cube[k], seeds[k])` -- or, with seeds None, as the README's
        pair `transform(cube[k], &find_local_minima(cube[k]))` -- in ONE call of the library (ws_segment_batch: the slices'
        uploads, transforms and label copies overlap).  What tests/integration.rs:267,356 loops over.  Returns the label cube
        (and, with seeds None, the number of minima of every slice).  Not a method of the reference."""
        c = np.ascontiguousarray(cube, dtype=np.uint8)
        if c.ndim != 3:
            raise ValueError("cube must be 3-D: (slices, rows, columns)")
        n, h, w = c.shape
        ctx = self._ctx()
        ph, pw = self._shape(c[0]) if n else (h, w)
        out = np.empty((n, ph, pw), dtype=np.uint64)
        counts = np.zeros(max(n, 1), dtype=np.uintp)
        failed = ctypes.c_size_t(0)
        if seeds is None:
            flat, offs = None, None
        else:
            if len(seeds) != n:
                raise ValueError("one seed list per slice")
            lists = [np.asarray(s, dtype=np.uint64).reshape(-1, 2) for s in seeds]
            offs = np.zeros(n + 1, dtype=np.uintp)
            offs[1:] = np.cumsum([len(l) for l in lists])
            flat = np.ascontiguousarray(np.concatenate(lists, axis=0) if lists else np.zeros((0, 2), dtype=np.uint64))
            if flat.shape[0] == 0:
                flat = np.zeros((1, 2), dtype=np.uint64)
        ctx.check(_ffi.lib().ws_segment_batch(ctx.handle, c.ctypes.data, n, h, w, w, h * w, flat.ctypes.data if flat is not None else None,
                                              offs.ctypes.data_as(_ffi.szp) if offs is not None else None, ctypes.byref(self._opt),
                                              out.ctypes.data, counts.ctypes.data_as(_ffi.szp), ctypes.byref(failed)))
        return out if seeds is not None else (out, counts[:n].astype(np.int64))


class MergingWatershed(_Transform):
    """lib.rs:1297-1562"""
    _merging = True

    def transform(self, input, _seeds=None):              # lib.rs:1524-1536: a stub in the reference
        a, _ = _as_image(input)
        out = np.empty(a.shape, dtype=np.uint64)
        rc = _ffi.lib().ws_merge_transform_stub(a.shape[0], a.shape[1], out.ctypes.data)
        if rc != _ffi.WS_OK:
            raise WatershedError(rc)
        return out

    def transform_final(self, input, seeds):
        """Not in the reference: the merged label plane after the last level."""
        return self._run_with_hook(input, seeds, None, True)[1]

    def merge_tree(self, input, seeds, want_labels=False):
        """Not in the reference: the lake hierarchy of the merging transform as a MergeTree -- one record per seed colour from one
        flood, no plane written (ws_merge_tree).  want_labels: also the segmenting label plane (u64) the colours refer to."""
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        tree = np.empty((ns + 1, 4), dtype=np.uint32)
        labels = np.empty(self._shape(a), dtype=np.uint64) if want_labels else None
        ctx = self._ctx()
        ctx.check(_ffi.lib().ws_merge_tree(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                                           tree.ctypes.data, labels.ctypes.data if want_labels else None))
        return MergeTree(tree[:, 0].copy(), tree[:, 1].copy(), tree[:, 2].copy(), tree[:, 3].copy(), labels)

    def merge_tree_cut(self, input, seeds, cuts, want_tree=False, want_lakes=False, weights=None, want_stats=False):
        """Not in the reference: the label planes of the merge tree pruned by `cuts` (a Cut or up to 32 of them), the whole route
        in one call (ws_merge_tree_cut): a (K, H', W') u64 array whose plane k shows every pixel the lake cuts[k] leaves it in,
        0 where it is hidden.  want_tree: also the MergeTree.  want_lakes: also (lakes, offsets, hidden) -- lakes[offsets[k] :
        offsets[k + 1]] are cut k's (colour, pixels) records in increasing colour, hidden[k] its pixels that show 0.
        A cut with a catalogue threshold (min_sum_w, min_w_max, min_depth), `weights` (a u8 or u16 plane of the image's shape;
        None: the image itself) or want_stats (also the catalogue, as merge_tree_stats returns it) take the route with the lake
        statistics (ws_merge_tree_stats_cut).  Returns planes, or (planes[, tree][, stats][, (lakes, offsets, hidden)])."""
        lst = _cut_list(cuts)
        k = len(lst)
        if k == 0:
            raise ValueError("merge_tree_cut needs at least one cut")
        with_stats = want_stats or weights is not None or any(c.catalogue for c in lst)
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        ph, pw = self._shape(a)
        planes = np.empty((k, ph, pw), dtype=np.uint64)
        tree = np.empty((ns + 1, 4), dtype=np.uint32) if want_tree else None
        offsets = np.zeros(k + 1, dtype=np.uint64)
        hidden = np.zeros(k, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        cap = max(min(ns, ph * pw), 1) * k if want_lakes else 0      # a cut shows no more colours than there are, or pixels
        lakes = np.empty((max(cap, 1), 2), dtype=np.uint64)
        ctx = self._ctx()
        stats = None
        if with_stats:
            arr, _ = _as_lake_cuts(lst)
            wt, dtype, wstride = _as_weights(weights, a.shape)
            stats = np.empty(ns + 1, dtype=LAKE_STATS_DTYPE) if want_stats else None
            ctx.check(_ffi.lib().ws_merge_tree_stats_cut(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                                                         wt.ctypes.data if wt is not None else None, dtype, wstride, arr, k,
                                                         tree.ctypes.data if want_tree else None, stats.ctypes.data if want_stats else None,
                                                         planes.ctypes.data, lakes.ctypes.data if want_lakes else None, cap, ctypes.byref(n),
                                                         offsets.ctypes.data, hidden.ctypes.data))
        else:
            arr, _ = _as_cuts(lst)
            ctx.check(_ffi.lib().ws_merge_tree_cut(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                                                   arr, k, tree.ctypes.data if want_tree else None, planes.ctypes.data,
                                                   lakes.ctypes.data if want_lakes else None, cap, ctypes.byref(n),
                                                   offsets.ctypes.data, hidden.ctypes.data))
        out = [planes]
        if want_tree:
            out.append(MergeTree(tree[:, 0].copy(), tree[:, 1].copy(), tree[:, 2].copy(), tree[:, 3].copy()))
        if want_stats:
            out.append(stats)
        if want_lakes:
            out.append((lakes[: n.value].copy(), offsets, hidden))
        return out[0] if len(out) == 1 else tuple(out)

    def merge_tree_cut_catalogue(self, input, seeds, cuts, weights=None, want_tree=False, want_stats=False, want_planes=True):
        """Not in the reference: merge_tree_cut with the regions its cuts show MEASURED -- the source list of every cut from one
        call (ws_merge_tree_cut_catalogue).  Returns (planes | None, lakes, region_stats, offsets, hidden, hidden_stats[, tree]
        [, stats]): planes, lakes, offsets and hidden as merge_tree_cut(want_lakes=True); region_stats a structured array
        (LAKE_STATS_DTYPE) next to lakes, record i the weighted and plain first moments, the box, the extrema and the first peak
        pixel of the pixels lakes[i] counts -- the region of colour lakes[i, 0] in its cut, which is NOT the catalogue's record of
        that colour; hidden_stats[k] the same over the pixels cut k shows as 0.  weights as merge_tree_stats (None: the image
        itself); rows and columns are those of the padded plane.  centroids(region_stats) gives the weighted centroids.
        want_planes=False: no plane is rendered or downloaded.  want_tree / want_stats: also the MergeTree / the catalogue."""
        lst = _cut_list(cuts)
        k = len(lst)
        if k == 0:
            raise ValueError("merge_tree_cut_catalogue needs at least one cut")
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        ph, pw = self._shape(a)
        arr, _ = _as_lake_cuts(lst)
        wt, dtype, wstride = _as_weights(weights, a.shape)
        planes = np.empty((k, ph, pw), dtype=np.uint64) if want_planes else None
        tree = np.empty((ns + 1, 4), dtype=np.uint32) if want_tree else None
        stats = np.empty(ns + 1, dtype=LAKE_STATS_DTYPE) if want_stats else None
        offsets = np.zeros(k + 1, dtype=np.uint64)
        hidden = np.zeros(k, dtype=np.uint64)
        n = ctypes.c_size_t(0)
        cap = max(min(ns, ph * pw), 1) * k      # a cut shows no more colours than there are, or pixels
        lakes = np.empty((cap, 2), dtype=np.uint64)
        region = np.empty(cap, dtype=LAKE_STATS_DTYPE)
        hidden_stats = np.empty(k, dtype=LAKE_STATS_DTYPE)
        ctx = self._ctx()
        ctx.check(_ffi.lib().ws_merge_tree_cut_catalogue(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                                                         wt.ctypes.data if wt is not None else None, dtype, wstride, arr, k,
                                                         tree.ctypes.data if want_tree else None, stats.ctypes.data if want_stats else None,
                                                         planes.ctypes.data if want_planes else None, lakes.ctypes.data, region.ctypes.data, cap,
                                                         ctypes.byref(n), offsets.ctypes.data, hidden.ctypes.data, hidden_stats.ctypes.data))
        out = [planes, lakes[: n.value].copy(), region[: n.value].copy(), offsets, hidden, hidden_stats]
        if want_tree:
            out.append(MergeTree(tree[:, 0].copy(), tree[:, 1].copy(), tree[:, 2].copy(), tree[:, 3].copy()))
        if want_stats:
            out.append(stats)
        return tuple(out)

    def merge_tree_cut_catalogue_cube(self, cube, seeds=None, cuts=(), weights=None, want_tree=False, want_stats=False, want_planes=True):
        """merge_tree_cut_catalogue of every slice cube[k] of a 3-D u8 array with seeds[k] -- or, with seeds None, the slice's own
        find_local_minima -- and the weight plane weights[k] (a u8 or u16 cube of the cube's shape; None: the cube itself) in ONE
        call of the library (ws_merge_tree_cut_catalogue_batch: slices that stack share one flood, and every stacked group is cut
        once, while its stamps are on the device).  Returns one tuple per slice, as merge_tree_cut_catalogue returns it for the
        slice alone: (planes | None, lakes, region_stats, offsets, hidden, hidden_stats[, tree][, stats]) in the slice's own colours,
        rows, columns and peak pixels, offsets from 0; the arrays are views of one array per output.  Not a method of the
        reference."""
        lst = _cut_list(cuts)
        k = len(lst)
        if k == 0:
            raise ValueError("merge_tree_cut_catalogue_cube needs at least one cut")
        c = np.asarray(cube)
        if c.ndim != 3:
            raise ValueError("cube must be 3-D: (slices, rows, columns)")
        if c.dtype != np.uint8:
            raise ValueError("cube must be uint8")
        n = c.shape[0]
        if seeds is not None and len(seeds) != n:
            raise ValueError("one seed list per slice")
        wt, dtype = None, 0
        if weights is not None:
            wt = np.asarray(weights)
            if wt.dtype not in (np.uint8, np.uint16) or wt.ndim != 3:
                raise TypeError("weights must be a 3-D uint8 or uint16 array (quantise float data first: pre_processor_with_max)")
            if wt.shape != c.shape:
                raise ValueError(f"weights must have the cube's shape {c.shape}, not {wt.shape}")
            wt = np.ascontiguousarray(wt)
            dtype = _ffi.WS_DTYPES[wt.dtype.name]
        c = np.ascontiguousarray(c)
        _, h, w = c.shape
        e = 2 if self.edge_correction else 0
        ph, pw = h + e, w + e
        arr, _ = _as_lake_cuts(lst)
        if seeds is None:
            flat, offs = None, None
            rec_cap = n * (h * w // 8 + 1)      # (as merge_tree_cube: a too small guess costs a second call, before any flood)
        else:
            lists = [np.asarray(s, dtype=np.uint64).reshape(-1, 2) for s in seeds]
            offs = np.zeros(n + 1, dtype=np.uintp)
            offs[1:] = np.cumsum([len(l) for l in lists])
            flat = np.ascontiguousarray(np.concatenate(lists, axis=0) if lists else np.zeros((0, 2), dtype=np.uint64))
            if flat.shape[0] == 0:
                flat = np.zeros((1, 2), dtype=np.uint64)
            rec_cap = int(offs[n]) + n
        counts = np.zeros(max(n, 1), dtype=np.uintp)
        planes = np.empty((n, k, ph, pw), dtype=np.uint64) if want_planes else None
        offsets = np.zeros(n * k + 1, dtype=np.uint64)
        hidden = np.zeros(max(n * k, 1), dtype=np.uint64)
        hidden_stats = np.empty(max(n * k, 1), dtype=LAKE_STATS_DTYPE)
        tree = np.empty((max(rec_cap, 1), 4), dtype=np.uint32)
        stats = np.empty(max(rec_cap, 1), dtype=LAKE_STATS_DTYPE) if want_stats else None
        cap = max(min(rec_cap, n * ph * pw), 1) * k      # a cut shows no more colours than there are, or pixels
        lakes = np.empty((cap, 2), dtype=np.uint64)
        region = np.empty(cap, dtype=LAKE_STATS_DTYPE)
        got = ctypes.c_size_t(0)
        if n:
            ctx = self._ctx()
            total = ctypes.c_size_t(0)
            failed = ctypes.c_size_t(0)
            for attempt in range(3):
                rc = _ffi.lib().ws_merge_tree_cut_catalogue_batch(
                    ctx.handle, c.ctypes.data, n, h, w, w, h * w, flat.ctypes.data if flat is not None else None,
                    offs.ctypes.data_as(_ffi.szp) if offs is not None else None, ctypes.byref(self._opt), wt.ctypes.data if wt is not None else None,
                    dtype, w, h * w, arr, k, tree.ctypes.data, stats.ctypes.data if want_stats else None, rec_cap, ctypes.byref(total),
                    planes.ctypes.data if want_planes else None, lakes.ctypes.data, region.ctypes.data, cap, ctypes.byref(got), offsets.ctypes.data,
                    hidden.ctypes.data, hidden_stats.ctypes.data, counts.ctypes.data_as(_ffi.szp), ctypes.byref(failed))
                if rc == _ffi.WS_ERR_CAPACITY and total.value > rec_cap and attempt < 2:      # more minima than guessed: before any flood
                    rec_cap = total.value
                    tree = np.empty((rec_cap, 4), dtype=np.uint32)
                    stats = np.empty(rec_cap, dtype=LAKE_STATS_DTYPE) if want_stats else None
                    continue
                if rc == _ffi.WS_ERR_CAPACITY and got.value > cap and attempt < 2:
                    cap = got.value
                    lakes = np.empty((cap, 2), dtype=np.uint64)
                    region = np.empty(cap, dtype=LAKE_STATS_DTYPE)
                    continue
                ctx.check(rc)
                break
        first = np.zeros(n + 1, dtype=np.int64)
        first[1:] = np.cumsum((counts[:n] if seeds is None else np.diff(offs)).astype(np.int64) + 1)
        out = []
        for i in range(n):
            lo, hi = int(offsets[i * k]), int(offsets[(i + 1) * k])
            one = [planes[i] if want_planes else None, lakes[lo:hi], region[lo:hi], offsets[i * k:(i + 1) * k + 1] - offsets[i * k],
                   hidden[i * k:(i + 1) * k], hidden_stats[i * k:(i + 1) * k]]
            t = tree[first[i]:first[i + 1]]
            if want_tree:
                one.append(MergeTree(t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), t[:, 3].copy()))
            if want_stats:
                one.append(stats[first[i]:first[i + 1]])
            out.append(tuple(one))
        return out

    def merge_tree_stats(self, input, seeds, weights=None, want_labels=False):
        """Not in the reference: merge_tree and a catalogue of its lakes from the same flood (ws_merge_tree_stats).  Returns
        (MergeTree, stats): stats is a numpy structured array (LAKE_STATS_DTYPE) of n_seeds + 1 records, record c the weighted
        and plain first moments, the box, the extrema and the first peak pixel of the pixels `area[c]` counts, record 0 those of
        the pixels never coloured; rows and columns are those of the padded plane.  weights: a u8 or u16 plane of the image's
        shape (None: the image itself).  centroids(stats) gives the weighted centroids."""
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        wt, dtype, wstride = _as_weights(weights, a.shape)
        tree = np.empty((ns + 1, 4), dtype=np.uint32)
        stats = np.empty(ns + 1, dtype=LAKE_STATS_DTYPE)
        labels = np.empty(self._shape(a), dtype=np.uint64) if want_labels else None
        ctx = self._ctx()
        ctx.check(_ffi.lib().ws_merge_tree_stats(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                                                 wt.ctypes.data if wt is not None else None, dtype, wstride, tree.ctypes.data,
                                                 stats.ctypes.data, labels.ctypes.data if want_labels else None))
        return MergeTree(tree[:, 0].copy(), tree[:, 1].copy(), tree[:, 2].copy(), tree[:, 3].copy(), labels), stats

    def merge_tree_shapes(self, input, seeds, weights=None, want_labels=False):
        """Not in the reference: merge_tree_stats and the second moments of every lake from the same flood (ws_merge_tree_shapes).
        Returns (MergeTree, stats, shapes[, labels]): shapes is a numpy structured array (LAKE_SHAPE_DTYPE) of n_seeds + 1 records,
        record c the exact 128-bit sums of v row^2, v col^2, v row col, row^2, col^2 and row col over the pixels `area[c]`
        counts, each as (low, high) u64, record 0 those of the pixels never coloured; rows and columns are those of the padded
        plane.  weights as merge_tree_stats.  ellipses(stats, shapes) gives sizes, elongations and position angles."""
        a, stride = _as_image(input)
        s, ns = _as_seeds(seeds)
        h, w = a.shape
        wt, dtype, wstride = _as_weights(weights, a.shape)
        tree = np.empty((ns + 1, 4), dtype=np.uint32)
        stats = np.empty(ns + 1, dtype=LAKE_STATS_DTYPE)
        shapes = np.empty(ns + 1, dtype=LAKE_SHAPE_DTYPE)
        labels = np.empty(self._shape(a), dtype=np.uint64) if want_labels else None
        ctx = self._ctx()
        ctx.check(_ffi.lib().ws_merge_tree_shapes(ctx.handle, a.ctypes.data, h, w, stride, s.ctypes.data, ns, ctypes.byref(self._opt),
                                                  wt.ctypes.data if wt is not None else None, dtype, wstride, tree.ctypes.data,
                                                  stats.ctypes.data, shapes.ctypes.data, labels.ctypes.data if want_labels else None))
        mt = MergeTree(tree[:, 0].copy(), tree[:, 1].copy(), tree[:, 2].copy(), tree[:, 3].copy(), labels)
        return (mt, stats, shapes, labels) if want_labels else (mt, stats, shapes)

    def merge_tree_cube(self, cube, seeds=None, want_labels=False):
        """merge_tree of every slice cube[k] of a 3-D u8 array with seeds[k] -- or, with seeds None, the slice's own
        find_local_minima -- in ONE call of the library (ws_merge_tree_batch: slices that stack run one flood, one set of
        per-level unions and one fold launch per level for the whole cube).  Returns a list of MergeTree, one per slice, in the
        slice's own colours (and, with seeds None, the number of minima of every slice); want_labels: every tree carries its
        slice's segmenting label plane (u64), views of one (S, H', W') array.  Not a method of the reference."""
        c = np.asarray(cube)
        if c.ndim != 3:
            raise ValueError("cube must be 3-D: (slices, rows, columns)")
        if c.dtype != np.uint8:
            raise ValueError("cube must be uint8")
        n = c.shape[0]
        if seeds is not None and len(seeds) != n:
            raise ValueError("one seed list per slice")
        c = np.ascontiguousarray(c)
        _, h, w = c.shape
        e = 2 if self.edge_correction else 0
        if seeds is None:
            flat, offs = None, None
            cap = n * (h * w // 8 + 1)      # minima are rarely denser than one in eight pixels; a too small guess costs a second call, before any flood
        else:
            lists = [np.asarray(s, dtype=np.uint64).reshape(-1, 2) for s in seeds]
            offs = np.zeros(n + 1, dtype=np.uintp)
            offs[1:] = np.cumsum([len(l) for l in lists])
            flat = np.ascontiguousarray(np.concatenate(lists, axis=0) if lists else np.zeros((0, 2), dtype=np.uint64))
            if flat.shape[0] == 0:
                flat = np.zeros((1, 2), dtype=np.uint64)
            cap = int(offs[n]) + n
        labels = np.empty((n, h + e, w + e), dtype=np.uint64) if want_labels else None
        counts = np.zeros(max(n, 1), dtype=np.uintp)
        tree = np.empty((max(cap, 1), 4), dtype=np.uint32)
        if n:
            ctx = self._ctx()
            total = ctypes.c_size_t(0)
            failed = ctypes.c_size_t(0)
            for attempt in range(2):
                rc = _ffi.lib().ws_merge_tree_batch(ctx.handle, c.ctypes.data, n, h, w, w, h * w,
                                                    flat.ctypes.data if flat is not None else None,
                                                    offs.ctypes.data_as(_ffi.szp) if offs is not None else None,
                                                    ctypes.byref(self._opt), tree.ctypes.data, cap, ctypes.byref(total),
                                                    labels.ctypes.data if want_labels else None, counts.ctypes.data_as(_ffi.szp),
                                                    ctypes.byref(failed))
                if rc == _ffi.WS_ERR_CAPACITY and total.value > cap and attempt == 0:
                    cap = total.value
                    tree = np.empty((cap, 4), dtype=np.uint32)
                    continue
                ctx.check(rc)
                break
        first = np.zeros(n + 1, dtype=np.int64)
        first[1:] = np.cumsum((counts[:n] if seeds is None else np.diff(offs)).astype(np.int64) + 1)
        out = []
        for k in range(n):
            t = tree[first[k]:first[k + 1]]
            out.append(MergeTree(t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), t[:, 3].copy(), labels[k] if want_labels else None))
        return out if seeds is not None else (out, counts[:n].astype(np.int64))

    def merge_tree_stats_cube(self, cube, seeds=None, weights=None, want_labels=False):
        """merge_tree_stats of every slice cube[k] of a 3-D u8 array with seeds[k] -- or, with seeds None, the slice's own
        find_local_minima -- and the weight plane weights[k] (a u8 or u16 cube of the cube's shape; None: the cube itself) in ONE
        call of the library (ws_merge_tree_stats_batch: slices that stack run one flood, one set of per-level unions and one
        fold launch per level, of the tree and of the statistics, for the whole cube).  Returns a list of (MergeTree, stats), one
        per slice, as merge_tree_stats returns them for the slice alone: the slice's own colours, rows, columns and peak pixels
        (and, with seeds None, the number of minima of every slice); want_labels as merge_tree_cube.  Not a method of the
        reference."""
        return self._tree_stats_cube(cube, seeds, weights, want_labels, False)

    def merge_tree_shapes_cube(self, cube, seeds=None, weights=None, want_labels=False):
        """merge_tree_shapes of every slice of a cube in ONE call of the library (ws_merge_tree_shapes_batch: slices that stack
        run the shape kernels once over the stack, after the tree's and the statistics').  cube, seeds, weights and want_labels
        as merge_tree_stats_cube.  Returns a list of (MergeTree, stats, shapes), one per slice, as merge_tree_shapes returns them
        for the slice alone -- rows and columns are the slice's own, so ellipses(stats, shapes) works on a slice's pair unchanged
        (and, with seeds None, the number of minima of every slice).  Not a method of the reference."""
        return self._tree_stats_cube(cube, seeds, weights, want_labels, True)

    def _tree_stats_cube(self, cube, seeds, weights, want_labels, with_shapes):
        """merge_tree_stats_cube and, with_shapes, merge_tree_shapes_cube: the two calls differ in one record array."""
        c = np.asarray(cube)
        if c.ndim != 3:
            raise ValueError("cube must be 3-D: (slices, rows, columns)")
        if c.dtype != np.uint8:
            raise ValueError("cube must be uint8")
        n = c.shape[0]
        if seeds is not None and len(seeds) != n:
            raise ValueError("one seed list per slice")
        wt, dtype = None, 0
        if weights is not None:
            wt = np.asarray(weights)
            if wt.dtype not in (np.uint8, np.uint16) or wt.ndim != 3:
                raise TypeError("weights must be a 3-D uint8 or uint16 array (quantise float data first: pre_processor_with_max)")
            if wt.shape != c.shape:
                raise ValueError(f"weights must have the cube's shape {c.shape}, not {wt.shape}")
            wt = np.ascontiguousarray(wt)
            dtype = _ffi.WS_DTYPES[wt.dtype.name]
        c = np.ascontiguousarray(c)
        _, h, w = c.shape
        e = 2 if self.edge_correction else 0
        if seeds is None:
            flat, offs = None, None
            cap = n * (h * w // 8 + 1)      # (as merge_tree_cube: a too small guess costs a second call, before any flood)
        else:
            lists = [np.asarray(s, dtype=np.uint64).reshape(-1, 2) for s in seeds]
            offs = np.zeros(n + 1, dtype=np.uintp)
            offs[1:] = np.cumsum([len(l) for l in lists])
            flat = np.ascontiguousarray(np.concatenate(lists, axis=0) if lists else np.zeros((0, 2), dtype=np.uint64))
            if flat.shape[0] == 0:
                flat = np.zeros((1, 2), dtype=np.uint64)
            cap = int(offs[n]) + n
        labels = np.empty((n, h + e, w + e), dtype=np.uint64) if want_labels else None
        counts = np.zeros(max(n, 1), dtype=np.uintp)
        tree = np.empty((max(cap, 1), 4), dtype=np.uint32)
        stats = np.empty(max(cap, 1), dtype=LAKE_STATS_DTYPE)
        shapes = np.empty(max(cap, 1), dtype=LAKE_SHAPE_DTYPE) if with_shapes else None
        if n:
            ctx = self._ctx()
            total = ctypes.c_size_t(0)
            failed = ctypes.c_size_t(0)
            for attempt in range(2):
                inputs = (ctx.handle, c.ctypes.data, n, h, w, w, h * w, flat.ctypes.data if flat is not None else None,
                          offs.ctypes.data_as(_ffi.szp) if offs is not None else None, ctypes.byref(self._opt),
                          wt.ctypes.data if wt is not None else None, dtype, w, h * w, tree.ctypes.data, stats.ctypes.data)
                rest = (cap, ctypes.byref(total), labels.ctypes.data if want_labels else None, counts.ctypes.data_as(_ffi.szp), ctypes.byref(failed))
                if with_shapes:
                    rc = _ffi.lib().ws_merge_tree_shapes_batch(*inputs, shapes.ctypes.data, *rest)
                else:
                    rc = _ffi.lib().ws_merge_tree_stats_batch(*inputs, *rest)
                if rc == _ffi.WS_ERR_CAPACITY and total.value > cap and attempt == 0:
                    cap = total.value
                    tree = np.empty((cap, 4), dtype=np.uint32)
                    stats = np.empty(cap, dtype=LAKE_STATS_DTYPE)
                    shapes = np.empty(cap, dtype=LAKE_SHAPE_DTYPE) if with_shapes else None
                    continue
                ctx.check(rc)
                break
        first = np.zeros(n + 1, dtype=np.int64)
        first[1:] = np.cumsum((counts[:n] if seeds is None else np.diff(offs)).astype(np.int64) + 1)
        out = []
        for k in range(n):
            t = tree[first[k]:first[k + 1]]
            mt = MergeTree(t[:, 0].copy(), t[:, 1].copy(), t[:, 2].copy(), t[:, 3].copy(), labels[k] if want_labels else None)
            rec = (mt, stats[first[k]:first[k + 1]])      # (views of one array, as the labels: 72 B a record add up)
            out.append(rec + (shapes[first[k]:first[k + 1]],) if with_shapes else rec)
        return out if seeds is not None else (out, counts[:n].astype(np.int64))
