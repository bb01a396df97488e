"""The cut catalogue (ws_tree_cut_catalogue_device, ws_merge_tree_cut_catalogue) derived with numpy from the CPU oracle: the planes
of tests/tree_cut_stats_ref.py's `cut_by_walk`, folded by label with tests/lake_stats_ref.py's `records_by_label` -- record a of
that fold is the region {p : out_k(p) == a} measured, record 0 the hidden pixels.  What the engine returns is that fold restricted
to the colours with pixels, in increasing colour.  The cases the CPU and GPU tests share are built here once per process and never
changed afterwards."""
import numpy as np

import lake_stats_ref as ls
import seed_cases as sc
import tree_cut_ref as tc
import tree_cut_stats_ref as ts

Cut = ts.Cut
RUN = 1024      # pixels of one step of a workgroup: the run its table serves


def _all_seeds():
    """48 x 52 noise in which EVERY pixel is a seed: 2496 colours.  Seeds that touch merge at level 0, so nearly every colour dies
    there and the chains of level 0 are long; the regions are few (checker48x52 is the case with many)."""
    h, w = 48, 52
    return ts.Field("all_seeds48x52", tc.Field("all_seeds48x52", sc.image("noise", h, w, 77), sc.from_pixels(np.arange(h * w), w)))


def _checker():
    """48 x 52 noise with a seed on every other pixel, like a chessboard: no two seeds touch, so none dies at level 0 (as nearly all
    of all_seeds48x52's do) and a cut that merges nothing shows 1246 regions, more than 500 of them in a run of 1024 pixels."""
    h, w = 48, 52
    r, c = np.indices((h, w))
    return ts.Field("checker48x52", tc.Field("checker48x52", sc.image("noise", h, w, 77), sc.from_pixels(np.flatnonzero(((r + c) % 2 == 0).ravel()), w)))


def _constant_weights():
    """random48x52 under a constant weight plane: every peak is a tie, so peak_pixel is the region's first pixel."""
    f = tc.field("random48x52")
    return ts.Field("random48x52_const", f, np.full(f.img.shape, 7, dtype=np.uint8))


_EXTRA = {"all_seeds48x52": _all_seeds, "checker48x52": _checker, "random48x52_const": _constant_weights}
_FIELDS = {}

ALL_SEEDS_CUTS = [Cut(show_level=254, merge_level=0), Cut(min_area=3), Cut(show_level=120, merge_level=40), Cut(show_level=254, merge_level=0)]
# 32 cuts of random48x52 in one call: 24 different ones (many tables, both levels, every threshold) and 8 repeats of them
_THIRTY_TWO = [Cut(min_area=(k * 7) % 5, min_leaves=k % 2, show_level=254 - 9 * (k % 5), merge_level=(k * 37) % 255,
                   min_sum_w=(0, 335, 336, 893)[k % 4], min_w_max=(0, 0, 239, 250)[(k // 4) % 4], min_depth=(0, 30, 55, 0, 87)[k % 5]) for k in range(24)]
THIRTY_TWO = _THIRTY_TWO[:12] + [_THIRTY_TWO[k] for k in (3, 0, 11, 7)] + _THIRTY_TWO[12:] + [_THIRTY_TWO[k] for k in (23, 3, 16, 12)]
REPEATS_32 = [(12, 3), (13, 0), (14, 11), (15, 7), (28, 27), (29, 3), (30, 20), (31, 16)]      # (position, position of the cut it repeats)

ALL = ts.ALL + ["all_seeds48x52", "checker48x52", "random48x52_const"]


def field(name):
    if name in _EXTRA:
        if name not in _FIELDS:
            _FIELDS[name] = _EXTRA[name]()
        return _FIELDS[name]
    return ts.field(name)


def cuts_of(name):
    """(field, cuts) of a shared case: the cut lists of tree_cut_stats_ref, and those of the cases that are this module's."""
    if name in ("all_seeds48x52", "checker48x52"):
        return field(name), ALL_SEEDS_CUTS
    if name == "random48x52_const":
        return field(name), ts.CUTS["random48x52"][:6]
    return ts.cuts_of(name)


def weights_of(f):
    """v(p) over the plane as the device form takes it: the plane's shape, no offset (a ring of zeros under edge correction)."""
    return ls.plane_weights(f.img, f.weights, f.edge)


def plane_weights_array(f):
    """The same as the array a device call is given: u8, or u16 for a u16 weight plane."""
    v = weights_of(f)
    return np.ascontiguousarray(v.astype(np.uint16 if f.weights is not None and np.asarray(f.weights).dtype == np.uint16 else np.uint8))


_FOLDS = {}


def fold(f, cut):
    """The n_seeds + 1 records of the fold by label over the plane of `cut` (the identity where a colour shows no pixel)."""
    key = (f.name, cut.key())
    if key not in _FOLDS:
        rec = ls.records_by_label(f.cut(cut), weights_of(f), f.n_seeds + 1)
        rec.setflags(write=False)
        _FOLDS[key] = rec
    return _FOLDS[key]


def expected(f, cuts):
    """What a call returns for `cuts`: (lakes (n, 2) u64, region records (n), offsets (K + 1), hidden (K), hidden records (K))."""
    planes = [f.cut(c) for c in cuts]
    lakes, offsets, hidden = tc.expected_lists(planes, f.n_seeds)
    region = ls.empty_records(len(lakes))
    hid = ls.empty_records(len(cuts))
    for k, c in enumerate(cuts):
        rec = fold(f, c)
        lo, hi = int(offsets[k]), int(offsets[k + 1])
        region[lo:hi] = rec[lakes[lo:hi, 0].astype(np.int64)]
        hid[k] = rec[0]
    return lakes, region, offsets, hidden, hid


def whole_plane(f):
    """The record of every pixel of the plane: what the regions of a cut and its hidden pixels join to."""
    return ls.records_by_label(np.zeros(f.shape, dtype=np.uint32), weights_of(f), 1)[0]


def regions_per_run(plane):
    """The number of distinct labels in every run of RUN consecutive pixels of the plane."""
    flat = np.asarray(plane).ravel()
    return [np.unique(flat[i: i + RUN]).size for i in range(0, flat.size, RUN)]
