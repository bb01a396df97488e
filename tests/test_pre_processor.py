"""pre_processor / pre_processor_with_max (lib.rs:1081-1173): the first "next" row of SURVEY 8f.
The reference has no test for it; the restatement is pinned by its own code reading (quirks listed in
include/ws_hip.h) with two independent implementations (C oracle, numpy) and the GPU against both."""
import numpy as np
import pytest

import __graft_entry__ as ge
import oracle_lib as ol


def _cases():
    rng = np.random.default_rng(3)
    out = []
    a = rng.random((40, 50))                                     # README-style Uniform(0,1) f64 field
    out.append(("uniform01_f64", a))
    b = rng.poisson(0.85, (30, 70)).astype(np.float64)           # tests/integration.rs:189 Poisson(0.85): many exact zeros
    out.append(("poisson_f64", b))
    c = rng.normal(0, 5, (33, 17)).astype(np.float32)
    c[3, 4] = np.nan; c[5, 6] = np.inf; c[7, 8] = -np.inf; c[9, 9] = 0.0; c[1, 1] = -0.0; c[2, 2] = 1e-42   # f32 subnormal
    out.append(("specials_f32", c))
    d = rng.normal(100, 30, (20, 20))
    d[0, 0] = 5e-324; d[1, 1] = np.nan; d[2, 2] = np.inf
    out.append(("all_positive_f64", d))                          # min fold stays at its seed 0
    out.append(("all_negative_f64", -np.abs(rng.normal(3, 1, (9, 11)))))   # max fold stays at 0
    out.append(("int32", rng.integers(-1000, 1000, (25, 25), dtype=np.int32)))
    out.append(("uint16", rng.integers(0, 65535, (16, 64), dtype=np.uint16)))
    out.append(("int16", rng.integers(-32768, 32767, (8, 8), dtype=np.int16)))
    out.append(("uint8", rng.integers(0, 255, (31, 3), dtype=np.uint8)))
    out.append(("cube_f32", rng.random((4, 10, 12)).astype(np.float32)))   # any dimension (lib.rs:1081: ArrayView<T, D>)
    out.append(("all_nan", np.full((5, 5), np.nan)))
    out.append(("all_zero", np.zeros((4, 4))))
    out.append(("empty", np.zeros((0, 7), dtype=np.float32)))
    return out


@pytest.mark.parametrize("name,arr", _cases(), ids=[c[0] for c in _cases()])
def test_oracle_pre_processor_two_restatements_agree(name, arr):
    for mx in (254, 127, 1):
        a = ol.pre_processor(arr, mx)
        b = ol.pre_processor_numpy(arr, mx)
        assert a.shape == arr.shape and (a == b).all(), (name, mx)


def test_oracle_pre_processor_quirks():
    x = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 5e-324, 1.0, 2.0, -2.0], dtype=np.float64)
    q = ol.pre_processor(x)
    assert q[0] == 255 and q[2] == 255 and q[3] == 255 and q[4] == 255 and q[5] == 255   # NaN, -inf, zeros, subnormal
    assert q[1] == 0                                                                  # +inf -> ALWAYS_FILL
    assert q[7] == 254 and q[8] == 0 and q[6] == int((1.0 + 2.0) / 4.0 * 254)          # min -2, max 2
    # folds are seeded with zero: an all-positive array is scaled from 0, not from its minimum
    y = np.array([10.0, 20.0], dtype=np.float64)
    assert ol.pre_processor(y).tolist() == [127, 254]
    with pytest.raises(AssertionError):
        ol.pre_processor(y, 255)
    with pytest.raises(AssertionError):
        ol.pre_processor(y, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,arr", _cases(), ids=[c[0] for c in _cases()])
def test_gpu_pre_processor_bit_exact(name, arr):
    ge.build_hip()
    pkg = ge.load_package()
    ws = pkg.TransformBuilder.default().build_segmenting()
    for mx in (254, 127, 1):
        got = ws.pre_processor_with_max(arr, mx)
        assert got.dtype == np.uint8 and got.shape == arr.shape
        assert (got == ol.pre_processor(arr, mx)).all(), (name, mx)
    assert (ws.pre_processor(arr) == ol.pre_processor(arr, 254)).all()


@pytest.mark.gpu
def test_gpu_pre_processor_large_and_pipeline():
    # tests/integration.rs:189-204 shape: Poisson f64 field -> pre_processor -> find_local_minima -> transform
    ge.build_hip()
    pkg = ge.load_package()
    rng = np.random.default_rng(11)
    field = rng.poisson(0.85, (1000, 1000)).astype(np.float64) + rng.random((1000, 1000)) * 1e-3
    ws = pkg.TransformBuilder.default().build_merging()
    img = ws.pre_processor(field)
    assert (img == ol.pre_processor(field)).all()
    seeds = ws.find_local_minima(img)
    assert (seeds == ol.find_local_minima(img)).all()
    seg = pkg.TransformBuilder.default().build_segmenting().transform(img, seeds)
    assert (seg == ol.segment_arrival(img, seeds)).all()
    with pytest.raises(AssertionError):
        ws.pre_processor_with_max(field, 255)


# ---- range overflow: max - min = +inf, the reference panics (lib.rs:1164) ------------------------------------------------------

import warnings

import preproc_cases as pc


@pytest.mark.parametrize("name,arr", pc.overflow_arrays(), ids=[c[0] for c in pc.overflow_arrays()])
def test_oracle_pre_processor_range_overflow_is_a_reference_panic(name, arr):
    with np.errstate(all="ignore"):
        assert not np.isfinite(np.nanmax(arr[np.isfinite(arr)]) - np.nanmin(arr[np.isfinite(arr)]))
    with warnings.catch_warnings():
        warnings.simplefilter("error")                       # the numpy twin refuses before it casts a NaN
        for mx in (254, 127, 1):
            with pytest.raises(ol.ReferencePanics, match="lib.rs:1164"):
                ol.pre_processor(arr, mx)
            with pytest.raises(ol.ReferencePanics, match="lib.rs:1164"):
                ol.pre_processor_numpy(arr, mx)
    # not the exception of a bad MAX, and a bad MAX is still reported as before (and first, as the reference asserts first)
    assert not issubclass(ol.ReferencePanics, AssertionError)
    with pytest.raises(AssertionError):
        ol.pre_processor(arr, 255)


def test_oracle_pre_processor_near_miss_of_the_overflow_is_quantised():
    arr = np.array(pc.NEAR_MISS, dtype=np.float64)
    assert np.isfinite(arr.max() - arr.min()) and arr.max() - arr.min() > 1.7e308
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for mx in (254, 127, 1):
            a = ol.pre_processor(arr, mx)
            assert (a == ol.pre_processor_numpy(arr, mx)).all()
            assert a[0] == 0 and a[1] == mx
    assert ol.pre_processor(arr, 254).tolist() == [0, 254, 127, 127]


def test_oracle_pre_processor_other_dtypes_cannot_overflow():
    # the widest range of every other type is exact and far below DBL_MAX in f64
    for arr in (np.array([np.finfo(np.float32).max, -np.finfo(np.float32).max], dtype=np.float32),
                np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max], dtype=np.int32)):
        assert (ol.pre_processor(arr) == ol.pre_processor_numpy(arr)).all()
        assert ol.pre_processor(arr).tolist() == [254, 0] or ol.pre_processor(arr).tolist() == [0, 254]


# ---- the inputs of the GPU tests (tests/test_gpu_pre_processor.py), checked here for what they claim ---------------------------

def test_rounding_set_tells_reordered_arithmetic_from_the_reference():
    """The reference's order is (v - min) / range, then * MAX, then truncate.  Over the rounding set a kernel that multiplies
    first, and one that multiplies by 1 / range, must each get at least one element wrong -- otherwise a bit-exact GPU
    comparison on the set could not notice them."""
    mul_first, recip = pc.reordered_counts()
    print(f"elements wrong with (v-min)*MAX/range: {mul_first}; with (v-min)*(1/range)*MAX: {recip}")
    assert mul_first > 0 and recip > 0
    # the two restatements agree on the whole set, whatever the input type
    for tag, a in pc.rounding_cases():
        for mx in pc.ROUNDING_MAX:
            assert (ol.pre_processor(a, mx) == ol.pre_processor_numpy(a, mx)).all(), (tag, mx)


@pytest.mark.parametrize("n", pc.PLACED_N)
def test_placed_extrema_cover_every_index_in_both_roles(n):
    idx, pairs = pc.placed_indices(n), pc.placed_pairs(n)
    if n == 1:
        assert pairs == [] and [t for t, _ in pc.placed_cases(1, "int16")] == [(0, None), (None, 0)]
        return
    assert {p for p, _ in pairs} == set(idx) and {q for _, q in pairs} == set(idx)
    for role in (0, 1):
        for i in idx:
            partners = [pq[1 - role] for pq in pairs if pq[role] == i]
            assert all(b != i for b in partners)
            if n > 64:                                        # a second wave exists: some partner sits in another one
                assert any(b // 64 != i // 64 for b in partners), (n, role, i)
    for dtype in pc.SIGNED:
        for (p, q), a in pc.placed_cases(n, dtype):
            assert a.dtype == np.dtype(dtype) and a.size == n
            assert a.argmin() == p and a.argmax() == q and (a == pc.LOW).sum() == 1 and (a == pc.HIGH).sum() == 1
            want = np.full(n, 127, dtype=np.uint8)
            want[p], want[q] = 0, 254
            assert (ol.pre_processor(a) == want).all()
    # one lost extreme changes every mid pixel: 50 without the minimum, 254 without the maximum
    assert ol.pre_processor(pc.placed(n, "int16", None, idx[-1]))[0] == 50
    assert ol.pre_processor(pc.placed(n, "int16", idx[0], None))[-1] == 254


def test_variant_and_edge_cases_agree_between_the_restatements():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for tag, a in pc.variant_cases() + pc.value_edge_cases():
            for mx in (254, 1):
                assert (ol.pre_processor(a, mx) == ol.pre_processor_numpy(a, mx)).all(), (tag, mx)
    edge = dict(pc.value_edge_cases())
    assert ol.pre_processor(edge["f64-tiny-and-predecessor"]).tolist()[:2] == [0, 255]      # normal: quantised; subnormal: NEVER_FILL
    assert ol.pre_processor(edge["f64-max-alone"]).tolist() == [254] and ol.pre_processor(edge["f64-lowest-alone"]).tolist() == [0]
    q = ol.pre_processor(edge["f32-subnormals"])
    assert q[-1] == 254 and (q != 255).all() and (np.diff(q.astype(int)) >= 0).all()      # normal as f64: quantised, not NEVER_FILL


def test_per_block_extremes_layout():
    for blocks in (4095, 4096):
        a = pc.per_block_extremes(blocks)
        owner = (np.arange(a.size) // 256) % blocks            # the k_minmax block an element belongs to
        hi = np.full(blocks, -10 ** 6)
        lo = np.full(blocks, 10 ** 6)
        np.maximum.at(hi, owner, a.astype(np.int64))
        np.minimum.at(lo, owner, a.astype(np.int64))
        assert np.unique(hi).size == blocks and np.unique(lo).size == blocks
        assert hi.argmax() == 300 and lo.argmin() == blocks - 1
