"""Inputs of the pre-processor tests (tests/test_pre_processor.py on the CPU, tests/test_gpu_pre_processor.py on the GPU): built
from numpy alone, so that the CPU tests can check what the arrays are claimed to contain before a kernel ever sees them.

The kernels' geometry these cases are laid out against (rustronomy-watershed_amd/csrc/ws_preproc.hip):
  k_minmax        256 threads = 4 waves of 64 lanes a block, B = min(ceil(n / 2048), 4096) blocks, element i belongs to thread
                  i % 256 of block (i / 256) % B: a shuffle tree per wave, 4 waves through LDS, one (min, max) partial a block
  k_minmax_final  one block of 256 threads walks the B partials with i += 256
  k_quantise      Q = min(ceil(n / 1024), 16384) blocks of 256, the same grid-stride loop
"""
import numpy as np

MID, LOW, HIGH = 1, -3, 5          # placed extrema: at MAX 254 the mid pixels are 127; 50 without the minimum, 254 without the maximum
MINMAX_CAP = 4096 * 2048           # elements from which k_minmax runs PREPROC_BLOCKS blocks (each thread: 8 trips, more beyond)
QUANTISE_CAP = 16384 * 1024        # elements from which k_quantise runs 16384 blocks (each thread: 4 trips, more beyond)

PLACED_N = (1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097, 2048 * 5 + 3)
SIGNED = ("float64", "float32", "int32", "int16")
UNSIGNED = ("uint8", "uint16")

OVERFLOW = [                       # max - min = +inf: the reference panics (lib.rs:1164)
    ("1e308", [-1e308, 1e308, 1.0, -3.0]),
    ("1.7e308", [-1.7e308, 1.7e308, 1.0]),
    ("1e308_specials", [np.nan, -1e308, np.inf, 1e308, -np.inf, 1.0, -3.0, np.nan]),
    ("1.7e308_specials", [-np.inf, -1.7e308, np.nan, 1.7e308, 1.0, np.inf]),
]
NEAR_MISS = [-8.9e307, 8.9e307, 1.0, -1.0]      # range 1.78e308 < DBL_MAX: finite


def overflow_arrays():
    out = [(name, np.array(v, dtype=np.float64)) for name, v in OVERFLOW]
    far = np.full(4099, 1.0)       # the two values that overflow sit in different blocks of the fold (3 blocks)
    far[3000] = -1e308
    far[4098] = 1e308
    out.append(("far_apart", far))
    return out


def placed_indices(n):
    return [i for i in sorted({0, 1, 31, 32, 63, 64, 127, 128, 191, 192, 255, 256, n - 2, n - 1}) if 0 <= i < n]


def placed_pairs(n):
    """(p, q) = (index of the minimum, index of the maximum): every index of placed_indices(n) occurs as p and as q, each time
    with the other extreme in another wave (i // 64 differs) -- where n has a second wave; within the one wave otherwise."""
    idx = placed_indices(n)
    pairs = []
    for k, a in enumerate(idx):
        rot = idx[k + len(idx) // 2:] + idx[:k + len(idx) // 2]      # start half a list away: partners spread over the waves
        others = [b for b in rot if b != a]
        far = [b for b in others if b // 64 != a // 64]
        if not (far or others):
            continue                                               # n == 1
        b = (far or others)[0]
        pairs += [(a, b), (b, a)]
    return sorted(set(pairs))


def placed(n, dtype, p=None, q=None):
    """Constant MID with the unique minimum LOW at p and the unique maximum HIGH at q (None: that extreme is absent, the
    fold's seed 0 stands in)."""
    a = np.full(n, MID, dtype=dtype)
    if p is not None:
        a[p] = LOW
    if q is not None:
        a[q] = HIGH
    return a


def placed_cases(n, dtype):
    """All placed-extrema arrays of one (n, dtype): [(tag, array)]."""
    out = []
    if dtype in SIGNED:
        out += [((p, q), placed(n, dtype, p, q)) for p, q in placed_pairs(n)]
        if n == 1:
            out += [((0, None), placed(1, dtype, 0, None))]
    if dtype in UNSIGNED or n == 1:
        out += [((None, q), placed(n, dtype, None, q)) for q in placed_indices(n)]
    return out


def flanked(n, dtype, p, q):
    """placed(), each extreme's neighbours NaN, +inf, -inf (those that exist and are not the other extreme)."""
    a = placed(n, dtype, p, q)
    specials = [np.nan, np.inf, -np.inf, np.nan]
    k = 0
    for centre in (p, q):
        for d in (-1, 1, -2, 2):
            j = centre + d
            if 0 <= j < n and j not in (p, q):
                a[j] = specials[k % 4]
                k += 1
    return a


def variant_cases():
    """[(tag, array)]: the extremes among non-finite neighbours, one finite value among non-finite ones, all equal, all negative."""
    out = []
    for dtype in ("float64", "float32"):
        for n, p, q in ((65, 63, 64), (65, 64, 1), (257, 255, 128), (257, 256, 0), (2049, 2048, 191), (2049, 32, 2047), (4097, 4095, 256)):
            out.append((f"flanked-{dtype}-{n}-{p}-{q}", flanked(n, dtype, p, q)))
        for fill in (np.nan, np.inf, -np.inf):
            for n, at, v in ((1, 0, 5.0), (64, 63, -3.0), (257, 256, 5.0), (300, 129, -3.0), (2049, 2048, 5.0), (2049, 700, -3.0)):
                a = np.full(n, fill, dtype=dtype)
                a[at] = v
                out.append((f"lone-{dtype}-{fill}-{n}-{at}", a))
    for dtype in SIGNED + UNSIGNED:
        for n in (1, 65, 257, 2049):
            out.append((f"equal-{dtype}-{n}", np.full(n, 7, dtype=dtype)))
    for dtype in SIGNED:
        for n in (1, 65, 257, 2049):
            out.append((f"negative-{dtype}-{n}", (-(1 + np.arange(n) % 5)).astype(dtype)))
    return out


# ---- rounding order ----------------------------------------------------------------------------------------------------------
# Integer-valued inputs 0..R and -(R // 2)..R - R // 2: (v - min) is an exact integer k and range = R, so the reference computes
# trunc(fl(fl(k / R) * MAX)).  Wherever k * MAX / R is an integer j the two roundings may land just below j where another order
# of the same operations lands on it.  R = 253, 506, 1012 are additions to the set the tests were specified with: over that set
# a kernel that multiplies first never differs (its product k * MAX is exact, so it needs fl(fl(j / MAX) * MAX) < j, and of the
# five MAX values only 253 has such j, reached only when R is a multiple of 253).
ROUNDING_R = (3, 7, 49, 127, 253, 254, 255, 506, 508, 1000, 1012, 65535)
ROUNDING_MAX = (1, 2, 127, 253, 254)


def rounding_cases():
    """[(tag, array)] over f64, f32, i32, and u16 where the values fit."""
    out = []
    for r in ROUNDING_R:
        for lo in (0, -(r // 2)):
            v = np.arange(lo, lo + r + 1, dtype=np.int64)
            for dtype in ("float64", "float32", "int32") + (("uint16",) if lo == 0 else ()):
                out.append((f"R{r}-from{lo}-{dtype}", v.astype(dtype)))
    return out


def reordered_counts():
    """How many elements of the rounding set (f64 arrays, every MAX) a kernel with another operation order gets wrong:
    (multiply before dividing, multiply by the reciprocal of the range)."""
    mul_first = recip = 0
    for tag, a in rounding_cases():
        if a.dtype != np.float64:
            continue
        mn, mx = min(0.0, a.min()), max(0.0, a.max())
        rng = mx - mn
        live = a != 0                                     # exact zeros are NEVER_FILL whatever the arithmetic
        for m in ROUNDING_MAX:
            ref = np.trunc(((a - mn) / rng) * m)
            mul_first += int(((np.trunc((a - mn) * m / rng) != ref) & live).sum())
            recip += int(((np.trunc((a - mn) * (1.0 / rng) * m) != ref) & live).sum())
    return mul_first, recip


def value_edge_cases():
    tiny = np.finfo(np.float64).tiny                      # 2.2250738585072014e-308
    big = np.finfo(np.float64).max                        # 1.7976931348623157e308
    f32 = np.finfo(np.float32)
    sub32 = (np.arange(1, 257, dtype=np.float64) * 2.0 ** -149).astype(np.float32)      # every f32 subnormal step 1..256: normal as f64
    assert (sub32 > 0).all() and (sub32 < f32.tiny).all() and np.unique(sub32).size == 256
    return [
        ("f64-tiny-and-predecessor", np.array([tiny, np.nextafter(tiny, 0.0), 1.0, -tiny, -np.nextafter(tiny, 0.0)])),
        ("f64-tiny-alone", np.array([tiny, np.nextafter(tiny, 0.0)])),
        ("f64-max-alone", np.array([big])),
        ("f64-lowest-alone", np.array([-big])),
        ("f64-max-among-small", np.array([1.0, big, 2.0, 0.5 * big])),
        ("f64-negative-zero", np.array([-0.0, 1.0, -1.0, 0.0])),
        ("f32-subnormals", sub32),
        ("f32-subnormals-and-one", np.concatenate([sub32, np.array([1.0, -1.0], dtype=np.float32)])),
        ("f32-min-max", np.array([f32.tiny, f32.max, -f32.max, -f32.tiny, 1.0], dtype=np.float32)),
        ("i32-limits", np.array([np.iinfo(np.int32).min, np.iinfo(np.int32).max, 1, -1, 0], dtype=np.int32)),
        ("i16-limits", np.array([-32768, 32767, 1, -1, 0], dtype=np.int16)),
        ("u16-limits", np.array([0, 65535, 1, 32768], dtype=np.uint16)),
        ("u8-limits", np.array([0, 255, 1, 128], dtype=np.uint8)),
    ]


# ---- beyond the block caps ---------------------------------------------------------------------------------------------------

def beyond_cap_cases():
    """[(tag, array)], made on demand (up to 34 MB each).  The extremes lie at indices >= the cap, where only the trips that a
    capped grid adds reach them."""
    n0, q0 = MINMAX_CAP, QUANTISE_CAP

    def one_past_min():                # n0 + 1 has ONE index past the cap: the minimum alone, then the maximum alone
        return placed(n0 + 1, np.int16, n0, None)

    def one_past_max():
        return placed(n0 + 1, np.int16, None, n0)

    def block_past():
        return placed(n0 + 2049, np.int16, n0 + 5, n0 + 2048)

    def quantise_past():               # not constant: a k_quantise trip that is skipped, repeated or shifted changes bytes
        a = (np.arange(q0 + 1025, dtype=np.int64) % 251 - 100).astype(np.int16)
        a[q0 + 3] = -3000
        a[q0 + 1024] = 5000
        return a

    def f32_past():
        a = placed(n0 + 1, np.float32, 77, n0)
        a[n0 - 1] = np.nan
        return a

    return [("i16-cap+1-min", one_past_min), ("i16-cap+1-max", one_past_max), ("i16-cap+2049", block_past),
            ("i16-quantise-cap+1025", quantise_past), ("f32-cap+1", f32_past)]


def per_block_extremes(blocks):
    """n = blocks * 2048 i16 elements (blocks <= 4096: exactly that many k_minmax blocks), MID everywhere but two elements in
    every block's region: block b's own maximum 2 + (b - 301) % blocks and its own minimum -(2 + b), in lanes that move with b.
    The global maximum is block 300's partial, the global minimum the last block's; every partial is distinct."""
    assert blocks <= 4096 and blocks > 301
    a = np.full(blocks * 2048, MID, dtype=np.int16)
    b = np.arange(blocks)
    trip = b % 8                                            # block b owns elements (t * blocks + b) * 256 + lane, t = 0..7
    a[(trip * blocks + b) * 256 + b % 256] = 2 + (b - 301) % blocks
    a[(((trip + 3) % 8) * blocks + b) * 256 + (b * 7 + 128) % 256] = -(2 + b)
    return a
