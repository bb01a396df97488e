"""The leaving chains of the two-launch label resolve (csrc/ws_resolve.hip), from the oracle's arrival stamps alone.

k_resolve_local collapses the parent forest inside every 64 x 64 tile; a pixel whose chain leaves its tile holds a
REFERENCE to the halo pixel where it leaves -- unless that halo pixel is a seed, in which case (seed tables, 16-byte
path) it holds the seed's colour at once.  `leaving_chains` says, per pixel: does its chain leave the tile, through
which side, and is the halo pixel it leaves to a seed.  tests/test_gpu_resolve_halo_seeds.py checks with it that its inputs
reach that code; tools/count_halo_seed_refs.py counts with it what the colours take off the work lists."""
import numpy as np

TS, REGION_ROWS = 64, 16
NEVER = np.uint64(0xFFFFFFFFFFFFFFFF)
UP, DOWN, LEFT, RIGHT = 0, 1, 2, 3
SIDE_NAMES = "UDLR"


def leaving_chains(keys):
    """keys: (h, w) uint64 arrival stamps of a finished flood (0: seed, NEVER: never coloured).  A stack of slices is the
    slices' stamp planes one above the other: a flooded pixel is an interior pixel of its slice, so no parent crosses a slice.
    Returns is_ref (h, w) bool, side (h, w) int8 (UP .. RIGHT where is_ref, else -1), at_seed (h, w) bool (the halo pixel
    where the chain leaves is a seed) and leaves_to (h, w) flat index of that halo pixel."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    h, w = keys.shape
    n = h * w
    idx = np.arange(n, dtype=np.int64).reshape(h, w)
    pad = np.full((h + 2, w + 2), NEVER, dtype=np.uint64)
    pad[1:-1, 1:-1] = keys
    k = keys
    d, r, l = pad[2:, 1:-1] < k, pad[1:-1, 2:] < k, pad[1:-1, :-2] < k
    flooded = (k != 0) & (k != NEVER)
    par = np.where(d, idx + w, np.where(r, idx + 1, np.where(l, idx - 1, idx - w)))      # first earlier neighbour in D, R, L, U
    par = np.where(flooded, par, idx).ravel()
    flat_keys = keys.ravel()
    assert (flat_keys[par[flooded.ravel()]] < flat_keys[flooded.ravel()]).all()             # a fixpoint: a parent is earlier
    tile = ((idx // w) // TS * ((w + TS - 1) // TS) + (idx % w) // TS).ravel()
    flat = idx.ravel()
    nxt = np.where(tile[par] == tile, par, flat)      # the in-tile forest; pointer jumping as the kernel does it
    while True:
        nn = nxt[nxt]
        if (nn == nxt).all():
            break
        nxt = nn
    leaves_to = par[nxt]
    is_ref = leaves_to != nxt                          # the in-tile root's parent lies in another tile
    step = leaves_to - nxt
    side = np.full(n, -1, dtype=np.int8)
    side[is_ref & (step == -w)] = UP
    side[is_ref & (step == w)] = DOWN
    side[is_ref & (step == -1)] = LEFT
    side[is_ref & (step == 1)] = RIGHT
    assert (side[is_ref] >= 0).all()
    at_seed = is_ref & (flat_keys[leaves_to] == 0)
    return {"is_ref": is_ref.reshape(h, w), "side": side.reshape(h, w), "at_seed": at_seed.reshape(h, w),
            "leaves_to": leaves_to.reshape(h, w)}


def counts(ch):
    """References, those ending at a halo seed, both by side, and references per 64 x 16 wave region before and after."""
    is_ref, at_seed, side = ch["is_ref"], ch["at_seed"], ch["side"]
    h, w = is_ref.shape
    by_side = {SIDE_NAMES[s]: (int((is_ref & (side == s)).sum()), int((at_seed & (side == s)).sum())) for s in range(4)}
    before, after = [], []
    for y0 in range(0, h, REGION_ROWS):
        for x0 in range(0, w, TS):
            sl = (slice(y0, y0 + REGION_ROWS), slice(x0, x0 + TS))
            before.append(int(is_ref[sl].sum()))
            after.append(int((is_ref[sl] & ~at_seed[sl]).sum()))
    return {"pixels": h * w, "references": int(is_ref.sum()), "at_halo_seed": int(at_seed.sum()), "by_side": by_side,
            "region_mean_before": float(np.mean(before)), "region_max_before": max(before),
            "region_mean_after": float(np.mean(after)), "region_max_after": max(after)}
