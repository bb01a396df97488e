#!/usr/bin/env python3
"""How many references of k_resolve_local end at a halo pixel that is a seed -- the chains that take the seed's colour
inside the kernel instead of a place on the work lists of k_resolve_chase.  Counted on the CPU from the oracle's arrival
stamps of the bench generator's field (seed 1, seeds = its local minima); the in-tile forest is cut as
tests/halo_seed_refs.py cuts it.

  tools/count_halo_seed_refs.py SIDE [SIDE ...]        (profiles/halo_seeds_ref_counts.txt: 1024 2048)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import halo_seed_refs as hs      # noqa: E402
import oracle_lib as ol          # noqa: E402


def main():
    sides = [int(a) for a in sys.argv[1:]] or [1024]
    ol.build()
    for n in sides:
        img = ol.random_field(n, n, 1)
        seeds = ol.find_local_minima(img)
        _, keys = ol.segment_arrival(img, seeds, want_keys=True)
        c = hs.counts(hs.leaving_chains(keys))
        refs, hit = c["references"], c["at_halo_seed"]
        print(f"{n} x {n}, {len(seeds)} seeds")
        print(f"  references            {refs:9d}   {100.0 * refs / c['pixels']:.2f} % of all pixels")
        print(f"  end at a halo seed    {hit:9d}   {100.0 * hit / max(refs, 1):.1f} % of the references")
        for s in hs.SIDE_NAMES:
            a, b = c["by_side"][s]
            print(f"    side {s}              {a:9d}   at a halo seed {b:9d}   {100.0 * b / max(a, 1):.1f} %")
        print(f"  references per 64 x 16 region: mean {c['region_mean_before']:.1f} (max {c['region_max_before']})"
              f" -> {c['region_mean_after']:.1f} (max {c['region_max_after']})")


if __name__ == "__main__":
    main()
