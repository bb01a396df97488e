"""What ws_merge_tree_from_arrival_device rests on, proved on the CPU oracle alone: a pixel is a seed pixel exactly when its
arrival stamp is 0, the label there is the colour that survived seeding (lib.rs:1670-1677), and the colours without such a
pixel are the ones that "do not exist" in the sense of ws_merge_tree -- so the seed list need not be passed, it is in the planes.
Over every input of tests/tiled_cases.py and the duplicate, shuffled and level-0-death inputs of tests/merging_cases.py and
tests/lake_stats_batch_cases.py; and that the set reaches the regimes the arrival and tiled forms have to get right.  Also the
boundary: the four new entry points are declared in every layer."""
import os
import re

import numpy as np
import pytest

import __graft_entry__ as ge
import lake_stats_batch_cases as lbc
import merge_tree_ref as mt
import merging_cases as mc
import oracle_lib as ol
import tiled_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ws_merge_tree_from_arrival_device", "ws_merge_tree_tiled_device", "ws_merge_tree_tiled2d_device", "ws_merge_tree_tiled")
NEVER = np.uint64(0xFFFFFFFFFFFFFFFF)      # the oracle's stamp of a pixel that is never coloured (its stamps are u64)


def _inputs():
    """(name, image, seeds in the image's own plane, max_level, world or 0): edge-corrected cases as the plain call they equal."""
    out = []
    for name, img, seeds, world in tc.all_cases():
        edge, shift = tc.edge_options(name)
        if edge:
            img, seeds = tc.padded_equivalent(img, seeds, shift)
        out.append((name, np.ascontiguousarray(img), np.asarray(seeds, dtype=np.int64).reshape(-1, 2), 254, world))
    rng = np.random.default_rng(20)
    for kind in ("few", "walls", "noise"):
        for form in ("shuffled", "repeats", "borders"):
            h, w = int(rng.integers(40, 70)), int(rng.integers(50, 90))
            img = mc.make_field(kind, h, w, rng)
            out.append((f"mc/{kind}/{form}", img, mc.make_seeds(form, h, w, h * w // 25, rng), 254 if kind != "few" else 60, 0))
    for case in (mc.seeded_plateau(516), mc.seeded_plateau(517)):      # mass deaths at level 0
        out.append((f"mc/{case.name}", case.img, case.seeds, case.max_level, 0))
    imgs, lists, dying = lbc.level_zero_death_case()
    for k, _ in dying:
        out.append((f"lbc/level0/slice{k}", imgs[k], lists[k], 254, 0))
    return out


INPUTS = _inputs()


def _painted(seeds, shape):
    paint = np.zeros(shape, dtype=np.int64)
    for i, (r, c) in enumerate(seeds):
        paint[r, c] = i + 1
    return paint


def test_the_input_set_is_the_one_the_issue_names():
    assert sum(1 for i in INPUTS if i[4]) == len(tc.all_cases()) == 110
    assert {tc.form_of(i[0]) for i in INPUTS if i[4]} == set(tc.FORMS)


@pytest.mark.parametrize("name,img,seeds,max_level,world", INPUTS, ids=[i[0] for i in INPUTS])
def test_stamp_zero_marks_the_seed_pixels(name, img, seeds, max_level, world):
    labels, keys = ol.segment_arrival(img, seeds.astype(np.uint64), max_level=max_level, want_keys=True)
    paint = _painted(seeds, img.shape)
    assert ((keys == 0) == (paint > 0)).all(), name
    at = paint > 0
    assert (labels[at].astype(np.int64) == paint[at]).all(), name
    # the colours that own a stamp-0 pixel are exactly the ones that exist; each owns ONE (no two pixels write the same pair)
    owners = np.bincount(labels[keys == 0].astype(np.int64), minlength=len(seeds) + 1)
    assert owners[0] == 0 and owners.max() <= 1, name
    ex = mt.existing(seeds, img.shape)
    assert ((owners == 0)[1:] == ~ex[1:]).all(), name


def test_the_inputs_reach_every_regime():
    never_was = last_pixel = uncoloured_low = uncoloured_wall = seam = halo = False
    for name, img, seeds, max_level, world in INPUTS:
        h, w = img.shape
        never_was |= bool((~mt.existing(seeds, img.shape)[1:]).any())
        last_pixel |= bool(((seeds[:, 0] == h - 1) & (seeds[:, 1] == w - 1)).any())
        keys = ol.segment_arrival(img, seeds.astype(np.uint64), max_level=max_level, want_keys=True)[1]
        dry = img[1:-1, 1:-1][keys[1:-1, 1:-1] == NEVER]      # interior pixels never coloured (the border never floods anyway)
        uncoloured_low |= bool(((dry > max_level) & (dry != 255)).any())
        uncoloured_wall |= bool((dry == 255).any())
        if world:
            rows = set(int(r) for r in seeds[:, 0])
            seam |= bool(rows & set(tc.seam_rows(h, world)))
            for r in range(world):
                r0, r1, lo, hi = tc.tile_rows(h, r, world)
                halo |= bool(rows & ({lo} if lo < r0 else set())) or bool(rows & ({hi - 1} if hi > r1 else set()))
    assert never_was and last_pixel and uncoloured_low and uncoloured_wall and seam and halo, \
        (never_was, last_pixel, uncoloured_low, uncoloured_wall, seam, halo)


def test_a_colour_dies_at_level_zero():
    imgs, lists, dying = lbc.level_zero_death_case()
    assert dying
    for k, colour in dying:
        parent, death, area, leaves, _, ex = mt.expected_tree(imgs[k], lists[k])
        assert ex[colour] and death[colour] == 0 and area[colour] == 1 and leaves[colour] == 1 and 0 < parent[colour] < colour


def test_the_new_entry_points_are_declared_in_every_layer():
    pkg = ge.load_package()
    header = open(os.path.join(ROOT, "include", "ws_hip.h")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "hip_ffi.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"^int\s+%s\(" % name, header, flags=re.M), name
        assert name in pkg._ffi.SIGNATURES, name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert re.search(r"pub fn %s\(\.\.\);" % name, doc), name
    assert re.search(r"#define WS_ABI_VERSION 3\b", header)
    ge.build_hip()
    assert pkg._ffi.lib().ws_abi_version() == 3
    for name in NEW:
        assert getattr(pkg._ffi.lib(), name) is not None
