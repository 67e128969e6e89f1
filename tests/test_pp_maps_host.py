"""Conditions on the engineered post-processing maps of tests/pp_maps.py, checked without a GPU: the maps of tests/test_postproc_tiers_gpu.py
are only worth running if the reference alone says that they reach the flood tiers, caps, ties and seams they are named after.  Every figure
comes from pp_maps.predict_tiers (a CPU restatement of the nuclei front on the oracle's stage entries) and from the C oracle itself."""
import numpy as np
import pytest

import pp_maps as P
from oracle import postproc_ref as pr
from oracle import synth


@pytest.fixture(scope="module")
def maps():
    return {(name, kind): fn(kind) for name, fn in (("tier", P.tier_map), ("cap", P.cap_map)) for kind in ("distinct", "tied")}


def test_tier_rule_first_match_wins():
    assert P.tier_rule(512, 1024, 5000) == "tiny" and P.tier_rule(513, 1024, 5000) == "small" and P.tier_rule(512, 1025, 5000) == "small"
    assert P.tier_rule(1024, 2304, 5000) == "small" and P.tier_rule(1025, 2304, 5000) == "big" and P.tier_rule(1024, 2305, 5000) == "big"
    assert P.tier_rule(2048, 16384, 5000) == "big" and P.tier_rule(2049, 16384, 1024) == "lds" and P.tier_rule(2048, 16385, 1025) == "global"


@pytest.mark.parametrize("kind", ["distinct", "tied"])
def test_tier_map_has_a_component_in_every_tier(maps, kind):
    m, n_markers, at = maps[("tier", kind)]
    comps, counts = P.predict_tiers(m)
    print("tier map (%s): %s" % (kind, counts))
    for name, first in sorted(at.items()):
        print("  %-8s %s" % (name, comps[first]))
        assert comps[first][0] == name
    assert all(counts[t] >= 1 for t in P.TIERS + ("single", "none"))
    # the figures DESIGN.md quotes
    assert comps[at["tiny"]][1:4] == (376, 468, 384) and comps[at["small"]][1:4] == (857, 999, 875)
    assert comps[at["big"]][1:4] == (1896, 6324, 6000) and comps[at["lds"]][2] == 18769 and comps[at["global"]][1:4] == (6388, 6724, 6400)


@pytest.mark.parametrize("kind", ["distinct", "tied"])
def test_cap_map_sits_on_every_cap_and_one_past_it(maps, kind):
    m, n_markers, at = maps[("cap", kind)]
    comps, counts = P.predict_tiers(m)
    limits = {"tiny": (512, 1024), "small": (1024, 2304), "big": (2048, 16384)}
    field = {"need": 1, "win": 2, "area": 3}
    for name, tier_at, tier_past, what, v_at, v_past in P.CAPS:
        a, b = comps[at[name + "@"]], comps[at[name + "+"]]
        print("cap %-9s at: %-6s need %4d win %5d area %4d | past: %-6s need %4d win %5d area %4d" % ((name,) + a[:4] + b[:4]))
        assert a[0] == tier_at and b[0] == tier_past, (name, a, b)
        assert a[field[what]] == v_at and b[field[what]] == v_past, (name, a, b)
        if what == "area":  # LDS heap: reached only past the big window, whatever `need` is
            assert a[2] > 16384 and b[2] > 16384
        else:  # every other figure inside the tier, so that the one named decides
            other = 2 if what == "need" else 1
            lim = limits[tier_at][other - 1]
            assert a[other] <= lim and b[other] <= lim, (name, a, b)
        assert a[4] >= 2 and b[4] >= 2
    assert all(counts[t] >= 1 for t in P.TIERS)


def test_distinct_maps_hold_no_equal_values_and_tied_maps_do(maps):
    for (name, kind), (m, _, _) in maps.items():
        if kind == "distinct":
            assert P.distinct_within_components(m), name
            assert P.tied_seed_pairs(m) == 0
        else:
            assert P.tied_seed_pairs(m) >= 1, name
    assert P.distinct_within_components(P.seam_map()[0]) and P.distinct_within_components(P.nuclei_threshold_map()[0])


def test_oracle_labels_every_map_with_one_instance_per_marker(maps):
    for (name, kind), (m, n_markers, _) in maps.items():
        ref = pr.proc(m, "Nuclei")
        assert ref.dtype == np.int32 and int(ref.max()) == n_markers == len(np.unique(ref)) - 1, (name, kind)
        assert P.front(m)[4] == n_markers
        assert P.predict_tiers(np.pad(m, ((0, 0), (0, 1), (0, 0))))[1] == P.predict_tiers(m)[1]  # a zero column changes no tier
    m, n_markers, at, masks = P.seam_map()
    ref = pr.proc(m, "Nuclei")
    assert int(ref.max()) == n_markers == len(np.unique(ref)) - 1 == P.front(m)[4]
    m, n_markers = P.nuclei_threshold_map()
    ref = pr.proc(m, "Nuclei")
    assert int(ref.max()) == n_markers == P.front(m)[4] and len(np.unique(ref)) - 1 == n_markers - 2  # the two 7-px components carry no label


def test_seam_map_crosses_the_seams():
    m, _, at, masks = P.seam_map()
    comp = P.front(m)[0]
    comps, _ = P.predict_tiers(m)
    for name, want in masks.items():
        c = comp[at[name]]
        assert c > 0 and (comp[want] == c).all(), name  # one component holds the whole shape
    sx = (63, 64, 127, 128, 191, 192)
    s = masks["serpentine"]
    assert all(s[:, x].sum() >= 10 for x in sx) and s[31:33].all(axis=0).sum() >= 1          # ten runs over every vertical seam, one joint over y = 32
    assert (s.sum(0)[3:-3] == 10).all() and (s[:, 3:-3].sum(1) <= 194).all()                 # one pixel wide
    t = masks["serpentine_t"]
    assert t[63].sum() >= 7 and t[64].sum() >= 7 and t[95].sum() >= 7 and t[96].sum() >= 7
    c = masks["comb"]
    assert c[54:64].any() and c[66:75].any() and c[64:66, 36:116].all() and c[:, 60].sum() > 2 and c[:, 66].sum() > 2
    # the marker front: holes over x = 128 and y = 64 filled (their 2 x 2 markers swallowed), the U on the last row not
    mk = m[..., 0] > 0.5
    markers = P.front(m)[1]
    assert not mk[50, 127] and not mk[50, 128] and markers[50, 127] == markers[50, 128] == markers[46, 124] > 0
    assert not mk[63, 144] and not mk[64, 144] and markers[63, 144] == markers[64, 144] == markers[58, 142] > 0
    assert markers[80, 130] == markers[74, 124] > 0                                           # ring in a ring: one marker
    assert markers[98, 44] == 0 and markers[96, 45] > 0 and markers[96, 45] != markers[92, 42] > 0
    assert comps[at["rings"]][4] == 5 and comps[at["border_ring"]][4] == 2


@pytest.mark.parametrize("tissue,ds", [("Gland", 1.0), ("Gland", 0.5), ("Lumen", 1.0), ("Lumen", 0.5)])
def test_gland_lumen_maps_sit_on_min_size(tissue, ds):
    thr, min_size, ksize, pad = P.gl_params(tissue, ds)
    assert (tissue, ds, min_size) in (("Gland", 1.0, 1000), ("Gland", 0.5, 250), ("Lumen", 1.0, 150), ("Lumen", 0.5, 37))
    m, n_inst, mid = P.gl_area_map(tissue, ds)
    fg = (m[..., 0] - (m[..., 1] > 0.5)) > np.float32(thr)
    lab, n = pr.label4(fg)
    areas = sorted(np.bincount(lab.ravel())[1:].tolist())
    assert areas[0] == min_size - 1 and areas.count(min_size) == 3, areas
    ref = pr.proc(m, tissue, ds)
    assert int(ref.max()) == n_inst == n - 1
    assert ref[mid["open"]] == 0 and (ref[mid["closed"]] > 0) == (ksize >= 2)  # a 1 x 1 element dilates nothing
    if ksize >= 2:  # the pair's dilations overlap: pixels between them carry the later id
        ids = np.unique(ref[lab == 0])
        assert len(ids) > 1
    for d in (pad - 1, pad, pad + 1):
        b = P.gl_border_map(tissue, ds, d)
        assert int(pr.proc(b, tissue, ds).max()) == 1


def test_tiny_maps_are_not_all_empty():
    """(Gland and lumen have nothing to keep below 150 pixels: their tiny maps check the empty paths.)"""
    n = sum(int(pr.proc(P.tiny_map(h, w), "Nuclei").max() > 0) for h, w in P.TINY_SIZES)
    assert n >= 5, n


def test_census_of_the_random_map():
    """Which tiers the suite's seeded random map reaches (printed; a statement of fact for DESIGN.md, not a condition)."""
    _, counts = P.predict_tiers(synth.nuclei_maps(512, 512, 31, 1500.0, noise=0.02))
    print("tier census of synth.nuclei_maps(512, 512, 31, 1500.0, noise=0.02): %s" % counts)
