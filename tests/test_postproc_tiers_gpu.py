"""The post-processing kernels (csrc/pp_label.hip, pp_nuclei.hip, pp_gland.hip) on engineered maps (tests/pp_maps.py): every watershed flood tier, every cap of the tier rule
and one past it, ties, labelling seams and holes, the min-area thresholds at equality, and tiny maps -- bit for bit against the C oracle, scipy or
the CPU tier predictor.  tests/test_pp_maps_host.py checks, without a GPU, that the maps reach what they are named after."""
import hashlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import pp_maps as P
from cerberus_amd.postproc import postproc_device
from oracle import postproc_ref as pr

pytestmark = pytest.mark.gpu

NUCLEI_MAPS = ("tier", "cap")
_BUILD = {"tier": P.tier_map, "cap": P.cap_map}
_cache = {}


def _nuclei(name, kind, pad=0):
    """(map, oracle labels, markers placed), the oracle run once per map; pad: zero columns appended (W % 4 == 1: the one-pixel passes)."""
    key = (name, kind, pad)
    if key not in _cache:
        if name in _BUILD:
            m, n = _BUILD[name](kind)[:2]
        elif name == "seam":
            m, n = P.seam_map()[:2]
        else:
            m, n = P.nuclei_threshold_map()
        assert m.shape[1] % 4 == 0
        m = np.ascontiguousarray(np.pad(m, ((0, 0), (0, pad), (0, 0))))
        ref = pr.proc(m, "Nuclei")
        ref.setflags(write=False)
        _cache[key] = (m, ref, n)
    return _cache[key]


def _run(m, tissue="Nuclei", ds=1.0, exact_ties=True, canvas=False):
    """-> (labels, n_inst, n_ambiguous).  canvas: the map read in place as a window of a 9-channel canvas at an odd row and column."""
    if canvas:
        H, W = m.shape[:2]
        cv = torch.zeros((H + 40, W + 60, 9), dtype=torch.float32, device="cuda")
        cv[21:21 + H, 31:31 + W, 2:4] = torch.from_numpy(m).cuda()
        dev = cv[21:21 + H, 31:31 + W, 2:4]
    else:
        dev = torch.from_numpy(np.ascontiguousarray(m)).cuda()
    lab, info = postproc_device(dev, tissue, ds, exact_ties=exact_ties)
    return lab.cpu().numpy(), int(info["n_inst"].item()), int(info["n_ambiguous"].item())


# ---- (a) every tier and cap, floods unmasked --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NUCLEI_MAPS)
def test_every_tier_and_cap_without_the_replay(name):
    """Values pairwise distinct inside every component: no tie exists, so the floods alone (exact_ties=False) must give the oracle's map, flag
    nothing, and the replay (exact_ties=True) has nothing to overwrite."""
    m, ref, n = _nuclei(name, "distinct")
    got, n_inst, amb = _run(m, exact_ties=False)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, (name, len(bad), bad[:5].tolist())
    assert amb == 0 and n_inst == int(ref.max()) == n
    again, n_inst2, amb2 = _run(m, exact_ties=True)
    assert again.tobytes() == got.tobytes() and amb2 == 0 and n_inst2 == n_inst


# ---- (b) the tiers really ran -----------------------------------------------------------------------------------------------------------------------------
_CHILD = r"""
import hashlib, sys
sys.path.insert(0, sys.argv[1])
import numpy as np, torch
import pp_maps as P
from cerberus_amd.postproc import postproc_device
for name, fn in (("tier", P.tier_map), ("cap", P.cap_map)):
    m = torch.from_numpy(fn("distinct")[0]).cuda()
    for exact in (False, True):
        lab, info = postproc_device(m, "Nuclei", exact_ties=exact)
        print("LABELS", name, int(exact), hashlib.sha1(lab.cpu().numpy().tobytes()).hexdigest(), int(info["n_inst"]), int(info["n_ambiguous"]))
"""
_PROBE = re.compile(r"flood tiers: small-window (\d+), lds-heap (\d+), global-heap (\d+), big-window (\d+), tiny-window (\d+)")


def test_flood_tier_counts_equal_the_prediction():
    """The developers' library prints the components per flood tier (CERB_PP_DEBUG_COUNTS) in a fresh interpreter; the five counts of every call
    must equal pp_maps.predict_tiers, an independent count on the CPU -- which also holds the seed, floodable-pixel and box kernels and the work-list
    kernel to it -- and the labels must be the product library's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("CERB_PP_ONE_PIXEL_THREADS", None)
    env.update(CERB_DEV_LIB="1", CERB_PP_DEBUG_COUNTS="1", PYTHONPATH=root + os.pathsep + env.get("PYTHONPATH", ""))
    out = subprocess.run([sys.executable, "-c", _CHILD, os.path.join(root, "tests")], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    probes = [tuple(int(v) for v in g) for g in _PROBE.findall(out.stderr)]
    labels = [l.split()[1:] for l in out.stdout.splitlines() if l.startswith("LABELS")]
    assert len(probes) == len(labels) == 4, (probes, labels)
    for (name, exact, digest, n_inst, amb), probe in zip(labels, probes):
        m, ref, n = _nuclei(name, "distinct")
        _, c = P.predict_tiers(m)
        want = (c["small"], c["lds"], c["global"], c["big"], c["tiny"])
        print("%s exact_ties=%s: small-window, lds-heap, global-heap, big-window, tiny-window = %s (predicted %s)" % (name, exact, probe, want))
        assert probe == want and min(probe) > 0, (name, exact, probe, want)
        got, n_inst_here, amb_here = _run(m, exact_ties=bool(int(exact)))
        assert hashlib.sha1(got.tobytes()).hexdigest() == digest and (int(n_inst), int(amb)) == (n_inst_here, amb_here) == (n, 0), (name, exact)
        assert np.array_equal(got, ref)


# ---- (c) both schedules and strides -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["quads", "odd_width", "canvas"])
@pytest.mark.parametrize("name", NUCLEI_MAPS)
def test_every_schedule_and_stride(name, layout):
    """W % 4 == 0 (four pixels per thread), one zero column more (W % 4 == 1: the one-pixel passes; the same tiers), and a window of a 9-channel
    canvas at an odd row and column (strided loads)."""
    m, ref, n = _nuclei(name, "distinct", pad=1 if layout == "odd_width" else 0)
    assert m.shape[1] % 4 == (1 if layout == "odd_width" else 0)
    for exact in (False, True):
        got, n_inst, amb = _run(m, exact_ties=exact, canvas=layout == "canvas")
        bad = np.argwhere(got != ref)
        assert len(bad) == 0 and amb == 0 and n_inst == n, (name, layout, exact, len(bad), bad[:5].tolist(), amb, n_inst)


# ---- (d) ties ---------------------------------------------------------------------------------------------------------------------------------------------
def test_tied_values_through_the_replay():
    """Values rounded to 1/16: equal-valued seeds in (nearly) every component.  With the replay the map is the oracle's; the floods must have
    flagged at least one map, or the replay was not exercised; without it equality is owed wherever nothing was flagged."""
    flagged = 0
    for name in NUCLEI_MAPS:
        for pad in (0, 1):
            m, ref, n = _nuclei(name, "tied", pad)
            got, n_inst, amb = _run(m, exact_ties=True)
            bad = np.argwhere(got != ref)
            assert len(bad) == 0 and n_inst == n, (name, pad, len(bad), bad[:5].tolist(), amb)
            flagged += int(amb > 0)
            fast, _, amb_fast = _run(m, exact_ties=False)
            print("%s pad %d: n_ambiguous %d, pixels that differ without the replay %d" % (name, pad, amb_fast, int((fast != ref).sum())))
            if amb_fast == 0:
                assert np.array_equal(fast, ref), (name, pad)
    assert flagged > 0


# ---- (e) seams and holes ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1])
def test_seams_and_holes(pad):
    m, ref, n = _nuclei("seam", "distinct", pad)
    for exact in (False, True):
        got, n_inst, amb = _run(m, exact_ties=exact)
        bad = np.argwhere(got != ref)
        assert len(bad) == 0 and amb == 0 and n_inst == n == int(ref.max()), (pad, exact, len(bad), bad[:5].tolist(), amb, n_inst)


@pytest.mark.parametrize("pad", [0, 1])
def test_label_mask_on_corridors_and_comb(pad):
    """cerb_label_mask (tile labelling + seam passes) on 1-px corridors that cross every seam and on the comb: scipy's 4-connected labels."""
    from scipy import ndimage

    from cerberus_amd.tissue import TissueRegions

    masks = P.seam_map()[3]
    for names in (("serpentine",), ("comb",), ("serpentine", "serpentine_t", "comb")):
        k = np.zeros((100, 200), bool)
        for nm in names:
            k |= masks[nm]
        k = np.ascontiguousarray(np.pad(k, ((0, 0), (0, pad))).astype(np.uint8))
        want, nw = ndimage.label(k, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
        assert nw == len(names)
        lab4, n4 = pr.label4(k)
        assert n4 == nw and np.array_equal(lab4, want)
        reg = TissueRegions(torch.from_numpy(k).cuda())
        assert reg.n == nw and np.array_equal(reg.lab.cpu().numpy(), want), names


# ---- (f) thresholds at equality ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1])
def test_nuclei_min_sizes_at_equality(pad):
    """Eroded mask components of 7 (dropped) and 8 pixels, markers of 3 (dropped) and 4 pixels, alone and beside a kept neighbour."""
    m, ref, n = _nuclei("threshold", "distinct", pad)
    for exact in (False, True):
        got, n_inst, amb = _run(m, exact_ties=exact)
        assert np.array_equal(got, ref) and amb == 0 and n_inst == n == int(ref.max()), (pad, exact, n_inst, amb)


@pytest.mark.parametrize("tissue,ds", [("Gland", 1.0), ("Gland", 0.5), ("Lumen", 1.0), ("Lumen", 0.5)])
def test_gland_lumen_min_size_padding_overlap_and_holes(tissue, ds):
    """Components of min_size - 1 and min_size; a box pad - 1, pad and pad + 1 pixels from every border (the padding is one-sided: the crop grows
    only where the whole pad fits); two instances whose dilations overlap (the later id wins); a ring with a slit that the dilation closes (the
    inside is then a hole and filled) beside one it leaves open."""
    pad = P.gl_params(tissue, ds)[3]
    m, n, _ = P.gl_area_map(tissue, ds)
    cases = [("area", m, n)] + [("border %d" % d, P.gl_border_map(tissue, ds, d), 1) for d in (pad - 1, pad, pad + 1)]
    for tag, mm, n_want in cases:
        ref = pr.proc(mm, tissue, ds).astype(np.int32)
        for canvas in (False, True):
            got, n_inst, _ = _run(mm, tissue, ds, canvas=canvas)
            bad = np.argwhere(got != ref)
            assert len(bad) == 0 and n_inst == n_want == int(ref.max()), (tissue, ds, tag, canvas, len(bad), bad[:5].tolist(), n_inst)


# ---- (g) tiny maps ----------------------------------------------------------------------------------------------------------------------------------------
def test_tiny_maps():
    """Every H x W in 1..9 x 1..9 and four thin ones: W = 4 (one quad per row), H = 1, W % 4 == 0 with H < 3, a single column."""
    wrong = []
    for h, w in P.TINY_SIZES:
        m = P.tiny_map(h, w)
        for tissue in ("Nuclei", "Gland", "Lumen"):
            ref = pr.proc(m, tissue, 1.0).astype(np.int32)
            got, _, _ = _run(m, tissue, 1.0)
            if got.shape != ref.shape or not np.array_equal(got, ref):
                wrong.append((h, w, tissue, int((got != ref).sum())))
    assert not wrong, wrong
