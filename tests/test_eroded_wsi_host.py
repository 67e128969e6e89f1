"""Whole-slide runs of IP-ERODED-3 / -11 models (two-class INST heads, one canvas channel) without a GPU: the band / halo / ownership protocol of
cerberus_amd/shard_postproc.py on one-channel maps with numpy stand-ins for the kernels (label_fn = tests/eroded_ref.py::proc, the table and relabel
stand-ins of tests/test_host_logic.py), the guard relation, the overlap precedence across a cut, and what the opt-in interface still refuses."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import eroded_ref
from conftest import ROOT
from oracle import synth
from test_host_logic import _np_table

# (tissue, H, W, seed, margin, guard) -- tests/test_eroded_wsi_gpu.py runs the same maps and cuts through the kernels.  The seeds are those for which
# the stand-in run is exact with nothing truncated AND at least 3 instances cross a cut (seeds 1.. were tried in order; most gland seeds put a
# 300-px gland within 192 rows of a cut, which the protocol reports as n_truncated > 0).  The gland map is taken as an already-half-resolution map.
BAND_CASES = [("Nuclei", 384, 320, 1, 64, 16), ("Gland", 768, 512, 29, 192, 24)]


NESTED_CASE = ("Nuclei", 768, 320, 1, 64, 16)  # two outer bands whose windows are cut into inner bands (bounded_label_fn)


def band_case_map(tissue, H, W, seed):
    m = synth.nuclei_maps(H, W, seed, 1500.0, noise=0.02) if tissue == "Nuclei" else synth.gland_maps(H, W, seed, noise=0.02)
    return np.ascontiguousarray(m[..., :1])  # channel 0, as a (H, W, 1) canvas


def band_cuts(H, n=3):
    return [i * H // n for i in range(n + 1)]


def crossing_instances(whole, cuts):
    got = set()
    for e in cuts[1:-1]:
        got |= (set(np.unique(whole[e - 1]).tolist()) & set(np.unique(whole[e]).tolist())) - {0}
    return got


def np_label_fn(window, tissue, ds):
    """tests/eroded_ref.py::proc as the protocol's label_fn: `ds` is not used -- the eroded scheme has no ds_factor"""
    lab = eroded_ref.proc(np.asarray(window), tissue).astype(np.int32)
    return lab, int(lab.max())


def np_relabel_fn(rows, mapping):
    return np.asarray(mapping)[np.asarray(rows)]


def run_bands_np(m, tissue, cuts, margin, guard):
    from cerberus_amd import shard_postproc as sp

    bands = [torch.from_numpy(m[cuts[i]:cuts[i + 1]]) for i in range(len(cuts) - 1)]
    outs, n, infos = sp.run_local(bands, tissue, margin, guard, 1.0, label_fn=np_label_fn, table_fn=_np_table, relabel_fn=np_relabel_fn)
    return np.concatenate([np.asarray(o) for o in outs], axis=0), n, infos


@pytest.mark.parametrize("tissue,H,W,seed,margin,guard", BAND_CASES)
def test_band_protocol_on_one_channel_maps_equals_the_whole_map(tissue, H, W, seed, margin, guard):
    from cerberus_amd.shard_postproc import same_partition

    m = band_case_map(tissue, H, W, seed)
    whole = eroded_ref.proc(m, tissue).astype(np.int32)
    cuts = band_cuts(H)
    lab, n, infos = run_bands_np(m, tissue, cuts, margin, guard)
    assert lab.shape == whole.shape and same_partition(whole, lab)
    assert sum(i["n_truncated"] for i in infos) == 0 and sum(i["n_unresolved"] for i in infos) == 0, infos
    assert n == len(np.unique(whole)) - 1 and sorted(np.unique(lab)[1:].tolist()) == list(range(1, n + 1))  # ids unique and dense
    assert len(crossing_instances(whole, cuts)) >= 3, "the case needs instances that cross a cut"


def test_one_channel_band_names_the_guard_it_needs():
    from cerberus_amd.shard_postproc import BandState

    band = torch.zeros((256, 64, 1))
    with pytest.raises(ValueError, match=r"\b23\b.*\b22\b"):
        BandState(1, 3, band, 256, 96, 22, "Gland")
    BandState(1, 3, band, 256, 96, 23, "Gland")
    for t in ("Lumen", "Nuclei"):
        with pytest.raises(ValueError, match=r"\b7\b.*\b6\b"):
            BandState(1, 3, band, 256, 96, 6, t)
        BandState(1, 3, band, 256, 96, 7, t)
    BandState(1, 3, torch.zeros((256, 64, 2)), 256, 96, 0, "Gland")  # the contour scheme's bands take any guard, as before
    with pytest.raises(AssertionError):
        BandState(1, 3, torch.zeros((256, 64, 3)), 256, 96, 48, "Gland")


def test_overlap_precedence_across_a_cut():
    """Two lumen cores one above the other, their facing rows 2 px apart (one empty row between them) and a cut through that row's lower neighbour:
    both 3 x 3 dilations claim pixels of the row between, and the later id -- the lower core -- gets them on the whole map and in the bands alike."""
    from cerberus_amd.shard_postproc import same_partition
    from oracle import postproc_ref as pr

    m = np.zeros((64, 48, 1), np.float32)
    m[22:30, 10:30] = 0.9   # core A: rows 22..29, 160 px (min_size 150)
    m[31:39, 14:34] = 0.9   # core B: rows 31..38; row 30 is the gap
    whole = eroded_ref.proc(m, "Lumen").astype(np.int32)
    assert whole.max() == 2
    da = pr.dilate_ellipse((m[..., 0] > 0.5).astype(np.uint8) * (np.arange(64)[:, None] < 30), 3) > 0
    db = pr.dilate_ellipse((m[..., 0] > 0.5).astype(np.uint8) * (np.arange(64)[:, None] > 30), 3) > 0
    both = da & db
    assert both.sum() >= 10 and (whole[both] == 2).all() and (whole[da & ~db] == 1).all()  # contested pixels exist; the later id has them
    cuts = [0, 31, 64]
    lab, n, infos = run_bands_np(m, "Lumen", cuts, 20, 7)
    assert n == 2 and all(i["n_truncated"] == 0 and i["n_unresolved"] == 0 for i in infos), infos
    assert same_partition(whole, lab)
    a_id, b_id = int(lab[25, 15]), int(lab[35, 20])
    assert a_id != b_id and np.array_equal(lab == a_id, whole == 1) and np.array_equal(lab == b_id, whole == 2)  # pixel for pixel, contested ones included
    assert (lab[both] == b_id).all()


def test_runner_default_still_refuses_and_the_option_is_off():
    from cerberus_amd import wsi

    net = types.SimpleNamespace(_decoders=[("Gland", "INST", 3, "Gland-INST"), ("Nuclei", "INST", 2, "Nuclei-INST")])
    with pytest.raises(NotImplementedError, match="Nuclei-INST.*IP-ERODED-3"):
        wsi.WSIRunner(net, (512, 512))
    p = inspect.signature(wsi.WSIRunner.__init__).parameters["eroded_maps"]
    assert p.default is False


def test_reference_tiling_with_eroded_nuclei_is_refused_by_name():
    from cerberus_amd.wsi import check_eroded_slide_options

    mixed = {"Gland-INST": "IP-ERODED-CONTOUR-11", "Lumen-INST": "IP-ERODED-3", "Nuclei-INST": "IP-ERODED-3"}
    with pytest.raises(ValueError, match="--reference_tiling.*Nuclei-INST"):
        check_eroded_slide_options(decoder_dict=mixed, reference_tiling=True)
    check_eroded_slide_options(decoder_dict=mixed, reference_tiling=False)
    check_eroded_slide_options(decoder_dict=dict(mixed, **{"Nuclei-INST": "IP-ERODED-CONTOUR-3"}), reference_tiling=True)  # eroded gland / lumen only: fine
    net = types.SimpleNamespace(_decoders=[("Gland", "INST", 3, "Gland-INST"), ("Nuclei", "INST", 2, "Nuclei-INST")])
    with pytest.raises(ValueError, match="--reference_tiling"):
        check_eroded_slide_options(net=net, reference_tiling=True)


def test_streaming_refuses_two_class_heads_in_the_plan():
    """Sub-band streaming is not built for one-channel canvases: plan_slide says so by name where a three-class model would be streamed."""
    from cerberus_amd.stream_bands import plan_slide

    three = types.SimpleNamespace(_decoders=[("Gland", "INST", 3, "Gland-INST"), ("Nuclei", "INST", 3, "Nuclei-INST")])
    two = types.SimpleNamespace(_decoders=[("Gland", "INST", 3, "Gland-INST"), ("Nuclei", "INST", 2, "Nuclei-INST")])
    kw = dict(slide_hw=(40000, 40000), win=256, out=256, batch=8, budget=int(120e9))
    assert plan_slide(three, **kw).mode == "streamed"
    with pytest.raises(ValueError, match="IP-ERODED-3.*not streamed"):
        plan_slide(two, **kw)
    assert plan_slide(two, **dict(kw, budget=int(400e9))).mode == "resident"  # a band that fits is planned as ever


def test_nuclei_call_size_is_lowered_for_one_channel_maps():
    from cerberus_amd.shard_postproc import eroded_max_band_px

    assert eroded_max_band_px(400_000_000, "Nuclei", 1, 40000, 512) == 100_000_000
    assert eroded_max_band_px(400_000_000, "Nuclei", 2, 40000, 512) == 400_000_000 and eroded_max_band_px(400_000_000, "Gland", 1, 20000, 256) == 400_000_000
    assert eroded_max_band_px(None, "Nuclei", 1, 40000, 512) is None
    # a map too wide for bands of a quarter call keeps the full call size (a slide is not refused after its inference for being wide)
    assert eroded_max_band_px(400_000_000, "Nuclei", 1, 48828, 512) == 100_000_000 and eroded_max_band_px(400_000_000, "Nuclei", 1, 48829, 512) == 400_000_000


def test_a_ranks_window_is_labelled_in_nested_bands_under_the_call_bound():
    """The multi-rank path has no max_band_px: a rank's one-channel nuclei window above the call bound is labelled by bounded_label_fn, the same protocol
    nested.  Two outer bands of a 768 x 320 nuclei map (windows of 448 rows), a bound of 256 rows' worth of pixels per call that cuts every window into four inner
    bands of 112 rows with 64-row halos: the result is the whole map's, and the inner bands' counters travel into the outer n_truncated."""
    from cerberus_amd import shard_postproc as sp

    tissue, H, W, seed, margin, guard = NESTED_CASE
    m = band_case_map(tissue, H, W, seed)
    whole = eroded_ref.proc(m, tissue).astype(np.int32)
    calls = []

    def counting(window, t, ds):
        calls.append(int(window.shape[0]) * int(window.shape[1]))
        return np_label_fn(window, t, ds)

    bound = 4 * 320 * (128 + 2 * margin)  # a quarter of it = one inner band of 128 rows with its two halos
    assert sp.eroded_max_band_px(bound, tissue, 1, W, margin) == bound // 4 and sp.local_band_count(448, W, bound // 4, margin) == 4
    fl = sp.bounded_label_fn(counting, bound, margin, guard, _np_table, np_relabel_fn)
    bands = [torch.from_numpy(m[:384]), torch.from_numpy(m[384:])]
    outs, n, infos = sp.run_local(bands, tissue, margin, guard, 1.0, label_fn=fl, table_fn=_np_table, relabel_fn=np_relabel_fn)
    assert len(calls) == 8 and max(calls) <= bound // 4, calls
    lab = np.concatenate([np.asarray(o) for o in outs], axis=0)
    assert sp.same_partition(whole, lab) and n == len(np.unique(whole)) - 1
    assert all(i["n_truncated"] == 0 and i["n_unresolved"] == 0 for i in infos), infos
    # two-channel windows and other tissues pass straight through, whatever the bound
    assert sp.bounded_label_fn(lambda w_, t, d: ("x", 1), 10, margin, guard)(torch.zeros((300, 320, 2)), "Nuclei", 1.0) == ("x", 1)
    assert sp.bounded_label_fn(lambda w_, t, d: ("x", 1), 10, margin, guard)(torch.zeros((300, 320, 1)), "Gland", 1.0) == ("x", 1)
    # what a labelling reports as its third value lands in n_truncated
    st = sp.BandState(0, 1, torch.from_numpy(m[:192]), 0, margin, guard, tissue)
    st.label(None, None, lambda w_, t, d: np_label_fn(w_, t, d) + (3,), _np_table)
    assert st.n_truncated == 3


def test_nuclei_calls_are_checked_before_the_inference():
    from cerberus_amd.shard_postproc import check_eroded_nuclei_calls

    assert check_eroded_nuclei_calls(8000, 10000, 400_000_000, 512) == 1      # 80 Mpx: one call of at most 100 Mpx
    assert check_eroded_nuclei_calls(20000, 20000, 400_000_000, 512) == 6     # 400 Mpx, one GPU: bands of at most 100 Mpx with their halos
    assert check_eroded_nuclei_calls(20000, 40000, 400_000_000, 512, world=2) > 1  # a rank's 800-Mpx band + halos: nested bands
    assert check_eroded_nuclei_calls(20000, 60000, 400_000_000, 512, world=2) > 1  # too wide for quarter calls: the full call size
    with pytest.raises(ValueError, match="Nuclei-INST.*IP-ERODED-3.*cannot be labelled in row bands"):
        check_eroded_nuclei_calls(20000, 200000, 400_000_000, 512, world=2)


def test_new_exports_are_declared_and_bound_and_the_option_is_mirrored():
    from cerberus_amd import _lib
    from cerberus_amd.cli import WSI_ALL_OPTIONS, WSI_OPTIONS, parse

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cerberus_hip.h")).read(), flags=re.S)
    for name, n_args in (("cerb_downsample2_map", 8), ("cerb_downsample2_map_region", 13), ("cerb_downsample2_inst", 7), ("cerb_downsample2_inst_region", 12)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, txt, flags=re.S)
        assert m and m.group(1).count(",") + 1 == n_args, name
        assert name in _lib.EXPORTS and len(getattr(_lib.lib(), name).argtypes) == n_args, name
    assert WSI_ALL_OPTIONS[:len(WSI_OPTIONS)] == WSI_OPTIONS and [o[:3] for o in WSI_ALL_OPTIONS[len(WSI_OPTIONS):]] == [("--eroded_maps", False, False)]
    assert parse("run_infer_wsi.py", WSI_ALL_OPTIONS, ["--synthetic"])["--eroded_maps"] is False
    assert parse("run_infer_wsi.py", WSI_ALL_OPTIONS, ["--synthetic", "--eroded_maps"])["--eroded_maps"] is True
    src = open(os.path.join(ROOT, "run_infer_wsi.py")).read()
    assert src.index('args["--eroded_maps"]') < src.index("refuse_eroded_codes(decoders)") < src.index("manager = InferManager(")
