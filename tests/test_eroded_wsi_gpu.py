"""Whole-slide runs of IP-ERODED-3 / -11 models on the GPU (opt-in: WSIRunner(eroded_maps=True), run_infer_wsi.py --eroded_maps): the one-channel x0.5
resample against today's two-channel call, the band protocol with the real kernels on the maps and cuts of tests/test_eroded_wsi_host.py, the root-side
and per-region drivers, and the command line.  Every comparison is exact.  The test-side reference is tests/eroded_ref.py::proc."""
import ctypes as C
import json
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import torch

import eroded_ref
from conftest import ROOT
from oracle import synth
from test_eroded_wsi_host import BAND_CASES, NESTED_CASE, band_case_map, band_cuts, crossing_instances

pytestmark = pytest.mark.gpu


# ---- 1. the resample ------------------------------------------------------------------------------------------------------------
def _half(fn_name, src, h, w, n_ch=None, lab=None, rid=0):
    """one of the four C entry points on `src` (a CUDA float32 (h, w, C) tensor or a strided view of one) -> (ho, wo, n_ch or 2) CUDA tensor"""
    from cerberus_amd import _lib

    L = _lib.lib()
    ho, wo = L.cerb_half_size(h), L.cerb_half_size(w)
    out = torch.full((ho, wo, 2 if n_ch is None else n_ch), -5.0, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = [src.data_ptr(), src.stride(0), src.stride(1), h, w] + ([] if n_ch is None else [n_ch])
    if fn_name.endswith("_region"):
        a += [lab.data_ptr(), lab.stride(0), int(lab.shape[0]), int(lab.shape[1]), rid]
    _lib.check(getattr(L, fn_name)(*(a + [out.data_ptr(), st])))
    return out


@pytest.mark.parametrize("h,w", [(37, 51), (128, 96)])  # 37 -> 18 (the odd last row is dropped), 51 -> 26 (the odd last column is replicated); even sides
def test_one_channel_resample_is_bit_equal_to_plane_0_of_the_two_channel_call(h, w):
    from cerberus_amd.tissue import half_inst_region
    from cerberus_amd.wsi import downsample2_inst

    rs = np.random.RandomState(h)
    plane = torch.from_numpy(rs.rand(h, w).astype(np.float32)).cuda()
    two = torch.stack([plane, torch.from_numpy(rs.rand(h, w).astype(np.float32)).cuda()], -1).contiguous()
    one = plane[..., None].contiguous()
    lab = torch.from_numpy(rs.randint(1, 4, (19, 26)).astype(np.int32)).cuda()  # a label window of another size, three regions
    want = _half("cerb_downsample2_inst", two, h, w)
    want_r = _half("cerb_downsample2_inst_region", two, h, w, lab=lab, rid=2)
    assert not torch.equal(want, want_r) and float(want.min()) >= 0.0
    if h % 2 == 0 and w % 2 == 0:  # the arithmetic itself, restated (tests/test_drivers_gpu.py)
        m = plane.cpu().numpy()
        ds = (m[0::2, 0::2] * 0.5 + m[0::2, 1::2] * 0.5) * 0.5 + (m[1::2, 0::2] * 0.5 + m[1::2, 1::2] * 0.5) * 0.5
        assert np.array_equal(want[..., 0].cpu().numpy(), ds.astype(np.float32))
    got = _half("cerb_downsample2_map", one, h, w, n_ch=1)
    got_r = _half("cerb_downsample2_map_region", one, h, w, n_ch=1, lab=lab, rid=2)
    assert got.shape == want.shape[:2] + (1,)
    assert torch.equal(got[..., 0], want[..., 0]) and torch.equal(got_r[..., 0], want_r[..., 0])
    # n_ch = 2 through the new entries is today's call, both planes
    assert torch.equal(_half("cerb_downsample2_map", two, h, w, n_ch=2), want)
    assert torch.equal(_half("cerb_downsample2_map_region", two, h, w, n_ch=2, lab=lab, rid=2), want_r)
    # a strided source: the plane is channel 0 of a three-channel canvas (pix_stride 3), inside a wider canvas (row stride)
    canvas = torch.full((h + 3, w + 5, 3), 0.77, dtype=torch.float32, device="cuda")
    view = canvas[1:1 + h, 2:2 + w, 0:1]
    view.copy_(one)
    assert view.stride(1) == 3 and view.stride(0) == 3 * (w + 5)
    assert torch.equal(_half("cerb_downsample2_map", view, h, w, n_ch=1), got)
    assert torch.equal(_half("cerb_downsample2_map_region", view, h, w, n_ch=1, lab=lab, rid=2), got_r)
    # the Python entry points take (h, w, 1) maps and return (h/2, w/2, 1)
    assert torch.equal(downsample2_inst(one), got) and torch.equal(downsample2_inst(view), got) and torch.equal(downsample2_inst(two), want)
    assert torch.equal(half_inst_region(view), got) and torch.equal(half_inst_region(one, lab, 2), got_r) and torch.equal(half_inst_region(two, lab, 2), want_r)
    # bad channel counts are refused by name
    from cerberus_amd import _lib

    with pytest.raises(_lib.CerberusHipError, match="n_ch"):
        _half("cerb_downsample2_map", two, h, w, n_ch=3)


# ---- 2. the band protocol with the real kernels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("tissue,H,W,seed,margin,guard", BAND_CASES)
def test_band_protocol_on_the_device_equals_one_call_on_the_whole_map(tissue, H, W, seed, margin, guard):
    from cerberus_amd.postproc import postproc_eroded_device
    from cerberus_amd.shard_postproc import assemble, run_local, same_partition

    m = torch.from_numpy(band_case_map(tissue, H, W, seed)).cuda()
    whole, info = postproc_eroded_device(m, tissue)
    whole = whole.cpu().numpy()
    cuts = band_cuts(H)
    outs, n, infos = run_local([m[cuts[i]:cuts[i + 1]] for i in range(3)], tissue, margin, guard, 0.5 if tissue != "Nuclei" else 1.0)
    lab = assemble(outs).cpu().numpy()
    print(tissue, "instances", n, infos)
    assert same_partition(whole, lab)
    assert sum(i["n_truncated"] for i in infos) == 0 and sum(i["n_unresolved"] for i in infos) == 0, infos
    assert n == int(info["n_inst"].item()) == len(np.unique(whole)) - 1
    assert len(crossing_instances(whole, cuts)) >= 3


# ---- 3. the root-side driver ---------------------------------------------------------------------------------------------------------
def test_runner_postprocess_dispatches_on_the_channel_count():
    from cerberus_amd.tissue import half_inst_region
    from cerberus_amd.wsi import WSIRunner

    gland = torch.from_numpy(band_case_map("Gland", 768, 512, 29)).cuda()
    lumen = torch.from_numpy(np.ascontiguousarray(synth.blob_maps(768, 512, 7, 30, 14.0, 30.0, noise=0.02)[..., :1])).cuda()
    nuclei = torch.from_numpy(band_case_map("Nuclei", 384, 320, 1)).cuda()
    inst, info = WSIRunner.postprocess(OrderedDict([("Nuclei-INST", nuclei), ("Gland-INST", gland), ("Lumen-INST", lumen)]), wsi_mode=True)
    hg, hl = half_inst_region(gland), half_inst_region(lumen)
    assert hg.shape == (384, 256, 1)
    want_g = eroded_ref.proc(hg.cpu().numpy(), "Gland").astype(np.int32)  # full-resolution parameters on the half-resolution map: no ds_factor
    want_l = eroded_ref.proc(hl.cpu().numpy(), "Lumen").astype(np.int32)
    assert want_g.max() >= 2 and want_l.max() >= 5 and (want_l * (want_g > 0)).max() > 0 and ((want_l > 0) & (want_g == 0)).any()
    assert np.array_equal(inst["Gland"].cpu().numpy(), want_g)
    assert np.array_equal(inst["Lumen"].cpu().numpy(), want_l * (want_g > 0))  # lumen *= gland > 0 (infer/wsi.py:799-804)
    assert np.array_equal(inst["Nuclei"].cpu().numpy(), eroded_ref.proc(nuclei.cpu().numpy(), "Nuclei").astype(np.int32))
    # tile-mode semantics: full resolution
    inst_t, _ = WSIRunner.postprocess(OrderedDict([("Gland-INST", gland)]), wsi_mode=False)
    assert np.array_equal(inst_t["Gland"].cpu().numpy(), eroded_ref.proc(gland.cpu().numpy(), "Gland").astype(np.int32))


# ---- 4. / 5. a mixed model end to end ------------------------------------------------------------------------------------------------
H, W, PATCH = 384, 288, 96


def _count(info):
    return {t: len(info.get(t, {})) for t in ("Nuclei", "Gland", "Lumen")}


@pytest.fixture(scope="module")
def mixed():
    """The mixed model of tests/test_eroded_gpu.py (Gland IP-ERODED-CONTOUR-11, Lumen / Nuclei IP-ERODED-3) with sparse-foreground biases, a 384 x 288
    slide of stain-field tiles, and the slide run once through WSIRunner(eroded_maps=True)."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    from model_dir import stain_atlas
    from test_eroded_gpu import CODES, _sparse_mixed_state_dict

    from cerberus_amd.tile import InferManager
    from cerberus_amd.wsi import WSIRunner

    atlas = stain_atlas(12, tile=PATCH)
    slide = np.concatenate([np.concatenate(atlas[r * 3:r * 3 + 3], axis=1) for r in range(4)], axis=0)
    assert slide.shape == (H, W, 3)
    kw, sd = _sparse_mixed_state_dict([slide])
    mgr = InferManager(checkpoint_path=None, decoder_dict=dict(CODES), model_args=kw)
    mgr.net.load_state_dict(sd, strict=True)
    run = WSIRunner(mgr.net, (H, W), PATCH, PATCH, batch_size=5, eroded_maps=True)
    run.infer_band(torch.from_numpy(slide).cuda(), 0)
    return {"mgr": mgr, "kw": kw, "sd": sd, "codes": CODES, "slide": slide, "run": run, "maps": run.gather_to_root()}


def test_slide_runner_on_a_mixed_model_end_to_end(mixed):
    from cerberus_amd.shard_postproc import assemble, run_local, same_partition
    from cerberus_amd.wsi import WSIRunner, build_wsi_inst_info, downsample2_inst

    run, maps = mixed["run"], mixed["maps"]
    assert run.canv["Nuclei-INST"].shape == (H, W, 1) and run.canv["Lumen-INST"].shape == (H, W, 1) and run.canv["Gland-INST"].shape == (H, W, 2)
    # the canvases are the tile driver's, bit for bit (same kernels, same patches, same channel layout)
    res = mixed["mgr"].infer_image(mixed["slide"], PATCH, PATCH, batch_size=4)
    for k, v in maps.items():
        assert torch.equal(v, res["raw"][k]), k
    rep = run.logit_report()  # the logit guard indexes heads, not channels
    assert rep["batches"] == 3 and set(rep["per_head_max"]) >= {"Lumen-INST", "Gland-INST", "Nuclei-INST"} and rep["max"] > 0
    inst, info = WSIRunner.postprocess(maps, wsi_mode=True)
    half_l = downsample2_inst(maps["Lumen-INST"])
    want_l = eroded_ref.proc(half_l.cpu().numpy(), "Lumen").astype(np.int32) * (inst["Gland"].cpu().numpy() > 0)
    assert np.array_equal(inst["Lumen"].cpu().numpy(), want_l)
    assert np.array_equal(inst["Nuclei"].cpu().numpy(), eroded_ref.proc(maps["Nuclei-INST"].cpu().numpy(), "Nuclei").astype(np.int32))
    counts = _count(build_wsi_inst_info(inst, maps, (H, W), 0.5))
    print("instances:", counts)
    assert counts["Nuclei"] > 3, "the end-to-end test needs nuclei to compare"
    # two ranks, simulated: each tissue's map in two bands through the ownership / id / relabel steps against the one-band result.  margin = the band
    # height, so each window IS the whole map: this checks ownership by first pixel, the published ids and the relabelling on the mixed model's own
    # canvases (one- and two-channel, half resolution), NOT a cut window -- the random-weight model's blobs are as tall as a band, and any real halo
    # would only be reported as n_truncated.  Cut windows with real halos are test_band_protocol_on_the_device_equals_one_call_on_the_whole_map.
    for t in ("Nuclei", "Gland", "Lumen"):
        half = t != "Nuclei"
        band = downsample2_inst(maps[t + "-INST"]) if half else maps[t + "-INST"]
        rows = int(band.shape[0]) // 2
        m, g, ds = (rows, 24, 0.5) if half else (rows, 48, 1.0)
        one, n1, _ = run_local([band], t, m, g, ds)
        two, n2, infos = run_local([band[:rows], band[rows:]], t, m, g, ds)
        assert n1 == n2 and all(i["n_unresolved"] == 0 for i in infos), (t, n1, n2, infos)
        assert same_partition(one[0].cpu().numpy(), assemble(two).cpu().numpy()), t


def test_command_line_with_eroded_maps(mixed, tmp_path):
    import joblib
    import yaml
    from PIL import Image

    from cerberus_amd.tissue import TissueRegions, load_mask, postprocess_regions, select_patches
    from cerberus_amd.wsi import SlideGeometry, WSIRunner, build_wsi_inst_info, label_inst_map

    maps = mixed["maps"]
    inst, _ = WSIRunner.postprocess(maps, wsi_mode=True)
    want = _count(build_wsi_inst_info(inst, maps, (H, W), 0.5))
    inp, model, msk = tmp_path / "in", tmp_path / "model", tmp_path / "masks"
    for d in (inp, model, msk):
        d.mkdir()
    np.save(str(inp / "s1.npy"), mixed["slide"])
    torch.save({"desc": mixed["sd"]}, str(model / "weights.tar"))
    with open(str(model / "settings.yml"), "w") as fh:
        yaml.safe_dump(json.loads(json.dumps({"dataset_kwargs": {"req_target_code": mixed["codes"]}, "model_kwargs": mixed["kw"]})), fh, sort_keys=False)
    base = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--model=%s" % model, "--input_dir=%s" % inp, "--wsi_file_ext=.npy", "--batch_size=4",
            "--patch_input_shape=%d" % PATCH, "--patch_output_shape=%d" % PATCH]
    r = subprocess.run(base + ["--eroded_maps", "--output_dir=%s" % (tmp_path / "out")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    dat = joblib.load(str(tmp_path / "out" / "dat" / "s1.dat"))
    assert _count(dat) == want, (_count(dat), want)
    # ---- with a tissue mask of two regions: against tissue.postprocess_regions called directly on the canvases of a run with the same patch selection
    m = np.zeros((H // 8, W // 8), np.uint8)
    m[2:20, 2:30] = 255
    m[28:46, 4:34] = 255
    Image.fromarray(np.stack([m] * 3, -1)).save(str(msk / "s1.png"))
    mask = load_mask(str(msk / "s1.png"))
    sel = select_patches(mask, SlideGeometry((H, W), PATCH, PATCH).out_boxes(), (H, W))
    run = WSIRunner(mixed["mgr"].net, (H, W), PATCH, PATCH, batch_size=4, patch_sel=sel, eroded_maps=True)
    run.infer_band(torch.from_numpy(mixed["slide"]).cuda(), 0)
    mmaps = run.gather_to_root()
    regions = TissueRegions(torch.from_numpy(mask).cuda())
    assert regions.n == 2
    records = postprocess_regions(mmaps, (H, W), regions)
    assert all(rec["inst"]["Lumen"].dim() == 2 and rec["inst"]["Gland"].dtype == torch.int32 for rec in records)
    nuc = {"Nuclei": label_inst_map(mmaps["Nuclei-INST"], "Nuclei", exact_ties=False)[0]}
    want_m = _count(build_wsi_inst_info(nuc, mmaps, (H, W), 0.5, region_records=records))
    r = subprocess.run(base + ["--eroded_maps", "--msk_dir=%s" % msk, "--output_dir=%s" % (tmp_path / "masked")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    dat_m = joblib.load(str(tmp_path / "masked" / "dat" / "s1.dat"))
    print("instances under the mask:", _count(dat_m))
    assert _count(dat_m) == want_m, (_count(dat_m), want_m)


def test_nested_bands_on_the_device_keep_a_ranks_calls_under_the_bound():
    """tests/test_eroded_wsi_host.py's nested case with the real kernels: two outer bands, every window labelled in four inner bands (bounded_label_fn, the
    multi-rank path's per-call bound); the result is one call's on the whole map."""
    from cerberus_amd import shard_postproc as sp
    from cerberus_amd.postproc import postproc_eroded_device

    tissue, Hh, Ww, seed, margin, guard = NESTED_CASE
    m = torch.from_numpy(band_case_map(tissue, Hh, Ww, seed)).cuda()
    whole = postproc_eroded_device(m, tissue)[0].cpu().numpy()
    calls = []

    def counting(window, t, ds):
        calls.append(int(window.shape[0]) * int(window.shape[1]))
        return sp._device_label_fn(window, t, ds)

    bound = 4 * Ww * (128 + 2 * margin)
    outs, n, infos = sp.run_local([m[:384], m[384:]], tissue, margin, guard, 1.0, label_fn=sp.bounded_label_fn(counting, bound, margin, guard))
    assert len(calls) == 8 and max(calls) <= bound // 4, calls
    assert sp.same_partition(whole, sp.assemble(outs).cpu().numpy()) and n == len(np.unique(whole)) - 1
    assert all(i["n_truncated"] == 0 and i["n_unresolved"] == 0 for i in infos), infos


def test_command_line_labels_one_channel_nuclei_in_bounded_calls(mixed, tmp_path):
    """run_infer_wsi.py --eroded_maps with CERB_ONE_CALL_MPX lowered under a 6144 x 288 slide: the driver takes the local-band path at the QUARTERED call
    size of one-channel nuclei maps (3 Mpx -> 750000 px: 4 bands) and says so in the slide's log; the dictionary's entry counts are those of the same
    labelling called directly on the canvases of an in-process run."""
    import glob
    import re

    import joblib
    import yaml

    from cerberus_amd.shard_postproc import sharded_postprocess
    from cerberus_amd.wsi import WSIRunner, build_wsi_inst_info

    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    from model_dir import stain_atlas

    Ht, atlas = 6144, stain_atlas(192, tile=PATCH)
    slide = np.concatenate([np.concatenate(atlas[r * 3:r * 3 + 3], axis=1) for r in range(Ht // PATCH)], axis=0)
    run = WSIRunner(mixed["mgr"].net, (Ht, W), PATCH, PATCH, batch_size=16, eroded_maps=True)
    run.infer_band(torch.from_numpy(slide).cuda(), 0)
    maps = run.gather_to_root()
    inst, info = sharded_postprocess(OrderedDict((k, v) for k, v in maps.items() if k.endswith("INST")), 0, 1, None, wsi_mode=True, max_band_px=3000000)
    assert info["Nuclei"]["local_bands"] == 4 and info["Gland"]["local_bands"] == 1 and info["Lumen"]["local_bands"] == 1, info
    want = _count(build_wsi_inst_info(inst, maps, (Ht, W), 0.5))
    inp, model = tmp_path / "in", tmp_path / "model"
    inp.mkdir()
    model.mkdir()
    np.save(str(inp / "s1.npy"), slide)
    torch.save({"desc": mixed["sd"]}, str(model / "weights.tar"))
    with open(str(model / "settings.yml"), "w") as fh:
        yaml.safe_dump(json.loads(json.dumps({"dataset_kwargs": {"req_target_code": mixed["codes"]}, "model_kwargs": mixed["kw"]})), fh, sort_keys=False)
    cmd = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--model=%s" % model, "--input_dir=%s" % inp, "--wsi_file_ext=.npy", "--batch_size=16",
           "--patch_input_shape=%d" % PATCH, "--patch_output_shape=%d" % PATCH, "--eroded_maps", "--output_dir=%s" % (tmp_path / "out"),
           "--logging_dir=%s" % (tmp_path / "log")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT, env=dict(os.environ, CERB_ONE_CALL_MPX="3"))
    assert r.returncode == 0, r.stderr[-3000:]
    log = open(glob.glob(str(tmp_path / "log" / "s1_*_std.log"))[0]).read()
    got = re.search(r"Nuclei \(one channel\) labelled in calls of at most (\d+) pixels: .*'local_bands': (\d+)", log)
    assert got and int(got.group(1)) == 750000 and int(got.group(2)) == 4, log[-2000:]
    dat = joblib.load(str(tmp_path / "out" / "dat" / "s1.dat"))
    print("instances:", _count(dat))
    assert _count(dat) == want and want["Nuclei"] > 3, (_count(dat), want)
