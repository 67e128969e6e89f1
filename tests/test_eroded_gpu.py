"""IP-ERODED-3 / -11 models on the GPU: two-class INST heads through inference and training, PostProcInstErodedMap on the device, the tile driver
and its command line.  Fixtures: tests/golden/pp_eroded.npz, net_eroded_mixed96.npz, net_eroded_g448.npz, train_eroded.npz (the reference itself,
tests/tools/gen_golden_eroded.py); where no stored map exists the reference is restated by tests/eroded_ref.py (held to it by the generator and by
tests/test_eroded_host.py)."""
import copy
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
from conftest import GOLDEN, ROOT
from oracle import net_ref, postproc_ref, synth

pytestmark = pytest.mark.gpu
PROB_TOL = 1e-4  # tests/test_net_gpu.py

PP = np.load(os.path.join(GOLDEN, "pp_eroded.npz"))
PP_NAMES = [str(x) for x in PP["names"]]
MIXED = [("Lumen", [("INST", 2)]), ("Gland", [("INST", 3)]), ("Nuclei", [("INST", 2)]), ("Nuclei#TYPE", [("TYPE", 7)]), ("Gland#TYPE", [("TYPE", 3)]),
         ("Patch-Class", [("OUT", 9)])]
CODES = OrderedDict([("Lumen-INST", "IP-ERODED-3"), ("Gland-INST", "IP-ERODED-CONTOUR-11"), ("Nuclei-INST", "IP-ERODED-3"), ("Nuclei-TYPE", "TP"),
                     ("Gland-TYPE", "TP"), ("Patch-Class", "PC")])


# ---- post-processing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", PP_NAMES)
def test_postproc_eroded_equals_the_reference_bit_for_bit(name):
    from cerberus_amd.postproc import postproc_eroded_device

    tissue, m, want = str(PP["tissue/" + name]), PP["in/" + name].astype(np.float32), PP["out/" + name]
    H, W = m.shape
    lab, info = postproc_eroded_device(torch.from_numpy(m).cuda(), tissue)
    got = lab.cpu().numpy()
    assert got.dtype == np.int32 and np.array_equal(got, want), (name, int((got != want).sum()))
    assert int(info["n_inst"].item()) == int(want.max())
    # a strided (H, W, 1) window of a larger canvas, read in place; its neighbours hold foreground that must not leak in
    canvas = torch.full((H + 5, W + 7, 3), 0.9, dtype=torch.float32, device="cuda")
    win = canvas[2:2 + H, 3:3 + W, 1:2]
    win.copy_(torch.from_numpy(m).cuda()[..., None])
    assert win.shape == (H, W, 1) and win.stride(1) == 3 and win.stride(0) == 3 * (W + 7)
    lab2, _ = postproc_eroded_device(win, tissue.upper())
    assert torch.equal(lab2, lab), name
    out = torch.full((H, W), -7, dtype=torch.int32, device="cuda")  # a caller's buffer with stale values; second run byte-equal to the first
    lab3, _ = postproc_eroded_device(torch.from_numpy(m).cuda(), tissue, out=out)
    assert lab3 is out and torch.equal(lab3, lab), name


def test_mirror_class_keeps_the_reference_protocol():
    from cerberus_amd.postproc import PostProcInstErodedMap

    for name, tissue in (("nuc_generic", "Nuclei"), ("gland_touching", "Gland"), ("lumen_generic", "Lumen")):
        m = PP["in/" + name].astype(np.float32)
        types_ = (np.arange(m.size).reshape(m.shape) % 5).astype(np.float32)
        raw = np.stack([types_, m], -1)  # the INST channel is looked up through idx_dict, wherever it sits
        inst, tmap = PostProcInstErodedMap.post_process(raw, {tissue + "-INST": [1, 2], tissue + "-TYPE": [0, 1]}, tissue, 0.5)  # scale: accepted, ignored
        assert isinstance(inst, np.ndarray) and inst.dtype == np.float64 and np.array_equal(inst, PP["out/" + name]), name
        assert tmap.shape == m.shape + (1,) and np.array_equal(tmap[..., 0], types_)  # NOT squeezed (loader/postproc.py:259-263)
        inst2, tmap2 = PostProcInstErodedMap.post_process(raw[..., 1:], {tissue + "-INST": [0, 1]}, tissue)
        assert tmap2 is None and np.array_equal(inst2, inst)
        dev_inst, _ = PostProcInstErodedMap.post_process(torch.from_numpy(raw).cuda(), {tissue + "-INST": [1, 2]}, tissue)
        assert dev_inst.is_cuda and dev_inst.dtype == torch.int32 and np.array_equal(dev_inst.cpu().numpy(), PP["out/" + name])


def test_instance_table_at_min_size_8_on_a_2048_map():
    """Thousands of nuclei in one call: the instance tables are sized n / min_size + 2 and the crops run in batches of what the workspace holds."""
    from cerberus_amd.postproc import postproc_eroded_device

    m = np.ascontiguousarray(synth.nuclei_maps(2048, 2048, 41, 1500.0, noise=0.02)[..., 0])
    want = eroded_ref.proc(m, "Nuclei")
    assert want.max() > 3000
    lab, info = postproc_eroded_device(torch.from_numpy(m).cuda(), "Nuclei")
    got = lab.cpu().numpy()
    assert int(info["n_inst"].item()) == int(want.max())
    assert np.array_equal(got, want.astype(np.int32)), int((got != want).sum())


# ---- network: inference --------------------------------------------------------------------------------------------------------
def _fixture_model(g):
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.weights import default_model_kwargs, make_state_dict, state_dict_sha256

    kw = default_model_kwargs([str(t) for t in g["tasks"]])
    kw["decoder_kwargs"] = OrderedDict((k, OrderedDict((a, b) for a, b in v)) for k, v in json.loads(str(g["decoder_kwargs_json"])))
    sd_np = make_state_dict(int(g["weight_seed"]), kw["decoder_kwargs"], kw["considered_tasks"])
    assert state_dict_sha256(sd_np) == str(g["weights_sha256"]), "the fixture's weights were not rebuilt bit for bit"
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    m = create_model(**kw)
    m.load_state_dict(sd, strict=True)
    tiles = np.random.RandomState(int(g["tile_seed"])).randint(0, 256, (int(g["n"]), int(g["hw"]), int(g["hw"]), 3)).astype(np.uint8)
    return m, sd, kw, tiles, [str(t) for t in g["head_name_list"]]


@pytest.fixture(scope="module", params=["eroded_mixed96", "eroded_g448"])
def net_case(request):
    g = np.load(os.path.join(GOLDEN, "net_%s.npz" % request.param))
    return (request.param, g) + _fixture_model(g)


@pytest.mark.parametrize("head_algo", [1, 2, 0])
def test_infer_step_vs_reference_golden(net_case, head_algo):
    """The bar of tests/test_net_gpu.py: |got - p64| <= noise/<head> + 1e-4 on the probabilities (p64: the reference's float64 evaluation, noise: its
    own float32-vs-float64 distance), TYPE maps differing on fewer than 1e-4 of the pixels; under the grouped launch on 4x4x1 matrix instructions
    (1, the default), the grouped launch on the zero-padded 16-row instruction (2) and one launch per head (0)."""
    from cerberus_amd.run_desc import infer_step

    tag, g, m, sd, kw, tiles, heads = net_case
    n, hw, osz = int(g["n"]), int(g["hw"]), int(g["out_shape"])
    och = {d[3]: d[2] for d in m._decoders}
    m.prepare()  # the load-time probe forward runs before the watch starts, as in tests/test_net_gpu.py: the words below are this batch's alone
    try:
        m.set_head_algo(head_algo)
        m.watch_logits()
        out = infer_step(torch.from_numpy(tiles), m, osz, heads)
        seen = m.logit_absmax()
    finally:
        m.set_head_algo(1)
        m.watch_logits(False)
    assert len(out) == n and set(out[0].keys()) == {k[len("out_dtype/"):] for k in g.files if k.startswith("out_dtype/")}
    for k in out[0]:
        a = np.stack([out[i][k] for i in range(n)])
        ref = g["out_full/" + k]
        assert str(a.dtype) == str(g["out_dtype/" + k]), k
        if k.endswith("INST"):
            assert a.shape == (n, osz, osz, och[k] - 1) == ref.shape, (k, a.shape, ref.shape)
            p64, noise = g["p64_full/" + k], float(g["noise/" + k])
            e64 = float(np.abs(a - p64).max())
            print("%s head_algo %d %s: |got - p64| %.3e (reference fp32: %.3e, noise %.3e)" % (tag, head_algo, k, e64, float(np.abs(ref - p64).max()), noise))
            assert e64 <= noise + PROB_TOL, (k, e64, noise)
        elif k.endswith("TYPE"):
            assert a.shape == (n, osz, osz)
            assert float((a != ref[..., 0]).mean()) < 1e-4, k
        else:
            assert np.array_equal(a, ref[..., 0]), k
    # the logit-guard words of the two-class heads: the largest |logit| of the batch (the kept window's when the forward is cropped)
    for k, v in seen.items():
        want = float(g["logit_absmax/" + k])
        assert (abs(v - want) if osz == hw else max(0.0, v - want)) <= 2e-3 * max(1.0, want), (k, v, want)
        assert v > 0.0, k


def test_logits_side_output_vs_oracle():
    """NetDesc.forward (the `logits` side output of the head kernels) against the oracle, which oracle/gen_golden_net.py held to the reference when the
    fixture was written; [N, out_ch, H, W] with out_ch 2 for the two-class heads.  (The 96^2 case: the oracle's CPU forward stays short.)"""
    g = np.load(os.path.join(GOLDEN, "net_eroded_mixed96.npz"))
    m, sd, kw, tiles, heads = _fixture_model(g)
    x = torch.from_numpy(tiles).float().permute(0, 3, 1, 2).contiguous()
    ref = net_ref.net_forward(sd, x, kw["decoder_kwargs"], kw["considered_tasks"])
    for algo in (1, 2, 0):
        try:
            m.set_head_algo(algo)
            out = m(torch.from_numpy(tiles))
        finally:
            m.set_head_algo(1)
        assert list(out.keys()) == list(ref.keys())
        for k, v in out.items():
            assert v.shape == ref[k].shape and (v.shape[1] == 2) == (k in ("Lumen-INST", "Nuclei-INST")), (k, v.shape)
            assert (v.cpu() - ref[k]).abs().max().item() < 2e-4, (k, algo)  # the bar of test_encoder_and_logits_vs_oracle


def test_three_class_head_is_not_disturbed_by_two_class_neighbours():
    """One grouped launch mixes 2- and 3-class INST heads: the Gland head's probabilities are byte-equal to what the same weights give in a model whose
    other INST heads have three classes too -- under every head algorithm."""
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    g = np.load(os.path.join(GOLDEN, "net_eroded_mixed96.npz"))
    m, sd, kw, tiles, heads = _fixture_model(g)
    kw3 = default_model_kwargs()
    sd3 = {k: torch.from_numpy(v) for k, v in make_state_dict(1).items()}
    same = [k for k in sd3 if tuple(sd3[k].shape) == tuple(sd[k].shape)]
    assert sorted(set(sd3) - set(same)) == sorted("output_head.%s.INST.x.1.conv.%s" % (d, p) for d in ("Lumen", "Nuclei") for p in ("weight", "bias"))
    for k in same:
        sd3[k] = sd[k]
    m3 = create_model(**kw3)
    m3.load_state_dict(sd3, strict=True)
    t = torch.from_numpy(tiles).cuda()
    for algo in (1, 2, 0):
        try:
            m.set_head_algo(algo)
            m3.set_head_algo(algo)
            a, b = m.infer_tiles(t, 96), m3.infer_tiles(t, 96)
            la, lb = m(t), m3(t)
        finally:
            m.set_head_algo(1)
            m3.set_head_algo(1)
        assert a["Lumen-INST"].shape == (2, 96, 96, 1) and a["Gland-INST"].shape == (2, 96, 96, 2) and b["Lumen-INST"].shape == (2, 96, 96, 2)
        for k in ("Gland-INST", "Gland-TYPE", "Nuclei-TYPE", "Patch-Class"):
            assert torch.equal(a[k], b[k]), (k, algo)
            assert torch.equal(la[k], lb[k]), (k, algo)


def test_roi_cropped_forward_is_the_centre_crop_of_the_full_one():
    """448 -> 144 with every INST head at two classes: head_kernel<true> / the grouped kernel on the 16-aligned cover of the window write one float per
    pixel; byte-equal to the uncropped computation (the invariant of test_crop_region_of_interest_is_bit_identical_to_the_full_computation)."""
    g = np.load(os.path.join(GOLDEN, "net_eroded_g448.npz"))
    m, sd, kw, tiles, heads = _fixture_model(g)
    t = torch.from_numpy(tiles).cuda()
    other = torch.from_numpy(np.random.RandomState(5).randint(0, 256, tiles.shape).astype(np.uint8)).cuda()
    for algo in (1, 0):
        try:
            m.set_head_algo(algo)
            m.set_crop_roi(False)
            full = {k: v.clone() for k, v in m.infer_tiles(t, 144).items()}
            whole = {k: v.clone() for k, v in m.infer_tiles(t, 448).items()}
            m.infer_tiles(other, 448)  # another image's activations in every workspace buffer
            m.set_crop_roi(True)
            roi = m.infer_tiles(t, 144)
        finally:
            m.set_crop_roi(True)
            m.set_head_algo(1)
        for k in full:
            assert torch.equal(full[k], roi[k]), (k, algo)
            if k != "Patch-Class":
                assert torch.equal(whole[k][:, 152:296, 152:296], roi[k]), (k, algo)
        assert roi["Nuclei-INST"].shape == (1, 144, 144, 1)


def test_net_create_still_refuses_other_inst_widths():
    from cerberus_amd import _lib

    L = _lib.lib()
    for och, ok in ((1, False), (2, True), (3, True), (4, False)):
        names, heads, ch = (C.c_char_p * 1)(b"Nuclei"), (C.c_char_p * 1)(b"INST"), (C.c_int * 1)(och)
        h = C.c_void_p()
        rc = L.cerb_net_create(names, heads, ch, 1, C.byref(h))
        if ok:
            assert rc == 0, L.cerb_last_error()
            L.cerb_net_destroy(h)
        else:
            assert rc != 0 and b"INST heads must have 2 or 3 channels" in L.cerb_last_error(), (och, L.cerb_last_error())


def test_ops_infer_tiles_shapes_follow_the_head():
    from cerberus_amd import ops  # noqa: F401  (registers torch.ops.cerberus_amd)
    from torch._subclasses.fake_tensor import FakeTensorMode

    g = np.load(os.path.join(GOLDEN, "net_eroded_mixed96.npz"))
    m, sd, kw, tiles, heads = _fixture_model(g)
    t = torch.from_numpy(tiles).cuda()
    got = torch.ops.cerberus_amd.infer_tiles(t, m.handle_value(), 96, 96, "Lumen-INST,Gland-INST")
    want = m.infer_tiles(t, 96)
    assert got[0].shape == (2, 96, 96, 1) and got[1].shape == (2, 96, 96, 2)
    assert torch.equal(got[0], want["Lumen-INST"]) and torch.equal(got[1], want["Gland-INST"])
    hv = m.handle_value()
    with FakeTensorMode():
        ft = torch.empty((2, 96, 96, 3), dtype=torch.uint8, device="cuda")
        fake = torch.ops.cerberus_amd.infer_tiles(ft, hv, 96, 96, "Lumen-INST,Gland-INST")
        assert [tuple(o.shape) for o in fake] == [(2, 96, 96, 1), (2, 96, 96, 2)]


# ---- network: training ---------------------------------------------------------------------------------------------------------
def test_train_step_on_the_mixed_model_vs_reference():
    """The reference's own train_step on the mixed model (train_eroded.npz), with the bars of tests/test_train_loss_gpu.py for the same quantities:
    losses 1e-4; d(loss)/d(logits) 2e-5 of the tensor's largest element (cerb_head_loss on the reference's logits); the full gradients of the two-class
    Nuclei head element by element against the reference's own inter-backend noise."""
    from cerberus_amd.losses import PARAMSET_LOSS, head_loss
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.train import Adam, train_step
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    g = np.load(os.path.join(GOLDEN, "train_eroded.npz"))
    kw = default_model_kwargs()
    kw["decoder_kwargs"] = OrderedDict((k, OrderedDict((a, b) for a, b in v)) for k, v in json.loads(str(g["decoder_kwargs_json"])))
    sd0 = {k: torch.from_numpy(v) for k, v in make_state_dict(int(g["weight_seed"]), kw["decoder_kwargs"], kw["considered_tasks"]).items()}
    N, H = int(g["N"]), int(g["H"])
    heads = [str(h) for h in g["heads"]]
    tiles = torch.from_numpy(g["img"]).cuda()
    keep = torch.from_numpy(g["dropout_mask"].reshape(N, 512)).cuda()
    targets, flags = {}, {}
    for j, h in enumerate(heads):
        t = g["target/" + h][..., 0].astype(np.float32)
        targets[h] = torch.from_numpy(t.reshape(N) if h == "Patch-Class" else t).cuda()
        flags[h] = torch.from_numpy(g["has_target"][:, j].astype(np.float32)).cuda()
    m = create_model(**kw)
    m.load_state_dict(sd0, strict=True)
    lo = {}
    losses, grads = m.train_grads(tiles, targets, flags, PARAMSET_LOSS, keep, logits_out=lo)
    assert lo["Lumen-INST"].shape == (N, H, H, 2) and lo["Gland-INST"].shape == (N, H, H, 3) and lo["Nuclei-INST"].shape == (N, H, H, 2)
    for h in heads:
        exp = float(g["loss/" + h])
        print("%-12s loss %.6f (reference %.6f)" % (h, losses[h], exp))
        assert abs(losses[h] - exp) <= 1e-4 * max(1.0, abs(exp)), (h, losses[h], exp)
    assert abs(sum(losses.values()) - float(g["overall_loss"])) <= 1e-4 * float(g["overall_loss"])
    # d(overall loss) / d(logits): cerb_head_loss on the logits the reference's network produced (our own train-mode logits for Nuclei-TYPE, whose
    # weight is 0 in paramset.yml: its gradient is zero whatever they are)
    for j, h in enumerate(heads):
        if "logits/" + h in g.files:
            lg, cl = torch.from_numpy(g["logits/" + h]).cuda(), False
        else:
            lg, cl = lo[h], True
        loss, dl = head_loss(h, lg, torch.from_numpy(g["target/" + h][..., 0].astype(np.float32)).cuda(), flags[h], copy.deepcopy(PARAMSET_LOSS), channels_last=cl)
        exp, ref = float(g["loss/" + h]), g["dlogits/" + h]
        got = dl.permute(0, 3, 1, 2).cpu().numpy() if cl else dl.cpu().numpy()
        assert abs(float(loss) - exp) <= 1e-4 * max(1.0, abs(exp)), (h, float(loss), exp)
        err = float(np.abs(got.reshape(ref.shape) - ref).max())
        assert err <= 2e-5 * max(1e-3, float(np.abs(ref).max())) + 1e-9, (h, err, float(np.abs(ref).max()))
    # full gradient tensors of the two-class head, per output channel relative to the tensor's largest element
    for k in [str(x) for x in g["grad_full_names"]]:
        ref = g["grad_full/" + k].astype(np.float64)
        got = grads[k].double().cpu().numpy().reshape(ref.shape)
        scale = max(float(np.abs(ref).max()), 1e-30)
        per_co = np.abs(got - ref).reshape(ref.shape[0], -1).max(axis=1) / scale
        p90, mx = float(np.percentile(per_co, 90)), float(per_co.max())
        cos = float((got * ref).sum() / (np.linalg.norm(got) * np.linalg.norm(ref)))
        bar = max(2e-3, 3.0 * float(g["grad_full_noise/" + k]))
        print("%-55s p90 %.2e max %.2e cos %.7f (bar %.1e)" % (k, p90, mx, cos, bar))
        assert p90 < bar and mx < 2e-2 and cos > 0.9999, (k, p90, bar, mx, cos)
    # the whole step in the reference's protocol (batch dict + run_info), then a second one on the re-packed weights
    has = np.full((N, len(heads)), None, dtype=object)
    for j, h in enumerate(heads):
        for n in range(N):
            if g["has_target"][n, j]:
                has[n, j] = h
    batch = {"img": torch.from_numpy(g["img"]), "dummy_target": has}
    for h in heads:
        batch[h] = torch.from_numpy(g["target/" + h].astype(np.float32))
    m2 = create_model(**kw)
    m2.load_state_dict(sd0, strict=True)
    opt = Adam(lr=1.0e-3, betas=(0.9, 0.999))
    res = train_step(batch, ({"net": {"desc": m2, "optimizer": opt, "extra_info": {"loss": PARAMSET_LOSS}}}, None), dropout_keep=keep)
    assert abs(res["EMA"]["overall_loss"] - float(g["overall_loss"])) <= 1e-4 * float(g["overall_loss"])
    assert res["raw"]["pred"]["Nuclei-INST"].shape == (2, H, H) and res["raw"]["pred"]["Gland-INST"].shape == (2, H, H, 2)  # torch.squeeze, as the reference
    res2 = train_step(batch, ({"net": {"desc": m2, "optimizer": opt, "extra_info": {"loss": PARAMSET_LOSS}}}, None), dropout_keep=keep)
    assert np.isfinite(res2["EMA"]["overall_loss"]) and res2["EMA"]["overall_loss"] != res["EMA"]["overall_loss"]
    new = m2.state_dict()
    k = "output_head.Nuclei.INST.x.1.conv.weight"
    assert tuple(new[k].shape) == (2, 96, 1, 1) and not torch.equal(new[k], sd0[k])


# ---- tile driver ----------------------------------------------------------------------------------------------------------------
def _mixed_kwargs():
    from cerberus_amd.weights import default_model_kwargs

    kw = default_model_kwargs()
    kw["decoder_kwargs"] = OrderedDict((k, OrderedDict(v)) for k, v in MIXED)
    return kw


def _driver_images():
    rs = np.random.RandomState(77)
    return [rs.randint(0, 256, (200, 180, 3)).astype(np.uint8), rs.randint(0, 256, (300, 260, 3)).astype(np.uint8)]


def _sparse_mixed_state_dict(imgs):
    """The seeded weights of the mixed model with every INST head's background bias raised until a share of the images' pixels stays foreground (as
    tests/tools/model_dir.py does for the default model): the plain recipe paints the whole of a noise image as one blob, which PostProcInstErodedMap
    returns as an empty map."""
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.weights import make_state_dict

    kw = _mixed_kwargs()
    sd = {k: torch.from_numpy(v) for k, v in make_state_dict(0, kw["decoder_kwargs"], kw["considered_tasks"]).items()}
    m = create_model(**kw)
    m.load_state_dict(sd, strict=True)
    tiles = torch.from_numpy(np.stack([im[:176, :176] for im in imgs])).cuda()
    lg = m(tiles)
    for name, q in (("Lumen", 0.2), ("Gland", 0.35), ("Nuclei", 0.3)):
        v = lg[name + "-INST"]
        rest = v[:, 0] if v.shape[1] == 2 else torch.logsumexp(torch.stack([v[:, 0], v[:, 2]]), 0)
        sd["output_head.%s.INST.x.1.conv.bias" % name][0] += float(torch.quantile((v[:, 1] - rest).flatten().float(), 1.0 - q))
    return kw, sd


def _check_driver_maps(raw, inst):
    """inst[...] against the restatement (the existing oracle, for the contour-code Gland) applied to the run's own downloaded canvases"""
    r = {k: v.cpu().numpy() for k, v in raw.items()}
    assert r["Lumen-INST"].shape[2] == 1 and r["Gland-INST"].shape[2] == 2 and r["Nuclei-INST"].shape[2] == 1
    gland = postproc_ref.proc(r["Gland-INST"], "Gland").astype(np.int32)
    lumen = eroded_ref.proc(r["Lumen-INST"], "Lumen").astype(np.int32) * (gland > 0)  # Lumen *= Gland > 0 (infer/tile.py:187-191)
    nuclei = eroded_ref.proc(r["Nuclei-INST"], "Nuclei").astype(np.int32)
    for t, want in (("Gland", gland), ("Lumen", lumen), ("Nuclei", nuclei)):
        got = np.asarray(inst[t])
        assert got.shape == want.shape and np.array_equal(got.astype(np.int32), want), (t, int((got != want).sum()))
    return gland, lumen, nuclei


def test_tile_driver_and_command_line_on_a_mixed_model(tmp_path):
    import scipy.io as sio
    import yaml
    from PIL import Image

    from cerberus_amd.tile import InferManager

    imgs = _driver_images()
    kw, sd = _sparse_mixed_state_dict(imgs)
    mgr = InferManager(checkpoint_path=None, decoder_dict=dict(CODES), model_args=kw)  # synthetic weights of the mixed model ...
    mgr.net.load_state_dict(sd, strict=True)                                           # ... with the sparse-foreground biases
    res = mgr.infer_images(imgs, 256, 256, batch_size=4)
    maps = []
    for im, r in zip(imgs, res):
        assert list(r["inst"].keys()) == ["Gland", "Lumen", "Nuclei"]
        maps.append(_check_driver_maps(r["raw"], {t: v.cpu().numpy() for t, v in r["inst"].items()}))
        assert r["inst"]["Gland"].shape == im.shape[:2] and r["type"]["Nuclei"].dtype == torch.uint8
    assert max(int(n.max()) for _, _, n in maps) > 3, "the driver test needs nuclei instances to compare"
    # a wrong pairing of code and head is said by name
    bad = InferManager(checkpoint_path=None, decoder_dict=dict(CODES, **{"Nuclei-INST": "IP-ERODED-CONTOUR-3"}), model_args=kw)
    with pytest.raises(ValueError, match="Nuclei-INST"):
        bad.infer_images(imgs[:1], 256, 256, batch_size=4)
    del bad
    # ---- the command line on the same two files and weights: <tissue>_mat/<name>.mat carry the same label maps
    inp, out, model = tmp_path / "in", tmp_path / "out", tmp_path / "model"
    inp.mkdir()
    model.mkdir()
    for name, im in zip(("a", "b"), imgs):
        Image.fromarray(im).save(str(inp / (name + ".png")))
    torch.save({"desc": sd}, str(model / "weights.tar"))
    with open(str(model / "settings.yml"), "w") as fh:
        yaml.safe_dump(json.loads(json.dumps({"dataset_kwargs": {"req_target_code": CODES}, "model_kwargs": kw})), fh, sort_keys=False)
    cmd = [sys.executable, os.path.join(ROOT, "run_infer_tile.py"), "--model=%s" % model, "--input_dir=%s" % inp, "--output_dir=%s" % out, "--batch_size=4",
           "--patch_input_shape=256", "--patch_output_shape=256"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    for name, (gland, lumen, nuclei) in zip(("a", "b"), maps):
        for t, want in (("gland", gland), ("lumen", lumen), ("nuclei", nuclei)):
            mat = sio.loadmat(str(out / ("%s_mat" % t) / (name + ".mat")))
            assert set(mat.keys()) >= {"inst_map", "type", "id"}
            assert np.array_equal(mat["inst_map"].astype(np.int32), want), (name, t)
