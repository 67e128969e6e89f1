"""The encoder's residual stages in the tile-planar layout (cerb_api.hip: encoder_stage_is_planar): their stride-1 3x3 convolutions on conv_wino4p.hip -- the
second one of a block with the block's identity as a tile-planar residual, written in place -- fed by planar stores of the max-pool and of the stride-2
convolutions, and handed back to NHWC by one planar_to_nhwc pass per stage.  conv_wino4p accumulates a position's input channels in the same ascending groups
of four as conv_wino4b / conv_wino4, shares their transforms and adds the residual where wino4_store_block does (after the output transform, before the ReLU
floor), so everything must give the bits of the NHWC path: torch.equal on every head output and on the `logits` side outputs, default against
cerb_net_set_planar(0), also after a forward of another batch size has left other values in every planar buffer.

Shapes: the smallest at which each path can go wrong -- an odd number of blocks (the last pair of an item repeats one), one block per image, a stage that
exits into an NHWC F(2x2) stage, maps that are no multiple of 16 right behind a planar stage (24^2, 56^2: the latter stays on conv_wino4b's packed items),
8 x 32 and 16 x 16 tiles of the stride-2 convolutions, a tile that hangs over the map (48 columns)."""
import ctypes as C
from collections import OrderedDict

import numpy as np
import pytest
import torch

import dev_kernels as D
from conftest import dev_switches
from dev_kernels import _check_planar, _to_planar

pytestmark = pytest.mark.gpu

ENC_STAGES = 0x7  # the stages that ship tile-planar where their geometry allows it (cerb_api.hip: kEncPlanarStages), bit li = backbone.layer<li + 1>
LAYERS = (3, 4, 6, 3)
ENC = "conv_wino4_enc<"
_model_cache = []


def _model():
    if not _model_cache:
        from cerberus_amd.net_desc import create_model
        from cerberus_amd.weights import default_model_kwargs, make_state_dict

        kw = default_model_kwargs()
        sd = {k: torch.from_numpy(v) for k, v in make_state_dict(11, kw["decoder_kwargs"], kw["considered_tasks"]).items()}
        m = create_model(**kw)
        m.load_state_dict(sd, strict=True)
        m.prepare()
        _model_cache.append(m)
    return _model_cache[0]


def _tiles(n, hw, seed):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (n, hw, hw, 3)).astype(np.uint8)).cuda()


def _all_outputs(m, t, hw):
    out = OrderedDict(("out/" + k, v.clone()) for k, v in m.infer_tiles(t, hw).items())
    out.update(("logits/" + k, v.clone()) for k, v in m(t).items())
    torch.cuda.synchronize()
    return out


def _same(got, ref, what):
    assert list(got.keys()) == list(ref.keys()) and len(ref) >= 2, what
    for k in ref:
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, (what, k)
        assert torch.equal(a, b), (what, k, int((a != b).sum()))


def _check(n, hw, seed, between, planar_stages, mask=ENC_STAGES):
    """default against cerb_net_set_planar(0); a forward of `between` tiles runs before the comparison is repeated.  planar_stages: the stages whose
    geometry allows the planar path at this tile size; returns the profile families of the planar run."""
    m = _model()
    t = _tiles(n, hw, seed)
    try:
        m.set_planar(False)
        m.profile(True)
        ref = _all_outputs(m, t, hw)
        kern_nhwc = [r[1] for r in m.profile_records()]
        m.profile(False)
        m.set_planar(True)
        m.profile(True)
        got = _all_outputs(m, t, hw)
        kern = [r[1] for r in m.profile_records()]
        m.profile(False)
        _same(got, ref, "first run")
        m.infer_tiles(_tiles(between, hw, seed + 1), hw)  # other values, another batch size, in every planar buffer
        _same(_all_outputs(m, t, hw), ref, "after a batch of %d" % between)
    finally:
        m.profile(False)
        m.set_planar(True)
    assert any(v.dtype == torch.float32 and 0.0 < float(v.abs().mean()) for v in ref.values()), "the comparison needs non-trivial maps"
    assert not any(k.startswith(ENC) or k in ("planar_to_nhwc", "maxpool3x3s2_planar") or k.startswith("conv_igemm_planar") for k in kern_nhwc), kern_nhwc
    on = [li for li in planar_stages if (mask >> li) & 1]
    assert sum(k.startswith(ENC) for k in kern) == sum(2 * LAYERS[li] - (1 if li else 0) for li in on), kern
    assert sum(k.startswith(ENC) and k.endswith(",res>") for k in kern) == sum(LAYERS[li] for li in on), kern
    assert kern.count("planar_to_nhwc") == len(on) and kern.count("maxpool3x3s2_planar") == (1 if 0 in on else 0), kern
    assert sum(k.startswith("conv_igemm_planar") for k in kern) == 2 * sum(1 for li in on if li), kern
    return kern


def test_odd_block_count_and_an_exit_into_an_nhwc_stage():
    """tile 64, N = 3: 32^2 and 16^2 run planar (three blocks at 16^2: the last pair repeats one), the 8^2 stage stays F(2x2) on NHWC."""
    kern = _check(3, 64, 31, 1, (0, 1))
    assert any(k.startswith("conv_wino<f2x2") for k in kern), kern


def test_three_planar_stages():
    """tile 128, N = 2: 64^2, 32^2, 16^2."""
    _check(2, 128, 32, 3, (0, 1, 2))


def test_every_shipped_stage_at_the_headline_tile_size():
    """tile 256, N = 1: 128^2 x 64, 64^2 x 128, 32^2 x 256 run planar; the product leaves 16^2 x 512 on conv_wino4b (it lost its A/B: ENC_STAGES)."""
    _check(1, 256, 33, 2, (0, 1, 2, 3))


@dev_switches
def test_all_four_stages_one_block_per_image_at_the_last():
    """tile 256, N = 1, with the developers' stage mask opening the last stage as well: 16^2 x 512, one block per image."""
    import os

    os.environ["CERB_ENC_PLANAR"] = "15"
    try:
        _check(1, 256, 33, 2, (0, 1, 2, 3), mask=15)
    finally:
        del os.environ["CERB_ENC_PLANAR"]


def test_odd_block_count_and_packed_items_behind_a_planar_stage():
    """tile 224, N = 1: 112^2 has 49 blocks; 56^2 and 28^2 are no multiples of 16 and stay on conv_wino4b's packed items."""
    kern = _check(1, 224, 34, 2, (0,))
    assert sum(k.startswith("conv_wino4b<f4x4,16t") for k in kern) >= 2 * LAYERS[1] - 1, kern


def test_a_map_that_is_no_multiple_of_16_stays_nhwc():
    """tile 96, N = 2: 48^2 runs planar, 24^2 does not."""
    _check(2, 96, 35, 1, (0,))


# ---- kernel level, through the developers' library ---------------------------------------------------------------------------------------------------
def _dev():
    """the bindings module and the developers' library; dev_kernels._SIGS declares the signatures of the cerb_devfwd_* entries used here"""
    return D, D.lib()


@dev_switches
def test_residual_instantiation_matches_conv_wino4b():
    """conv_wino4p's residual instantiation against conv_wino4b<...,res> on the same weights: out of place and written over the residual; then
    planar_to_nhwc of the buffer the convolution wrote.  16^2 x 64 -> 64 with three images (the last pair repeats a block), 32^2 x 128 -> 128 with one."""
    for n, hw, c in ((3, 16, 64), (1, 32, 128)):
        _residual_case(n, hw, c)


def _residual_case(n, hw, c):
    D, L = _dev()
    g = torch.Generator().manual_seed(100 + c)
    w = (torch.randn((c, c, 3, 3), generator=g) / (3.0 * c ** 0.5)).contiguous()
    bias = (0.1 * torch.randn((c,), generator=g)).cuda()
    x = torch.randn((n, hw, hw, c), generator=g).cuda()
    res = torch.randn((n, hw, hw, c), generator=g).cuda()
    xb, rb = D.banded(x, hw), D.banded(res, hw)  # (kept alive: the NHWC kernels read their inputs through a zero guard band)
    ref = D.Guarded((n, hw, hw, c))
    D.ok(L.cerb_devfwd_conv3x3(C.c_void_p(w.data_ptr()), D.ptr(bias), D.ptr(xb), D.ptr(rb), D.ptr(ref), n, hw, hw, c, c, 1, 0, D.stream()), "nhwc")
    assert ref.intact() and float((ref.t > 0).float().mean()) > 0.2 and float((ref.t == 0).float().mean()) > 0.2, "the ReLU floor must cut some values, not all"
    xp, rp = _to_planar(x), _to_planar(res)
    size = int(L.cerb_devfwd_planar_elems(n, hw, hw, c))
    assert size == xp.numel()
    out = D.Guarded((size,), init=torch.zeros(size))
    D.ok(L.cerb_devfwd_conv3x3(C.c_void_p(w.data_ptr()), D.ptr(bias), D.ptr(xp), D.ptr(rp), D.ptr(out), n, hw, hw, c, c, 1, 1, D.stream()), "planar")
    assert out.intact()
    _check_planar(out.t, ref.t, "out of place")
    assert torch.equal(rp, _to_planar(res)), "the residual is only read"
    inplace = D.Guarded((size,), init=rp.cpu())
    D.ok(L.cerb_devfwd_conv3x3(C.c_void_p(w.data_ptr()), D.ptr(bias), D.ptr(xp), D.ptr(inplace), D.ptr(inplace), n, hw, hw, c, c, 1, 1, D.stream()), "in place")
    assert inplace.intact()
    _check_planar(inplace.t, ref.t, "in place")
    # the non-residual encoder instantiation on the same input, then the stage exit of both buffers
    ref0 = D.Guarded((n, hw, hw, c))
    D.ok(L.cerb_devfwd_conv3x3(C.c_void_p(w.data_ptr()), D.ptr(bias), D.ptr(xb), None, D.ptr(ref0), n, hw, hw, c, c, 1, 0, D.stream()), "nhwc, no residual")
    out0 = D.Guarded((size,), init=torch.zeros(size))
    D.ok(L.cerb_devfwd_conv3x3(C.c_void_p(w.data_ptr()), D.ptr(bias), D.ptr(xp), None, D.ptr(out0), n, hw, hw, c, c, 1, 1, D.stream()), "planar, no residual")
    assert ref0.intact() and out0.intact()
    _check_planar(out0.t, ref0.t, "no residual")
    for buf, want in ((inplace, ref), (out0, ref0)):
        back = D.Guarded((n, hw, hw, c))
        D.ok(L.cerb_devfwd_planar_to_nhwc(D.ptr(buf), D.ptr(back), n, hw, hw, c, D.stream()), "planar_to_nhwc")
        assert back.intact() and torch.equal(back.t, want.t)
        _check_planar(buf.t, want.t, "the exit pass only reads")


@dev_switches
def test_stride2_and_maxpool_planar_stores_match_the_nhwc_stores():
    """conv_igemm's planar epilogue against its NHWC one: 16 x 16 tiles (32^2 -> 16^2), 8 x 32 tiles (64^2 -> 32^2) and tiles that hang over the map
    (96^2 -> 48^2), 3x3 and 1x1; the max-pool's planar store against its NHWC one at 32^2 -> 16^2 and 64^2 -> 32^2."""
    for ks, n, hw, cin, cout in ((3, 2, 32, 64, 128), (1, 2, 32, 64, 128), (3, 1, 96, 64, 64), (1, 1, 64, 128, 256)):
        _stride2_case(ks, n, hw, cin, cout)
    for n, hw in ((2, 32), (1, 64)):
        _maxpool_case(n, hw)


def _stride2_case(ks, n, hw, cin, cout):
    D, L = _dev()
    g = torch.Generator().manual_seed(200 + ks + hw)
    w = (torch.randn((cout, cin, ks, ks), generator=g) / (ks * cin ** 0.5)).contiguous()
    bias = (0.1 * torch.randn((cout,), generator=g)).cuda()
    x = D.banded(torch.randn((n, hw, hw, cin), generator=g).cuda(), hw)
    relu = 1 if ks == 3 else 0  # conv1 of the block has a ReLU, the downsample has none
    ho = hw // 2
    ref = D.Guarded((n, ho, ho, cout))
    D.ok(L.cerb_devfwd_conv_s2(C.c_void_p(w.data_ptr()), D.ptr(bias), D.ptr(x), D.ptr(ref), n, hw, hw, cin, cout, ks, relu, 0, D.stream()), "nhwc")
    size = int(L.cerb_devfwd_planar_elems(n, ho, ho, cout))
    out = D.Guarded((size,), init=torch.zeros(size))
    D.ok(L.cerb_devfwd_conv_s2(C.c_void_p(w.data_ptr()), D.ptr(bias), D.ptr(x), D.ptr(out), n, hw, hw, cin, cout, ks, relu, 1, D.stream()), "planar")
    assert ref.intact() and out.intact() and float(ref.t.abs().mean()) > 0.0
    _check_planar(out.t, ref.t, (ks, hw))


def _maxpool_case(n, hw):
    D, L = _dev()
    x = torch.randn((n, hw, hw, 64), generator=torch.Generator().manual_seed(300 + hw)).cuda()
    ho = hw // 2
    ref = D.Guarded((n, ho, ho, 64))
    D.ok(L.cerb_devfwd_maxpool(D.ptr(x), D.ptr(ref), n, hw, hw, 64, 0, D.stream()), "nhwc")
    size = int(L.cerb_devfwd_planar_elems(n, ho, ho, 64))
    out = D.Guarded((size,), init=torch.zeros(size))
    D.ok(L.cerb_devfwd_maxpool(D.ptr(x), D.ptr(out), n, hw, hw, 64, 1, D.stream()), "planar")
    assert ref.intact() and out.intact()
    _check_planar(out.t, ref.t, hw)
