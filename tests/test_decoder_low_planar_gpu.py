"""The decoder's two lowest levels (32^2 x 256 -> 128 and 64^2 x 128 -> 64 channels on a 256-pixel tile) in the tile-planar layout: their entry pass
(upsample2_add_planar at C = 128 / 256) and their 3x3 convolutions on conv_wino4p.hip instead of conv_wino4b.hip.  Both kernels accumulate a position's
input channels in ascending groups of four in one matrix-instruction chain and share their transforms (wino_common.h), so the planar levels must give
the bits of the NHWC path: torch.equal on every output of every head and on the `logits` side outputs, planar levels on against cerb_net_set_planar(0).

Shapes: the smallest at which the new paths can go wrong -- one block per image at the lowest level (tile 128), an odd number of blocks there (the last
pair of a conv_wino4p item repeats a block), maps whose sides are multiples of 4 but not of 16 (tile 160: blocks hang over the map, the guard ring and the
never-written pixels must stay zero, also after a larger batch has used the same buffers), and a grouped launch of two decoders instead of five."""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import dev_switches

pytestmark = pytest.mark.gpu

LOW_CONV = "conv_wino4_planar<"      # profile families of the two lowest levels' convolutions (conv_plan.h: kPlanarFamily)
LOW_ENTRY = "upsample2_add_planar<"  # ... and of their entry passes
PLANAR_LOW_LEVELS = 2                # how many of the two lowest levels ship tile-planar (cerb_api.hip: kPlanarLowest = 0)
_models = {}


def _model(two_decoders=False):
    """Seeded weights; one handle per model for the whole file."""
    if two_decoders not in _models:
        from cerberus_amd.net_desc import create_model
        from cerberus_amd.weights import default_model_kwargs, make_state_dict

        kw = default_model_kwargs(["Gland", "Nuclei"] if two_decoders else None)
        if two_decoders:
            kw["decoder_kwargs"] = OrderedDict((k, OrderedDict(v)) for k, v in [("Gland", [("INST", 3)]), ("Nuclei", [("INST", 3)])])
        sd = {k: torch.from_numpy(v) for k, v in make_state_dict(7 if two_decoders else 5, kw["decoder_kwargs"], kw["considered_tasks"]).items()}
        m = create_model(**kw)
        m.load_state_dict(sd, strict=True)
        m.prepare()
        _models[two_decoders] = m
    return _models[two_decoders]


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


def _check(m, n, hw, seed, between=None):
    """planar levels on against cerb_net_set_planar(0); `between`: a batch size run on the same handle before the comparison is repeated."""
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
        if between:
            m.infer_tiles(_tiles(between, hw, seed + 1), hw)  # other values, more images, in every planar buffer
            _same(_all_outputs(m, t, hw), ref, "after a batch of %d" % between)
    finally:
        m.profile(False)
        m.set_planar(True)
    assert any(v.dtype == torch.float32 and 0.0 < float(v.abs().mean()) for v in ref.values()), "the comparison needs non-trivial maps"
    assert not any(k.startswith(LOW_CONV) or k.startswith(LOW_ENTRY) or k.startswith("conv_wino4p") for k in kern_nhwc), kern_nhwc
    # the planar kernels are the ones that ran (the records are those of the last forward: the logits call)
    assert sum(k.startswith(LOW_CONV) for k in kern) == 2 * PLANAR_LOW_LEVELS and sum(k.startswith(LOW_ENTRY) for k in kern) == PLANAR_LOW_LEVELS, kern
    assert sum(k.startswith("conv_wino4p<") for k in kern) == 4 and kern.count("upsample2_add_planar") == 2, kern
    assert (PLANAR_LOW_LEVELS < 2) == ("upsample2_add" in kern), kern


def test_one_block_per_image_at_the_lowest_level():
    """tile 128, N = 2: level maps 16^2, 32^2, 64^2, 128^2."""
    _check(_model(), 2, 128, 21)


def test_odd_block_count_at_the_lowest_level():
    """tile 128, N = 3: three blocks at the lowest level, the last pair repeats a block."""
    _check(_model(), 3, 128, 22)


def test_blocks_hang_over_the_map_and_nothing_stale_is_read():
    """tile 160, N = 1: level maps 20^2, 40^2, 80^2, 160^2; repeated on the same handle after a batch of three."""
    _check(_model(), 1, 160, 23, between=3)


def test_two_decoders_in_the_grouped_launch():
    """groups != 5: two dense decoders, no Patch-Class."""
    _check(_model(two_decoders=True), 2, 128, 24)


@dev_switches
@pytest.mark.parametrize("c", [128, 256])
def test_entry_pass_matches_the_nhwc_kernel_bit_for_bit(c):
    """upsample2_add_planar against upsample2_add on a 20^2 map (blocks hang over it), two groups, two images: every pixel of the tile-planar result
    equals the NHWC kernel's, from an NHWC `prev` shared by the groups (the lowest level's conv_map input, prev_gs = 0) and from a tile-planar `prev`
    per group; whatever no pixel maps to (guard ring, pixels beyond the map) is still zero."""
    import dev_kernels as D

    L = D.lib()   # (dev_kernels._SIGS declares the signatures of the cerb_devfwd_* entries)
    G, N, H, W = 2, 2, 20, 20
    g = torch.Generator().manual_seed(c)
    skip = torch.randn((N, H, W, c), generator=g).cuda()
    prev = torch.randn((G, N, H // 2, W // 2, c), generator=g).cuda()

    def planar_index(h, w):
        """float offset of channel 0 of pixel (y, x) of image 0, plane 0, and the strides (cerb_common.h: cerb_planar_offset)"""
        byp, bxp, ncc = (h + 15) // 16 + 2, (w + 15) // 16 + 2, c // 16
        y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        off = (((y // 16 + 1) * bxp + x // 16 + 1) * ncc) * 4096 + (((y % 4) * 4 + x % 4) * 16 + ((y // 4) % 4) * 4 + (x // 4) % 4) * 16
        return off, byp * bxp * ncc * 4096

    def to_nhwc(buf, n, h, w):
        off, per_image = planar_index(h, w)
        idx = (torch.arange(n).view(n, 1, 1, 1) * per_image + off.view(1, h, w, 1) + (torch.arange(c) // 16 * 4096 + torch.arange(c) % 16).view(1, 1, 1, c)).cuda()
        return buf[idx], idx

    def to_planar(t):  # [n][h][w][c] -> a zero-ringed tile-planar tensor
        n, h, w, _ = t.shape
        buf = torch.zeros(int(L.cerb_devfwd_planar_elems(n, h, w, c)), device="cuda")
        _, idx = to_nhwc(buf, n, h, w)
        buf[idx] = t
        return buf

    for prev_planar, shared in ((0, True), (0, False), (1, False)):
        case = (c, prev_planar, shared)
        ref = D.Guarded((G, N, H, W, c))
        pv = prev[0] if shared else prev
        D.ok(L.cerb_devfwd_upsample2_add(D.ptr(skip), D.ptr(pv.contiguous()), D.ptr(ref), G, N, H, W, c, 0 if shared else pv[0].numel(), D.stream()), case)
        gs = int(L.cerb_devfwd_planar_elems(N, H, W, c))
        out = D.Guarded((G, gs), init=torch.zeros(G * gs))
        if prev_planar:
            src = torch.stack([to_planar(prev[k]) for k in range(G)])
            prev_gs = src[0].numel()
        else:
            src, prev_gs = pv.contiguous(), 0 if shared else pv[0].numel()
        D.ok(L.cerb_devfwd_upsample2_add_planar(D.ptr(skip), D.ptr(src), D.ptr(out), G, N, H, W, c, prev_gs, gs, prev_planar, D.stream()), case)
        assert ref.intact() and out.intact(), case
        written = torch.zeros(G, gs, dtype=torch.bool, device="cuda")
        for k in range(G):
            got, idx = to_nhwc(out.t[k], N, H, W)
            assert torch.equal(got, ref.t[k]), (case, k, int((got != ref.t[k]).sum()))
            written[k].view(-1)[idx.reshape(-1)] = True
        assert bool((out.t[~written] == 0).all()), case
