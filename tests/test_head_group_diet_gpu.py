"""The grouped head kernel's per-shape bodies (cerberus_amd/csrc/net_kernels.hip: head_group_body<OUT_CH, KIND>) against its generic body, which is
the code every head ran before: the specialised bodies only leave out work no result needs, so EVERY output must be bit-identical.  The developers'
library reads CERB_HEAD_GENERIC at each launch (=1: the generic body for every head), so one process computes both; tiles of 96 x 96 (the smallest
geometry of the golden fixtures), N = 3.  Compared with torch.equal: INST probability maps, TYPE maps, Patch-Class, the `logits` of m(tiles) and the
logit_absmax words."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import dev_switches

pytestmark = pytest.mark.gpu
N, HW = 3, 96
MIXED = [("Lumen", [("INST", 2)]), ("Gland", [("INST", 3)]), ("Nuclei", [("INST", 2)]), ("Nuclei#TYPE", [("TYPE", 7)]), ("Gland#TYPE", [("TYPE", 3)]),
         ("Patch-Class", [("OUT", 9)])]  # tests/test_eroded_gpu.py
MULTIHEAD = [("Gland", [("INST", 3), ("TYPE", 3)])]  # several heads over one decoder


def _model(decoder_kwargs=None, tasks=None, seed=0, edit=None):
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    kw = default_model_kwargs(tasks)
    if decoder_kwargs is not None:
        kw["decoder_kwargs"] = OrderedDict((k, OrderedDict(v)) for k, v in decoder_kwargs)
    sd = {k: torch.from_numpy(v) for k, v in make_state_dict(seed, kw["decoder_kwargs"], kw["considered_tasks"]).items()}
    if edit is not None:
        edit(sd)
    m = create_model(**kw)
    m.load_state_dict(sd, strict=True)
    return m


def _tiles(seed=11):
    return torch.from_numpy(np.random.RandomState(seed).randint(0, 256, (N, HW, HW, 3)).astype(np.uint8)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _arm(m, generic, runs):
    """Every run of `runs` (name -> callable returning a dict of tensors) under one body, each with its own logit_absmax words."""
    assert os.environ.get("CERB_DEV_LIB") == "1"
    if generic:
        os.environ["CERB_HEAD_GENERIC"] = "1"
    else:
        os.environ.pop("CERB_HEAD_GENERIC", None)
    try:
        got = OrderedDict()
        for name, fn in runs.items():
            m.watch_logits()
            out = fn()
            words = m._logit_watch.clone()
            m.watch_logits(False)
            for k, v in out.items():
                got[name + "/" + k] = v.clone()
            got[name + "/logit_absmax"] = words
        torch.cuda.synchronize()
        return got
    finally:
        os.environ.pop("CERB_HEAD_GENERIC", None)


def _compare(m, runs, differ_ok=False):
    m.prepare()  # the load-time probe forward runs before either arm
    spec, gen = _arm(m, False, runs), _arm(m, True, runs)
    assert list(spec.keys()) == list(gen.keys()) and len(spec) >= 2 * len(runs)
    for k in spec:
        a, b = spec[k], gen[k]
        assert a.shape == b.shape and a.dtype == b.dtype, k
        assert torch.equal(_bits(a), _bits(b)), (k, int((_bits(a) != _bits(b)).sum()))
    return spec


def _default_runs(m, t):
    return OrderedDict([
        ("full_i64", lambda: m.infer_tiles(t, HW)),                               # the infer_step path
        ("full_u8", lambda: m.infer_tiles(t, HW, type_dtype=torch.uint8)),        # the canvas path (type_is_u8)
        # 3 x 71 x 3 = 639 sixteen-pixel blocks: an odd count (the last task has one block), and the 16-aligned cover is wider than the window
        ("crop_71x33", lambda: m.infer_tiles(t, [71, 33])),
        ("logits", lambda: m(t)),
    ])


@dev_switches
def test_default_model_planar_features():
    """Six heads (INST 3 x 3, TYPE 7, TYPE 3, Patch-Class): uncropped with int64 and uint8 TYPE maps, the odd-count crop, the logits side output."""
    m, t = _model(), _tiles()
    got = _compare(m, _default_runs(m, t))
    assert got["full_i64/Nuclei-TYPE"].dtype == torch.int64 and got["full_u8/Nuclei-TYPE"].dtype == torch.uint8
    assert got["crop_71x33/Gland-INST"].shape == (N, 71, 33, 2) and got["full_i64/Lumen-INST"].shape == (N, HW, HW, 2)
    assert torch.equal(got["full_i64/Nuclei-TYPE"], got["full_u8/Nuclei-TYPE"].long())
    assert len(torch.unique(got["full_i64/Nuclei-TYPE"])) > 2 and 0.0 < float(got["full_i64/Gland-INST"].mean()) < 1.0, "the comparison needs non-trivial maps"
    assert int((got["full_i64/logit_absmax"][:5] > 0).sum()) == 5


@dev_switches
def test_default_model_nhwc_features():
    """cerb_net_set_planar(0): the last decoder level, and with it the heads' features, in NHWC."""
    m, t = _model(seed=1), _tiles(12)
    m.set_planar(False)
    _compare(m, _default_runs(m, t))


@dev_switches
def test_two_class_inst_heads_next_to_three_class_ones():
    m, t = _model(MIXED, seed=2), _tiles(13)
    got = _compare(m, _default_runs(m, t))
    assert got["full_i64/Lumen-INST"].shape == (N, HW, HW, 1) and got["full_i64/Gland-INST"].shape == (N, HW, HW, 2)
    assert got["crop_71x33/Nuclei-INST"].shape == (N, 71, 33, 1) and got["logits/Lumen-INST"].shape == (N, 2, HW, HW)


@dev_switches
def test_multi_head_decoder():
    """{Gland: {INST, TYPE}}: two heads read one trunk."""
    m, t = _model(MULTIHEAD, tasks=["Gland"], seed=3), _tiles(14)
    got = _compare(m, _default_runs(m, t))
    assert got["full_i64/Gland-INST"].shape == (N, HW, HW, 2) and got["full_i64/Gland-TYPE"].shape == (N, HW, HW)


@dev_switches
def test_non_finite_hidden_channels_keep_their_bits():
    """+inf, -inf and nan in three hidden channels of one head's b1 (the conv bias in front of the folded BN): the one-instruction ReLU of the
    specialised bodies must give what fmaxf gave -- compared on the raw bit patterns, NaNs included."""
    def edit(sd):
        for d, h in (("Gland", "INST"), ("Nuclei#TYPE", "TYPE")):
            b = sd["output_head.%s.%s.x.0.block.0.conv.bias" % (d, h)]
            b[5], b[40], b[77] = float("inf"), float("-inf"), float("nan")

    old = os.environ.get("CERB_AUTO_PRECISION")
    os.environ["CERB_AUTO_PRECISION"] = "0"  # the load-time probe would answer infinite logits with another convolution algorithm
    try:
        m, t = _model(seed=4, edit=edit), _tiles(15)
        got = _compare(m, _default_runs(m, t))
    finally:
        if old is None:
            os.environ.pop("CERB_AUTO_PRECISION", None)
        else:
            os.environ["CERB_AUTO_PRECISION"] = old
    lg = got["logits/Gland-INST"]
    assert not torch.isfinite(lg).all(), "the planted values did not reach the logits"
    assert torch.isfinite(got["logits/Lumen-INST"]).all()
