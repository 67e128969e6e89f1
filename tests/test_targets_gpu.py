"""cerberus_amd.targets on the GPU against what the REFERENCE's own gen_targets returned (tests/golden/targets.npz, written by
tests/tools/gen_golden_targets.py): class maps exactly, weight maps to 4e-6, the distance sum behind them bit for bit."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT  # noqa: F401

pytestmark = pytest.mark.gpu

# |device - reference| per weight-map pixel.  Everything up to x = (d1 + d2) / sigma is bit-exact; numpy's float32 exp (documented up to about
# 2.5 ulp) and expf (1 ulp) differ by at most about 3.5 ulp relative, times w0 = 10 -> 2.1e-6, plus the two roundings of values below 16
# (ulp 9.5e-7 each).
WMAP_BAR = 4e-6


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "targets.npz"))


def _case(g, name):
    c2t = OrderedDict((str(h), str(c)) for h, c in zip(g[name + "/c2t_heads"], g[name + "/c2t_codes"]))
    kw = {} if bool(g[name + "/gen_unet_weight_map"]) else {"gen_unet_weight_map": False}
    return g[name + "/ann"].astype(np.int32), [str(c) for c in g[name + "/channel"]], c2t, tuple(int(v) for v in g[name + "/crop"]), kw


def _cases(g):
    return [str(c) for c in g["cases"]]


def test_every_map_against_the_reference(gold):
    """Every fixture case through gen_targets: keys, order, has_flag, shapes and dtypes; class / pixel maps equal on EVERY pixel; weight maps
    within WMAP_BAR on every pixel; d1 + d2 (return_dsum) equal to the stored near_1 + near_2 bit for bit."""
    from cerberus_amd.targets import gen_targets

    worst, n_dsum = 0.0, 0
    for name in _cases(gold):
        ann, channel, c2t, crop, kw = _case(gold, name)
        tgt, has_flag, dsum = gen_targets(torch.from_numpy(ann).cuda(), channel, c2t, crop, "seg", return_dsum=True, **kw)
        assert isinstance(tgt, OrderedDict) and list(tgt.keys()) == [str(k) for k in gold[name + "/keys"]], name
        assert [("" if v is None else v) for v in has_flag] == [str(v) for v in gold[name + "/has_flag"]], name
        for k, v in tgt.items():
            exp = gold[name + "/out/" + k]
            assert v.is_cuda and tuple(v.shape) == crop + (1,) == exp.shape, (name, k)
            got = v.cpu().numpy()
            head = k[: -len("#WEIGHT-MAP")] if k.endswith("#WEIGHT-MAP") else k
            if head not in channel:  # dummy fill
                assert v.dtype == torch.float32 and not got.any() and not exp.any(), (name, k)
            elif k.endswith("#WEIGHT-MAP"):
                assert v.dtype == torch.float32 and exp.dtype == np.float32
                err = float(np.abs(got.astype(np.float64) - exp.astype(np.float64)).max())
                worst = max(worst, err)
                print("weight map %-28s %-22s max |device - reference| = %.3e" % (name, k, err))
                assert err <= WMAP_BAR, (name, k, err)
            else:
                assert v.dtype == torch.int32
                assert np.array_equal(got, exp.astype(np.int32)), (name, k, int((got != exp).sum()))
        for head, d in dsum.items():
            key = name + "/dsum/" + head
            if key not in gold.files:
                continue
            exp = gold[key]
            got = d.cpu().numpy()
            assert got.dtype == np.float32 == exp.dtype and got.shape == exp.shape
            assert got.tobytes() == exp.tobytes(), (name, head, int((got != exp).sum()), float(np.abs(got - exp).max()))
            n_dsum += 1
    print("largest weight-map difference over all cases: %.3e (bar %.1e)" % (worst, WMAP_BAR))
    assert n_dsum >= 18


def test_numpy_annotation_and_wide_integer_types_are_accepted(gold):
    from cerberus_amd.targets import gen_targets

    ann, channel, c2t, crop, kw = _case(gold, "sparse_ids")
    a, _ = gen_targets(torch.from_numpy(ann).cuda(), channel, c2t, crop, "seg")
    for other in (ann, ann.astype(np.int64), torch.from_numpy(ann.astype(np.int64)).cuda()):
        b, _ = gen_targets(other, channel, c2t, crop, "seg")
        for k in a:
            assert b[k].is_cuda and torch.equal(a[k], b[k]), k


def test_whole_annotation_modes(gold):
    """task_mode != 'seg' hands every getter the whole annotation (loader/targets.py:226-227): a 2-D annotation gives what the channel gives in
    'seg' mode; a 3-D one leaves only the dummy fills in the reference's final list, paired with the leading codes."""
    from cerberus_amd.targets import gen_targets

    ann, channel, c2t, crop, kw = _case(gold, "split_and_removed_c3")
    a, fa = gen_targets(torch.from_numpy(ann).cuda(), channel, c2t, crop, "seg")
    b, fb = gen_targets(torch.from_numpy(ann[..., 0]).cuda(), channel, c2t, crop, "class")
    assert fa == fb and list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    c, fc = gen_targets(torch.from_numpy(np.repeat(ann, 2, -1)).cuda(), ["T"], OrderedDict([("T", "TP"), ("X", "IP")]), crop, "class")
    assert fc == ["T", None] and list(c) == ["T"] and c["T"].dtype == torch.float32 and not bool(c["T"].any())
    with pytest.raises(ValueError, match="2-D"):
        gen_targets(torch.from_numpy(np.repeat(ann, 2, -1)).cuda(), ["N"], c2t, crop, "class")


def test_batch_equals_singles_and_is_bitwise_reproducible(gold):
    """gen_targets_batch on stacked annotations with different instance counts (0, 1, few, many) == the single-sample calls, bit for bit, and two
    calls on the same batch give identical bits for every output (class maps, weight maps, distance sums)."""
    from cerberus_amd.targets import gen_targets, gen_targets_batch

    nuc = _case(gold, "nuclei_c3_crop")[0]
    gla = _case(gold, "gland_c11_crop")[0]
    one = np.zeros_like(nuc)
    one[100:140, 90:150] = 9
    two = one.copy()
    two[80:95, 60:85] = 4  # 5 pixels from the first: their windows overlap
    batch = np.stack([nuc, np.zeros_like(nuc), one, gla, two])
    ann = torch.from_numpy(np.concatenate([batch, batch[::-1]], -1).copy()).cuda()  # channel 0 / channel 1: the same maps in the opposite sample order
    c2t = OrderedDict([("A", "IP-ERODED-CONTOUR-3"), ("B", "IP-ERODED-CONTOUR-11"), ("A2", "IP-ERODED-11"), ("B-IP", "IP")])
    channel = ["A", "B", "A2", "B-IP"]
    ann = torch.cat([ann, ann], -1).contiguous()
    crop = (200, 176)
    out1, ds1 = gen_targets_batch(ann, channel, c2t, crop, return_dsum=True)
    out2, ds2 = gen_targets_batch(ann, channel, c2t, crop, return_dsum=True)
    assert sorted(out1) == sorted(["A", "A#WEIGHT-MAP", "B", "B#WEIGHT-MAP", "A2", "A2#WEIGHT-MAP", "B-IP", "dummy_target"])
    assert out1["dummy_target"].shape == (5, 10) and out1["dummy_target"].dtype == object
    for k in out1:
        if k == "dummy_target":
            assert np.array_equal(out1[k], out2[k])
            continue
        assert out1[k].is_cuda and tuple(out1[k].shape) == (5,) + crop + (1,)
        assert out1[k].dtype == (torch.float32 if k.endswith("#WEIGHT-MAP") else torch.int32), k
        assert torch.equal(out1[k], out2[k]) and out1[k].cpu().numpy().tobytes() == out2[k].cpu().numpy().tobytes(), k
    for k in ds1:
        assert torch.equal(ds1[k], ds2[k]), k
    assert sorted(ds1) == ["A", "A2", "B"]
    # the weight maps of the empty and the one-instance samples are all 1, the others are not
    wa = out1["A#WEIGHT-MAP"]
    assert float(wa[1].min()) == 1.0 == float(wa[1].max()) and float(wa[2].max()) == 1.0 and float(wa[0].max()) > 1.5 and float(wa[4].max()) > 1.0
    for n in range(5):
        single, has_flag, dss = gen_targets(ann[n], channel, c2t, crop, "seg", return_dsum=True)
        assert list(out1["dummy_target"][n]) == has_flag
        for k, v in single.items():
            assert torch.equal(v, out1[k][n]), (n, k)
        for k, v in dss.items():
            assert torch.equal(v, ds1[k][n]), (n, k)


def test_batch_without_weight_maps_synchronises_nothing_and_gives_ones(gold):
    from cerberus_amd.targets import gen_targets_batch

    ann, channel, c2t, crop, kw = _case(gold, "no_weight_map")
    out = gen_targets_batch(torch.from_numpy(ann[None]).cuda(), channel, c2t, crop, gen_unet_weight_map=False)
    assert np.array_equal(out["N"][0].cpu().numpy(), gold["no_weight_map/out/N"].astype(np.int32))
    w = out["N#WEIGHT-MAP"]
    assert w.dtype == torch.float32 and float(w.min()) == 1.0 == float(w.max())


def test_generated_targets_feed_train_step_like_the_reference_maps(gold):
    """The dict gen_targets_batch returns for the 448 x 448 sample (twice, N = 2; the five dense heads of models/paramset.yml on a model built
    without the Patch-Class branch -- train_step takes that head's target as one number per sample, [N, 1, 1, 1], which no target code of
    gen_targets produces: 'PC' returns a map) goes into train_step as it is, CUDA tensors and all; every
    per-head loss equals that of the same step fed the reference's own maps from the fixture, within the bar tests/test_train_loss_gpu.py
    applies to losses."""
    from cerberus_amd.losses import PARAMSET_LOSS
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.targets import gen_targets_batch
    from cerberus_amd.train import Adam, train_step
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    name = "paramset_448"
    ann, channel, c2t, crop, kw = _case(gold, name)
    c2t = OrderedDict((h, c) for h, c in c2t.items() if h != "Patch-Class")
    heads = list(c2t)
    seed = int(np.load(os.path.join(GOLDEN, "train_loss.npz"))["weight_seed"])
    img = torch.from_numpy(np.random.RandomState(5).randint(0, 256, (2, 448, 448, 3)).astype(np.uint8))
    keep = None  # no Patch-Class branch: no dropout mask is drawn
    tasks = ["Lumen", "Gland", "Nuclei", "Nuclei#TYPE", "Gland#TYPE"]  # the model's considered_tasks: every decoder but Patch-Class

    def step(batch):
        m = create_model(**default_model_kwargs(considered_tasks=tasks))
        m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(seed, considered_tasks=tasks).items()}, strict=True)
        return train_step(batch, ({"net": {"desc": m, "optimizer": Adam(lr=1.0e-3), "extra_info": {"loss": PARAMSET_LOSS}}}, None), dropout_keep=keep)

    got_batch = gen_targets_batch(torch.from_numpy(np.stack([ann, ann])).cuda(), channel, c2t, crop)
    tensors = {k: v for k, v in got_batch.items() if k != "dummy_target"}
    assert all(v.is_cuda for v in tensors.values())
    before = {k: (v.data_ptr(), v.clone()) for k, v in tensors.items()}
    keys_before = list(got_batch)
    batch = dict(got_batch)
    batch["img"] = img
    res = step(batch)
    assert list(got_batch) == keys_before
    for k, v in tensors.items():  # the same device tensors, untouched
        assert got_batch[k] is v and v.is_cuda and v.data_ptr() == before[k][0] and torch.equal(v, before[k][1]), k
    ref_batch = {"img": img, "dummy_target": got_batch["dummy_target"]}
    for k in tensors:
        ref_batch[k] = torch.from_numpy(np.stack([gold[name + "/out/" + k]] * 2).astype(np.float32))
    exp = step(ref_batch)
    for h in heads:
        e, g_ = float(exp["EMA"][h + "_loss"]), float(res["EMA"][h + "_loss"])
        print("%-12s loss with generated targets %.7f, with the reference's maps %.7f" % (h, g_, e))
        assert abs(g_ - e) <= 1e-4 * max(1.0, abs(e)), (h, g_, e)
    assert abs(float(res["EMA"]["overall_loss"]) - float(exp["EMA"]["overall_loss"])) <= 1e-4 * max(1.0, abs(float(exp["EMA"]["overall_loss"])))
    assert float(exp["EMA"]["Nuclei-INST_loss"]) > 0
