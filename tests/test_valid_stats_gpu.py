"""cerberus_amd.valid_stats on the GPU (cerb_valid_stats_* through the C ABI): integer-equal to what the REFERENCE's own ProcStepRawOutput accumulated
(tests/golden/valid_stats.npz), to the numpy restatement where the reference has no answer (N = 1, a Patch-Class target in the batch), and the
fused valid_step_stats against valid_step + update."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from valid_stats_helpers import CHANNEL_INFO, HEADS, MAXC, edge_step, golden_steps, nested, restate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return golden_steps()


@pytest.fixture(scope="module")
def vstep():
    return np.load(os.path.join(GOLDEN, "valid_step.npz"))


@pytest.fixture(scope="module")
def model(vstep):
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    m = create_model(**default_model_kwargs())
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(int(vstep["weight_seed"])).items()}, strict=True)
    return m


def _stats():
    from cerberus_amd.valid_stats import ValidStats

    return ValidStats(CHANNEL_INFO)


def _raw(pred, true, dummy):
    return {"pred": pred, "true": true, "dummy": dummy, "channel_info": CHANNEL_INFO}


def _batch(vstep, case):
    heads = [str(h) for h in vstep["heads"]]
    has = np.full(vstep[case + "has_target"].shape, None, dtype=object)
    for j, h in enumerate(heads):
        has[vstep[case + "has_target"][:, j], j] = h
    batch = {"img": torch.from_numpy(vstep[case + "img"]), "dummy_target": has}
    for h in heads:
        batch[h] = torch.from_numpy(vstep[case + "target/" + h])
    return batch


def test_reference_arrays_in_reference_counters_out(gold):
    """The epoch of the fixture through ValidStats.update: the accumulator equals the reference's after EACH step, as integers; counters() is the
    reference's nested dict; scalars() equals proc_cum_epoch_step_output's with == and has its keys in its order."""
    g, steps = gold
    st = _stats()
    for name, pred, true, dummy, hw, exp in steps:
        st.update(_raw(pred, true, dummy))
        got = st.counters_int()
        assert got.dtype == np.int64 and got.shape == (len(HEADS), MAXC, 4)
        assert np.array_equal(got, exp.astype(np.int64)) and np.array_equal(got.astype(np.float64), exp), (name, np.argwhere(got != exp)[:5])
    assert st.steps == 3
    cnt = st.counters()
    assert cnt == nested(steps[-1][5].astype(np.int64)) and list(cnt) == list(HEADS)
    assert list(cnt["Nuclei-TYPE"]) == list(range(1, 7)) and list(cnt["Patch-Class"]) == list(range(9)) and isinstance(cnt["Lumen-INST"][1]["over_inter"], np.float64)
    sc = st.scalars()
    assert list(sc.keys()) == [str(n) for n in g["scalar_names"]]
    for n, v in zip(g["scalar_names"], g["scalar_values"]):
        assert sc[str(n)] == v, (str(n), sc[str(n)], v)


def test_edge_step_equals_the_restatement(gold):
    """N = 1 (the case the reference's squeeze gets wrong), probabilities exactly 0.5, nextafter(0.5, 0 / 1) and NaN, labels above the class range and
    NaN labels, an all-dummy head, a Patch-Class map that varies inside the tile, odd sizes that take the one-pixel path."""
    for hw, seed in (((12, 20), 3), ((7, 9), 4)):
        pred, true, dummy, hw = edge_step(1, hw[0], hw[1], seed)
        exp = restate(np.zeros((len(HEADS), MAXC, 4), np.int64), pred, true, dummy, hw)
        assert exp[0, 1, 0] > 0 and exp[3, 1, 1] > 0 and exp[5, 0, 2] > 0 and not exp[1].any()
        st = _stats()
        st.update(_raw(pred, true, dummy))
        assert np.array_equal(st.counters_int(), exp), (hw, np.argwhere(st.counters_int() != exp)[:5])
        sq = _stats()  # the same step torch.squeeze'd, as the reference's valid_step would hand it over
        sq.update(_raw({k: np.squeeze(v) for k, v in pred.items()}, {k: np.squeeze(v) for k, v in true.items()}, dummy))
        assert np.array_equal(sq.counters_int(), exp)


def test_input_forms_agree_bit_for_bit(gold):
    """numpy vs CUDA tensors, int32 vs float32 true maps, uint8 vs int64 type maps, natural shapes (trailing 1 on the true maps, Patch-Class as a map
    or as one value per sample) vs squeezed ones: one accumulator, bit for bit."""
    g, steps = gold
    name, pred, true, dummy, hw, _ = steps[2]  # step c: int32 true maps, uint8 type maps, Patch-Class one value per sample
    n = dummy.shape[0]
    assert true["Lumen-INST"].dtype == np.int32 and pred["Nuclei-TYPE"].dtype == np.uint8 and pred["Patch-Class"].shape == (n,)
    base = _stats()
    base.update(_raw(pred, true, dummy), hw=hw)
    ref = base.counters_int()
    assert ref.any() and np.array_equal(ref, restate(np.zeros_like(ref), pred, true, dummy, hw))
    spread = lambda a: np.ascontiguousarray(np.broadcast_to(a.reshape(n, 1, 1), (n,) + hw))
    forms = {
        "cuda": ({k: torch.from_numpy(v).cuda() for k, v in pred.items()}, {k: torch.from_numpy(v).cuda() for k, v in true.items()}),
        "float32 true": (pred, {k: v.astype(np.float32) for k, v in true.items()}),
        "int64 true and type": ({k: (v.astype(np.int64) if k.endswith("TYPE") else v) for k, v in pred.items()}, {k: v.astype(np.int64) for k, v in true.items()}),
        "trailing 1": (pred, {k: (v.reshape(n, 1, 1, 1) if k == "Patch-Class" else v[..., None]) for k, v in true.items()}),
        "patch-class maps": ({k: (spread(v) if k == "Patch-Class" else v) for k, v in pred.items()}, {k: (spread(v) if k == "Patch-Class" else v) for k, v in true.items()}),
        "patch-class map vs value": ({k: (spread(v) if k == "Patch-Class" else v) for k, v in pred.items()}, true),
        "non-contiguous": ({k: (torch.from_numpy(np.concatenate([v, v], -1)).cuda()[..., :2] if k.endswith("INST") else v) for k, v in pred.items()}, true),
    }
    for what, (p, t) in forms.items():
        st = _stats()
        st.update(_raw(p, t, dummy), hw=hw)
        got = st.counters_int()
        assert got.tobytes() == ref.tobytes(), (what, np.argwhere(got != ref)[:5])


def test_two_runs_a_side_stream_and_reset(gold):
    g, steps = gold
    final = steps[-1][5].astype(np.int64)
    a, b = _stats(), _stats()
    for name, pred, true, dummy, hw, _ in steps:
        a.update(_raw(pred, true, dummy))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        for name, pred, true, dummy, hw, _ in steps:
            b.update(_raw(pred, true, dummy))
    side.synchronize()
    assert a.counters_int().tobytes() == b.counters_int().tobytes() == final.tobytes()
    a.reset()  # a fresh epoch
    assert a.steps == 0 and not a.counters_int().any()
    name, pred, true, dummy, hw, exp = steps[0]
    a.update(_raw(pred, true, dummy))
    assert np.array_equal(a.counters_int(), exp.astype(np.int64))
    with pytest.raises(TypeError, match="CUDA"):
        a.update_device(pred, true, dummy)
    with pytest.raises(ValueError):
        a.update(_raw(pred, {k: v[:, :50] for k, v in true.items()}, dummy))
    assert np.array_equal(a.counters_int(), exp.astype(np.int64))  # the refused steps added nothing


def test_patch_class_target_in_the_batch(vstep, model):
    """Where the reference raises (a Patch-Class target in the batch): the per-head rules on the natural maps.  The reference's own valid_step arrays
    of that batch -- 'true' [N, H, H, W] -- give the restatement's counters on (pred, the targets fed in); so does cerberus_amd's valid_step."""
    from cerberus_amd.train import valid_step

    case = "pc/"
    batch = _batch(vstep, case)
    dummy = batch["dummy_target"]
    hw = tuple(vstep[case + "img"].shape[1:3])
    assert vstep[case + "true/Lumen-INST"].ndim == 4 and np.any(dummy == "Patch-Class")
    target = {k: vstep[case + "target/" + k] for k in HEADS}
    pred = {k: vstep[case + "pred/" + k] for k in HEADS}
    exp = restate(np.zeros((len(HEADS), MAXC, 4), np.int64), pred, target, dummy, hw)
    assert exp[5, :9, 3].min() > 0 and exp[5, :, 1].any() and exp[0, 1, 0] > 0
    st = _stats()
    st.update(_raw(pred, {k: vstep[case + "true/" + k] for k in HEADS}, dummy))
    assert np.array_equal(st.counters_int(), exp), np.argwhere(st.counters_int() != exp)[:5]
    raw = valid_step(dict(batch), ({"net": {"desc": model}}, None))["raw"]
    assert raw["true"]["Gland-TYPE"].ndim == 4
    st.reset()
    st.update(raw)
    got = st.counters_int()
    assert np.array_equal(got, restate(np.zeros_like(got), raw["pred"], target, dummy, hw))
    nat = _stats()  # the same predictions with the natural targets
    nat.update(_raw(raw["pred"], target, dummy))
    assert nat.counters_int().tobytes() == got.tobytes()


@pytest.mark.parametrize("case", ["nopc/", "pc/"])
def test_fused_step_equals_valid_step_plus_update(vstep, gold, model, case):
    """valid_step_stats: the same forward and the same decisions as valid_step, so the same integers as ValidStats.update(valid_step(batch)['raw']);
    nothing heavier than 'dummy' and 'channel_info' comes back.  On nopc/ every counter of a head is within 2 * k_head of the reference's own
    (k_head: the flagged pixels the reference's forward decides within 1e-4, from the fixture) and nr_pixels is exact."""
    from cerberus_amd.train import valid_step
    from cerberus_amd.valid_stats import ValidStats, valid_step_stats, validate

    batch = _batch(vstep, case)
    run_info = ({"net": {"desc": model}}, None)
    raw = valid_step(dict(batch), run_info)["raw"]
    two = ValidStats(raw["channel_info"])
    two.update(raw)
    fused = ValidStats(raw["channel_info"])
    res = valid_step_stats(dict(batch), run_info, fused)
    assert list(res) == ["raw"] and sorted(res["raw"]) == ["channel_info", "dummy"] and res["raw"]["dummy"].shape == batch["dummy_target"].shape
    assert list(res["raw"]["channel_info"]) == list(model.decoder_info_list) and list(fused.heads) == list(HEADS)
    got = fused.counters_int()
    assert got.any() and got.tobytes() == two.counters_int().tobytes(), np.argwhere(got != two.counters_int())[:5]
    assert validate(model, [batch, batch], stats=fused) == validate(model, [batch, batch]) and fused.steps == 2
    assert np.array_equal(fused.counters_int(), 2 * got)
    if case == "nopc/":
        g, steps = gold
        exp = steps[0][5].astype(np.int64)
        k_head = dict(zip([str(n) for n in g["k_head_names"]], [int(k) for k in g["k_head"]]))
        for i, key in enumerate(HEADS):
            assert np.array_equal(got[i, :, 3], exp[i, :, 3]), key  # nr_pixels
            diff = int(np.abs(got[i] - exp[i]).max())
            print("%-12s largest counter difference to the reference %d (k_head %s)" % (key, diff, k_head.get(key, "-")))
            assert diff <= 2 * k_head.get(key, 0), (key, diff)
        # a model in training mode validates through its inference twin: the same weights, the same integers
        from cerberus_amd.net_desc import create_model
        from cerberus_amd.weights import default_model_kwargs

        m = create_model(**default_model_kwargs())
        m.load_state_dict(model.state_dict(), strict=True)
        m.train()
        m.forward_train(batch["img"].cuda())
        tw = ValidStats(raw["channel_info"])
        valid_step_stats(dict(batch), ({"net": {"desc": m}}, None), tw)
        assert tw.counters_int().tobytes() == got.tobytes()


def test_device_maps_in_no_host_copy(model):
    """gen_targets_batch's maps and infer_tiles' maps go into update_device as they are: every map passed is a CUDA tensor, and the counters equal those
    of the same arrays fed from the host."""
    from cerberus_amd.targets import gen_targets_batch

    rs = np.random.RandomState(11)
    n, s = 3, 96
    yy, xx = np.mgrid[0:s, 0:s]
    inst = np.zeros((n, s, s), np.int32)
    for i in range(n):
        for j in range(12):
            cy, cx, r = rs.uniform(0, s), rs.uniform(0, s), rs.uniform(5, 14)
            inst[i][(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = j + 1
    ann = np.stack([inst, inst, inst, np.where(inst > 0, rs.randint(1, 7, inst.shape), 0), np.where(inst > 0, rs.randint(1, 3, inst.shape), 0),
                    np.broadcast_to(rs.randint(0, 9, (n, 1, 1)), inst.shape)], -1).astype(np.int32)
    c2t = OrderedDict([("Lumen-INST", "IP-ERODED-CONTOUR-3"), ("Gland-INST", "IP-ERODED-CONTOUR-11"), ("Nuclei-INST", "IP-ERODED-CONTOUR-3"), ("Nuclei-TYPE", "TP"),
                       ("Gland-TYPE", "TP"), ("Patch-Class", "PC")])
    tgt = gen_targets_batch(torch.from_numpy(ann).cuda(), list(c2t), c2t, (s, s))
    dummy = tgt["dummy_target"]
    dummy[1, :] = None  # one sample without targets
    tiles = torch.from_numpy(rs.randint(0, 256, (n, s, s, 3)).astype(np.uint8)).cuda()
    for dtype in (torch.int64, torch.uint8):
        pred = model.infer_tiles(tiles, [s, s], type_dtype=dtype)
        true = {k: tgt[k] for k in HEADS}
        for d in (pred, true):
            assert all(torch.is_tensor(d[k]) and d[k].is_cuda for k in HEADS)
        assert true["Lumen-INST"].dtype == torch.int32 and tuple(true["Lumen-INST"].shape) == (n, s, s, 1) and pred["Nuclei-TYPE"].dtype == dtype
        dev = _stats()
        dev.update_device(pred, true, dummy)
        host = _stats()
        host.update(_raw({k: v.cpu().numpy() for k, v in pred.items()}, {k: v.cpu().numpy() for k, v in true.items()}, dummy))
        got = dev.counters_int()
        assert got.tobytes() == host.counters_int().tobytes()
        exp = restate(np.zeros_like(got), {k: v.cpu().numpy() for k, v in pred.items()}, {k: v.cpu().numpy() for k, v in true.items()}, dummy, (s, s))
        assert np.array_equal(got, exp) and got[0, 1, 3] == 2 * s * s and got[:, :, 1].any()
