"""cerberus_amd.inst_metrics on the GPU (cerb_inst_* through the C ABI) against the restatement in Python integers (tests/inst_metrics_ref.py).

Bars: every integer with ==.  sum_iou against the restatement's math.fsum: |d| <= K * 2^-52 * sum_iou with K the number of matched pairs -- the
worst case of re-ordering a float64 sum of K terms in (0.5, 1].  The ratios are host float64 from those numbers and held to the same relative
bound."""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import inst_metrics_cases as cases
import inst_metrics_ref as ref

pytestmark = pytest.mark.gpu

CASES = cases.cases()
RATIOS = ("dq", "sq", "pq", "aji", "dice2", "dice1")


def _check(got, want, what=""):
    """got: cerberus_amd.inst_metrics.summary's dict; want: the restatement's"""
    for k in cases.KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    rel = want["tp"] * 2.0 ** -52
    print("%s sum_iou %r restated %r bound %r" % (what, got["sum_iou"], want["sum_iou"], rel * want["sum_iou"]))
    assert abs(got["sum_iou"] - want["sum_iou"]) <= rel * want["sum_iou"], (what, got["sum_iou"], want["sum_iou"])
    for k in RATIOS:
        if math.isnan(want[k]):
            assert math.isnan(got[k]), (what, k, got[k])
        else:
            assert abs(got[k] - want[k]) <= rel * abs(want[k]), (what, k, got[k], want[k])


def _check_table(tab, true, pred):
    a, b, c = ref.pairs(true, pred)
    assert tab.true_ids.cpu().tolist() == sorted(a) and tab.true_area.cpu().tolist() == [a[i] for i in sorted(a)]
    assert tab.pred_ids.cpu().tolist() == sorted(b) and tab.pred_area.cpu().tolist() == [b[i] for i in sorted(b)]
    assert tab.true_ids.dtype == torch.int32 and tab.pairs.dtype == torch.int64 and tab.pairs.is_cuda
    assert [tuple(r) for r in tab.pairs.cpu().tolist()] == [(t, p, n) for (t, p), n in sorted(c.items())]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_hand_computed_cases(case):
    from cerberus_amd import inst_metrics as im

    name, true, pred, want, ious = case
    tab = im.pair_table(true, pred)
    got = im.summary(tab)
    assert tuple(got[k] for k in cases.KEYS) == want
    _check(got, ref.stats(true, pred), name)
    _check_table(tab, true, pred)
    pq = im.panoptic_quality(tab)
    assert (pq["tp"], pq["fp"], pq["fn"]) == want[:3] and pq["pq"] == got["pq"]
    for fn, k in ((im.aji, "aji"), (im.dice2, "dice2"), (im.dice1, "dice1")):
        v = fn(tab)
        assert (math.isnan(v) and math.isnan(got[k])) or v == got[k]
    with pytest.raises(ValueError):
        im.panoptic_quality(tab, match_iou=0.4)


@pytest.fixture(scope="module")
def blobs():
    true = cases.blob_labels(96, 130, 60, 5, 70000)
    pred = cases.blob_labels(96, 130, 64, 6, 70000)
    keep = cases.blob_labels(96, 130, 60, 5, 70000, rmin=2.5, rmax=8.0)  # the same centres and ids order, other radii: real matches
    pred = np.where(keep > 0, keep, pred).astype(np.int32)
    return true, pred, ref.stats(true, pred)


def test_odd_shape_with_id_gaps_and_as_a_strided_crop(blobs):
    from cerberus_amd import inst_metrics as im

    true, pred, want = blobs
    assert want["tp"] > 5 and want["fp"] > 5 and max(true.max(), pred.max()) > 50000
    tab = im.pair_table(true, pred)
    _check(im.summary(tab), want, "96x130")
    _check_table(tab, true, pred)
    big_t = torch.full((120, 200), 777, dtype=torch.int32, device="cuda")  # what lies around the crop must not be counted
    big_p = torch.full((131, 177), 888, dtype=torch.int32, device="cuda")
    vt, vp = big_t[5:101, 3:133], big_p[30:126, 41:171]
    vt.copy_(torch.from_numpy(true))
    vp.copy_(torch.from_numpy(pred))
    assert not vt.is_contiguous() and not vp.is_contiguous()
    tab2 = im.pair_table(vt, vp)
    _check(im.summary(tab2), want, "crop")
    assert torch.equal(tab2.pairs, tab.pairs) and torch.equal(tab2.true_area, tab.true_area) and torch.equal(tab2.pred_area, tab.pred_area)
    # a crop that starts 16-byte aligned in rows a multiple of four elements apart takes the 16-byte loads; its last four-pixel group (130 = 4 * 32 + 2) is partial
    big_t = torch.full((100, 200), 777, dtype=torch.int32, device="cuda")
    big_p = torch.full((100, 136), 888, dtype=torch.int32, device="cuda")
    vt, vp = big_t[2:98, 4:134], big_p[4:100, 0:130]
    assert vt.data_ptr() % 16 == 0 and vp.data_ptr() % 16 == 0 and vt.stride(0) % 4 == 0 and vp.stride(0) % 4 == 0
    vt.copy_(torch.from_numpy(true))
    vp.copy_(torch.from_numpy(pred))
    tab3 = im.pair_table(vt, vp)
    assert torch.equal(tab3.pairs, tab.pairs) and torch.equal(tab3.true_area, tab.true_area) and torch.equal(tab3.pred_area, tab.pred_area)


def test_noise_tile_spills_the_lds_table():
    from cerberus_amd import inst_metrics as im

    rs = np.random.RandomState(7)
    true, pred = rs.randint(1, 201, (64, 64)).astype(np.int32), rs.randint(1, 201, (64, 64)).astype(np.int32)
    tab = im.pair_table(true, pred)
    assert tab.n_pairs > 1024  # more distinct pairs in the one tile than the LDS table has slots
    _check_table(tab, true, pred)
    _check(im.summary(tab), ref.stats(true, pred), "noise")


def test_overflow_retry_gives_the_same_table():
    from cerberus_amd import inst_metrics as im

    rs = np.random.RandomState(8)
    true, pred = rs.randint(0, 24, (48, 80)).astype(np.int32), rs.randint(0, 24, (48, 80)).astype(np.int32)
    full = im.pair_table(true, pred)
    assert 400 <= full.n_pairs <= 600 and full.retries == 0
    small = im.pair_table(true, pred, _capacity=64)
    assert small.retries >= 1
    assert torch.equal(small.pairs, full.pairs) and torch.equal(small.true_area, full.true_area)
    assert im.summary(small) == im.summary(full)
    _check_table(small, true, pred)


def test_ids_outside_the_bounds_are_background(blobs):
    from cerberus_amd import inst_metrics as im

    true, pred, _ = blobs
    t, p = true.copy(), pred.copy()
    t[10:14, 20:30], p[50:53, 60:70] = -5, -(2 ** 31)
    bound = 70000
    t[70:75, 5:9], p[0:3, 100:130] = bound + 1, 2 ** 31 - 1
    tz, pz = np.where((t < 0) | (t > bound), 0, t), np.where((p < 0) | (p > bound), 0, p)
    tab = im.pair_table(t, p, max_true_id=bound, max_pred_id=bound)
    want = im.pair_table(tz, pz)
    assert torch.equal(tab.pairs, want.pairs) and torch.equal(tab.true_ids, want.true_ids) and torch.equal(tab.pred_area, want.pred_area)
    _check(im.summary(tab), ref.stats(tz, pz), "bounds")


@pytest.fixture(scope="module")
def nuclei_1024():
    from cerberus_amd.postproc import postproc_device
    from cerberus_amd.synth_maps import nuclei_maps

    prob = torch.from_numpy(nuclei_maps(1024, 1024, 3, density_per_mpx=3000.0)).cuda()
    true, _ = postproc_device(prob, "Nuclei")
    pred, _ = postproc_device(torch.roll(prob, (2, 1), (0, 1)).contiguous(), "Nuclei")
    pred = torch.where(pred % 11 == 3, torch.zeros_like(pred), pred)  # some misses
    return true, pred, ref.stats(true.cpu().numpy(), pred.cpu().numpy())


def test_1024_nuclei_map_and_bitwise_repeat(nuclei_1024):
    from cerberus_amd import inst_metrics as im

    true, pred, want = nuclei_1024
    assert want["n_true"] > 1500 and want["tp"] > 500 and want["fn"] > 50
    tab = im.pair_table(true, pred)
    assert tab.retries == 0
    s1, f1 = im.summary_device(tab)
    got = im.summary(tab)
    _check(got, want, "1024")
    tab2 = im.pair_table(true, pred)
    s2, f2 = im.summary_device(tab2)
    assert torch.equal(tab.pairs, tab2.pairs) and torch.equal(s1, s2)
    assert f1.cpu().numpy().tobytes() == f2.cpu().numpy().tobytes()  # sum_iou: one fixed order


def test_remap_label_against_the_reference():
    from cerberus_amd import inst_metrics as im

    g = np.load(os.path.join(GOLDEN, "remap_label.npz"))
    for i in range(len(g.files) // 3):
        lab = g["c%d/in" % i]
        for mode, by_size in (("plain", False), ("by_size", True)):
            out = im.remap_label(lab, by_size)
            assert isinstance(out, np.ndarray) and out.dtype == np.int32 and np.array_equal(out, g["c%d/%s" % (i, mode)]), (i, mode)
    dev = im.remap_label(torch.from_numpy(g["c0/in"]).cuda(), True)
    assert dev.is_cuda and dev.dtype == torch.int32 and np.array_equal(dev.cpu().numpy(), g["c0/by_size"])
    empty = im.remap_label(np.zeros((5, 7), np.int64))
    assert empty.dtype == np.int32 and empty.shape == (5, 7) and not empty.any()


def test_per_class_pq_equals_pq_on_filtered_maps(blobs):
    from cerberus_amd import inst_metrics as im

    true, pred, _ = blobs
    rs = np.random.RandomState(9)
    tt, tp = rs.randint(1, 4, 70001).astype(np.int32), rs.randint(1, 4, 70001).astype(np.int32)
    tab = im.pair_table(true, pred)
    stats = im.InstanceStats(4)
    stats.update(true, pred, tt, tp)
    per = stats.per_image()[0]
    for k in (1, 2, 3):
        tz = np.where(np.isin(true, np.flatnonzero(tt == k)), true, 0).astype(np.int32)
        pz = np.where(np.isin(pred, np.flatnonzero(tp == k)), pred, 0).astype(np.int32)
        a = im.summary(tab, tt, torch.from_numpy(tp), cls=k)
        b = im.summary(im.pair_table(tz, pz))
        want = ref.stats(true, pred, tt, tp, k)
        assert want["tp"] > 0 and want["fp"] > 0 and want["fn"] > 0
        # the integers with ==; sum_iou is added over other positions in the two tables, so each side is held to the bar of the file
        assert [a[x] for x in cases.KEYS] == [b[x] for x in cases.KEYS], (k, a, b)
        _check(a, want, "class %d" % k)
        _check(b, want, "class %d, filtered maps" % k)
        assert per[k]["tp"] == a["tp"] and per[k]["pq"] == a["pq"]
        assert im.panoptic_quality(tab, tt, tp, cls=k)["pq"] == a["pq"]
    assert per["all"] == im.summary(tab)


def test_instance_stats_pools_and_averages(blobs):
    from cerberus_amd import inst_metrics as im

    true, pred, want = blobs
    stats = im.InstanceStats()
    stats.update(true, pred)
    stats.update(CASES[1][1], CASES[1][2])  # 'split'
    w2 = ref.stats(CASES[1][1], CASES[1][2])
    c = stats.counters()["all"]
    for k in cases.KEYS:
        assert c[k] == want[k] + w2[k]
    s = stats.scalars()
    pooled = ref.ratios(dict(c, sum_iou=want["sum_iou"] + w2["sum_iou"]))
    rel = (want["tp"] + w2["tp"]) * 2.0 ** -52
    for k in RATIOS:
        assert abs(s["all-%s" % k] - pooled[k]) <= rel * abs(pooled[k])
        assert abs(s["all-%s-mean" % k] - (want[k] + w2[k]) / 2) <= rel * abs(want[k] + w2[k])
    stats.reset()
    assert stats.images == 0 and stats.counters()["all"]["n_true"] == 0


def test_row_stride_past_2_31_elements():
    """h = 3 rows 2^30 + 64 elements apart: the last row starts past 2^31 elements.  Both maps are views into one uninitialised buffer; only the viewed
    rows are written, and only they may be read (y * row_stride + x in 64 bits, csrc/inst_metrics.hip: im_load4)."""
    from cerberus_amd import inst_metrics as im

    free, _ = torch.cuda.mem_get_info()
    if free < 20 * 2 ** 30:
        pytest.skip("needs 20 GB of free device memory")
    stride, w, shift = 2 ** 30 + 64, 200, 4096
    buf = torch.empty(2 * stride + shift + w, dtype=torch.int32, device="cuda")
    vt = torch.as_strided(buf, (3, w), (stride, 1), 0)
    vp = torch.as_strided(buf, (3, w), (stride, 1), shift)
    true = cases.blob_labels(3, w, 12, 21, 900, rmin=2.0, rmax=6.0)
    pred = cases.blob_labels(3, w, 12, 22, 900, rmin=2.0, rmax=6.0)
    vt.copy_(torch.from_numpy(true))
    vp.copy_(torch.from_numpy(pred))
    tab = im.pair_table(vt, vp)
    _check_table(tab, true, pred)
    _check(im.summary(tab), ref.stats(true, pred), "2^31")
    del tab, vt, vp, buf
    torch.cuda.empty_cache()


def test_tile_instance_stats_equals_its_own_label_maps():
    from cerberus_amd import inst_metrics as im
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.synth_tiles import stain_field
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    model = create_model(**default_model_kwargs())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(3).items()}, strict=True)
    img = np.stack([stain_field(256, 1), np.random.RandomState(2).randint(0, 256, (256, 256, 3)).astype(np.uint8)])
    inst, _ = im.label_maps_device(model, img, ["Nuclei", "Gland"])
    # the annotation: the model's own instances moved by one pixel (so that there are matches), with a few discs drawn over them
    ann = {}
    for tissue, (n_disc, rmin, rmax) in (("Nuclei", (20, 4.0, 9.0)), ("Gland", (3, 20.0, 50.0))):
        own = [np.roll(m.cpu().numpy(), 1, axis=1) for m in inst[tissue]]
        ann[tissue] = np.stack([np.where(d > 0, d + 100000, o).astype(np.int32)
                                for o, d in zip(own, (cases.blob_labels(256, 256, n_disc, s, 50, rmin, rmax) for s in (31, 32)))])
    stats = im.tile_instance_stats(model, img, ann)
    assert list(stats) == ["Nuclei", "Gland"] and stats["Nuclei"].images == 2
    print("tile stats", {t: {k: s.counters()["all"][k] for k in ("tp", "fp", "fn")} for t, s in stats.items()})
    assert sum(s.counters()["all"]["tp"] for s in stats.values()) > 0
    for tissue in ann:
        per = stats[tissue].per_image()
        for n in range(2):
            assert inst[tissue][n].is_cuda and inst[tissue][n].dtype == torch.int32
            assert per[n]["all"] == im.summary(im.pair_table(ann[tissue][n], inst[tissue][n])), (tissue, n)
            _check(per[n]["all"], ref.stats(ann[tissue][n], inst[tissue][n].cpu().numpy()), "%s %d" % (tissue, n))
    # with annotated classes: per-class figures from the majority classes on both sides
    ann_type = {"Nuclei": (ann["Nuclei"] % 3 + 1).astype(np.uint8) * (ann["Nuclei"] > 0)}
    typed = im.tile_instance_stats(model, img[:1], {"Nuclei": ann["Nuclei"][:1]}, ann_type={"Nuclei": ann_type["Nuclei"][:1]})
    per = typed["Nuclei"].per_image()[0]
    assert per["all"] == stats["Nuclei"].per_image()[0]["all"]
    assert sum(per[k]["n_true"] for k in typed["Nuclei"].groups()[1:]) == per["all"]["n_true"]


def test_compute_stats_cli(tmp_path, capsys):
    import json
    import sys

    import scipy.io as sio
    from conftest import ROOT

    sys.path.insert(0, ROOT)
    import compute_stats

    pd, td = tmp_path / "out", tmp_path / "ann"
    (pd / "nuclei_mat").mkdir(parents=True)
    td.mkdir()
    want, maps = {}, {}
    for i, name in enumerate(("a", "b", "c")):
        true = cases.blob_labels(70, 90, 20, 40 + i, 50)
        pred = np.where(cases.blob_labels(70, 90, 20, 40 + i, 50, 2.5, 8.0) > 0, true, 0).astype(np.int32) if i < 2 else cases.blob_labels(70, 90, 20, 50, 50)
        ids = np.unique(pred[pred > 0])
        sio.savemat(str(pd / "nuclei_mat" / (name + ".mat")), {"inst_map": pred, "id": ids, "type": ids % 2 + 1})
        t_ids = np.unique(true[true > 0])
        if i == 1:
            np.save(str(td / (name + ".npy")), {"inst_map": true, "inst_type": (t_ids % 2 + 1)[:, None]}, allow_pickle=True)
        else:
            sio.savemat(str(td / (name + ".mat")), {"inst_map": true, "inst_type": (t_ids % 2 + 1)[:, None]})
        want[name], maps[name] = ref.stats(true, pred), (true, pred)
    res = compute_stats.main(["--pred_dir=%s" % pd, "--true_dir=%s" % td, "--tissue=nuclei", "--types=3", "--gpu="])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    assert json.loads(line)["images"] == 3
    assert [r["name"] for r in res["per_image"]] == ["a", "b", "c"]
    types = np.arange(51) % 2 + 1
    for r in res["per_image"]:
        w = want[r["name"]]
        rel = w["tp"] * 2.0 ** -52
        for k in RATIOS:
            assert abs(r[k] - w[k]) <= rel * abs(w[k]), (r["name"], k)
        for k in (1, 2):
            wk = ref.stats(maps[r["name"]][0], maps[r["name"]][1], types, types, k)
            assert abs(r["pq_class%d" % k] - wk["pq"]) <= wk["tp"] * 2.0 ** -52 * wk["pq"]
    for k in cases.KEYS:
        assert res["counters"][k] == sum(w[k] for w in want.values())
    rows = open(str(pd / "stats.csv")).read().strip().splitlines()
    assert rows[0].startswith("name,dq,sq,pq,aji,dice2,dice1,pq_class1,pq_class2") and len(rows) == 5 and rows[-1].startswith("pooled,")
