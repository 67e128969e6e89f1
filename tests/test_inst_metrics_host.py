"""Instance metrics, host side: the restatement (tests/inst_metrics_ref.py) against hand-computed answers and the reference's remap_label,
argument checks of cerberus_amd.inst_metrics and the command line of compute_stats.py.  No GPU."""
import math
import os

import numpy as np
import pytest
from conftest import ROOT

import inst_metrics_cases as cases
import inst_metrics_ref as ref

CASES = cases.cases()


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_against_hand_computed(case):
    name, true, pred, want, ious = case
    got = ref.stats(true, pred)
    assert tuple(got[k] for k in cases.KEYS) == want, name
    assert got["sum_iou"] == math.fsum(n / d for n, d in ious)
    for k, v in cases.expected_ratios(want, ious).items():
        assert (math.isnan(v) and math.isnan(got[k])) or got[k] == v, (name, k, got[k], v)


def test_half_iou_does_not_match_and_tie_goes_to_the_smaller_id():
    by_name = {c[0]: c for c in CASES}
    _, t, p, _, _ = by_name["half"]
    a, b, c = ref.pairs(t, p)
    assert 2 * c[(1, 1)] == a[1] + b[1] - c[(1, 1)] and ref.stats(t, p)["tp"] == 0
    _, t, p, _, _ = by_name["tie"]
    a, b, c = ref.pairs(t, p)
    assert c[(1, 9)] * (a[1] + b[5] - c[(1, 5)]) == c[(1, 5)] * (a[1] + b[9] - c[(1, 9)])  # equal ratios
    assert np.flatnonzero(p.ravel() == 9)[0] < np.flatnonzero(p.ravel() == 5)[0]  # the larger id comes first in raster order
    assert ref.stats(t, p)["aji_inter"] == 3


def test_restated_class_filter_equals_zeroed_maps():
    t = cases.blob_labels(40, 52, 14, 1, 60)
    p = cases.blob_labels(40, 52, 15, 2, 60)
    rs = np.random.RandomState(3)
    tt, tp = rs.randint(1, 4, 61), rs.randint(1, 4, 61)
    for k in (1, 2, 3):
        tz = np.where(np.isin(t, np.flatnonzero(tt == k)), t, 0)
        pz = np.where(np.isin(p, np.flatnonzero(tp == k)), p, 0)
        a, b = ref.stats(t, p, tt, tp, k), ref.stats(tz, pz)
        assert a == b or all((a[x] == b[x]) or (math.isnan(a[x]) and math.isnan(b[x])) for x in a)


def test_restated_remap_label_against_the_reference(golden_dir):
    g = np.load(os.path.join(golden_dir, "remap_label.npz"))
    n = len(g.files) // 3
    assert n >= 6
    for i in range(n):
        lab = g["c%d/in" % i]
        assert lab.shape[0] <= 64 and lab.shape[1] <= 64
        for mode, by_size in (("plain", False), ("by_size", True)):
            out = ref.remap_label(lab, by_size)
            assert out.dtype == np.int32 and np.array_equal(out, g["c%d/%s" % (i, mode)]), (i, mode)
    assert ref.remap_label(np.zeros((4, 5), np.int64)).dtype == np.int32


def test_argument_checks():
    import torch

    from cerberus_amd import _lib, inst_metrics as im

    with pytest.raises(ValueError, match="assignment solver"):
        im.summary_device(None, match_iou=0.3)
    with pytest.raises(ValueError, match="assignment solver"):
        im.panoptic_quality(None, match_iou=0.49)
    with pytest.raises(ValueError, match="type_true and type_pred"):
        im.summary_device(None, cls=1)
    with pytest.raises(TypeError):
        im._label_map([[1, 2]], "true", torch.device("cpu"))
    with pytest.raises(ValueError, match=r"\[H, W\]"):
        im._label_map(np.zeros((2, 3, 4), np.int32), "true", torch.device("cpu"))
    with pytest.raises(TypeError, match="integers"):
        im._label_map(np.zeros((2, 3), np.float32), "true", torch.device("cpu"))
    r = im.ratios(dict(tp=0, fp=0, fn=0, sum_iou=0.0, aji_inter=0, aji_union=0, dice2_inter=0, dice2_total=0, dice1_inter=0, dice1_total=0))
    assert r["dq"] == 0.0 and r["sq"] == 0.0 and r["pq"] == 0.0 and all(math.isnan(r[k]) for k in ("aji", "dice2", "dice1"))
    if not torch.cuda.is_available():  # no CPU path
        for call in (lambda: im.pair_table(np.zeros((4, 4), np.int32), np.zeros((4, 4), np.int32)), lambda: im.remap_label(np.zeros((4, 4), np.int32)),
                     lambda: im.InstanceStats()):
            with pytest.raises(_lib.CerberusHipError):
                call()


def test_ratios_agree_with_the_restatement():
    from cerberus_amd import inst_metrics as im

    for _, true, pred, _, _ in CASES:
        s = ref.stats(true, pred)
        for k, v in im.ratios(s).items():
            assert (math.isnan(v) and math.isnan(s[k])) or v == s[k]


def test_cli_parsing(tmp_path, capsys):
    import sys

    from cerberus_amd.cli import STATS_OPTIONS, parse

    sys.path.insert(0, ROOT)
    import compute_stats

    a = parse("compute_stats.py", STATS_OPTIONS, ["--pred_dir=out", "--true_dir", "ann", "--types=7"])
    assert a["--pred_dir"] == "out" and a["--true_dir"] == "ann" and a["--types"] == "7" and a["--tissue"] == "nuclei" and a["--gpu"] == "0"
    with pytest.raises(SystemExit) as e:
        compute_stats.main(["--help"])
    assert e.value.code == 0 and "--pred_dir" in capsys.readouterr().out
    with pytest.raises(SystemExit, match="required"):
        compute_stats.main(["--pred_dir=x"])
    # a file on one side only is refused by name, before anything touches a device
    pd, td = tmp_path / "pred", tmp_path / "true"
    (pd / "nuclei_mat").mkdir(parents=True)
    td.mkdir()
    for f in ("a.mat", "b.mat"):
        (pd / "nuclei_mat" / f).write_bytes(b"")
    for f in ("a.npy", "c.mat"):
        (td / f).write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        compute_stats.main(["--pred_dir=%s" % pd, "--true_dir=%s" % td])
    msg = str(e.value)
    assert "b.mat" in msg and "c.mat" in msg and "a.mat" not in msg and "a.npy" not in msg
