"""cerberus_amd.inst_features on the GPU (cerb_inst_shape, cerb_inst_hull_rows, cerb_inst_relate, cerb_points_knn through the Python API and therefore
the C ABI) against the restatement in Python integers (tests/inst_features_ref.py).

Bars: every integer with ==.  The derived float64 columns are not part of the exactness contract: the formulas run in numpy float64 on the
restatement's integers deviate from their evaluation in fractions.Fraction by at most 1.14e-13 relative over every instance of
inst_features_cases.shape_cases() (measured by tests/test_inst_features_host.py, which asserts the figure rounded up to 1.2e-13 =
cases.DERIVED_MEASURED; the worst column is minor_axis of the one-pixel-wide lines, where a + b - d cancels); the device-side torch arithmetic is
allowed 16 x that, cases.DERIVED_BAR = 1.92e-12, for differences in operation order.  Near-circular shapes (l1 - l2 < 1e-9 l1: the disc and the
squares) are excluded from eccentricity and orientation only."""
import csv
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import inst_features_cases as cases
import inst_features_ref as ref
from conftest import ROOT, dev_switches

pytestmark = pytest.mark.gpu

SHAPE_CASES = cases.shape_cases()
_REF = {}


def _want(name, m, n):
    """the restatement of one map, computed once and shared"""
    if name not in _REF:
        rows, hulls = ref.shape_rows(m, n)
        _REF[name] = (ref.inst_table(m, n), rows, hulls)
    return _REF[name]


def _device_table(lab, n):
    from cerberus_amd.postproc import inst_table_device

    return inst_table_device(lab, None, n)


def _check_map(name, m, n, lab=None):
    from cerberus_amd import inst_features as ft

    tab_w, rows_w, hulls_w = _want(name, m, n)
    lab = torch.from_numpy(m).cuda() if lab is None else lab
    table = _device_table(lab, n)
    assert table.cpu().tolist() == tab_w, name
    shape = ft.shape_table(lab, table)
    assert shape.dtype == torch.int64 and shape.is_cuda and tuple(shape.shape) == (n, 8)
    got = shape.cpu().tolist()
    for i in range(n):
        assert got[i] == rows_w[i], (name, i + 1, got[i], rows_w[i])
    counts, offsets, points = ft.hull_points(lab, table)
    assert counts.dtype == torch.int32 and offsets.dtype == torch.int64 and points.dtype == torch.int32
    assert counts.cpu().tolist() == [len(hl) for hl in hulls_w], name
    assert offsets.cpu().tolist() == [sum(len(hl) for hl in hulls_w[:i]) for i in range(n)], name
    assert [tuple(p) for p in points.cpu().tolist()] == [p for hl in hulls_w for p in hl], name
    return table, shape


@pytest.mark.parametrize("case", SHAPE_CASES, ids=[c[0] for c in SHAPE_CASES])
def test_shape_and_hull_cases(case):
    _check_map(*case)


def test_table_computed_inside_and_host_input():
    """table=None: cerb_inst_table runs inside, n = the map's largest id (the id 40 that the stated bound of 17 made background is an instance now);
    a numpy map is accepted"""
    from cerberus_amd import inst_features as ft

    name, m, _ = SHAPE_CASES[0]
    n = int(m.max())
    assert n == 40
    rows_w = _want(name + "/max", m, n)[1]
    assert ft.shape_table(m).cpu().tolist() == rows_w
    assert ft.shape_table(torch.from_numpy(m).cuda()).cpu().tolist() == rows_w


def test_row_strided_view():
    """the map as a window of a larger tensor: a row stride above the width, and a neighbourhood of other ids that must not be read"""
    name, m, n = SHAPE_CASES[0]
    big = torch.full((m.shape[0] + 9, m.shape[1] + 31), 3, dtype=torch.int32, device="cuda")
    view = big[4:4 + m.shape[0], 17:17 + m.shape[1]]
    view.copy_(torch.from_numpy(m))
    assert view.stride(0) == m.shape[1] + 31 and not view.is_contiguous()
    _check_map(name, m, n, lab=view)


def test_fuzz_maps():
    for name, m, n in cases.fuzz_maps():
        _check_map(name, m, n)


@dev_switches
def test_per_pixel_atomics_form_agrees():
    """the developers' library keeps the naive form of cerb_inst_shape (every foreground pixel issuing its own atomics, CERB_INST_SHAPE_PER_PIXEL) as the
    other side of scripts/dev_inst_features_time.py's A/B: the same rows"""
    os.environ["CERB_INST_SHAPE_PER_PIXEL"] = "1"
    try:
        for case in SHAPE_CASES:
            if case[0] in ("blobs70x97", "waves_and_singles", "row1x130"):
                _check_map(*case)
    finally:
        del os.environ["CERB_INST_SHAPE_PER_PIXEL"]


def test_second_call_on_the_same_buffers():
    """the calls clear what they say they clear: shape (cerb_inst_shape), extents (cerb_inst_hull_rows), parent_rows (cerb_inst_relate) -- buffers full
    of other numbers, and a second call without clearing, give the same result"""
    import ctypes as C

    from cerberus_amd import _lib

    name, m, n = SHAPE_CASES[0]
    tab_w, rows_w, _ = _want(name, m, n)
    lab = torch.from_numpy(m).cuda()
    table = _device_table(lab, n)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, w = m.shape
    bh = torch.where(table[:, 0] > 0, table[:, 4] - table[:, 3], torch.zeros_like(table[:, 0]))
    offs = (torch.cumsum(bh, 0) - bh).contiguous()
    total = int(bh.sum())
    shape = torch.full((n, 8), 123456789, dtype=torch.int64, device="cuda")
    ext = torch.full((total, 2), 7, dtype=torch.int32, device="cuda")
    pts = torch.full((2 * total, 2), -5, dtype=torch.int32, device="cuda")
    results = []
    for _ in range(2):
        _lib.check(L.cerb_inst_shape(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), shape.data_ptr(), st))
        _lib.check(L.cerb_inst_hull_rows(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), offs.data_ptr(), ext.data_ptr(), pts.data_ptr(),
                                         shape.data_ptr(), st))
        results.append((shape.cpu().tolist(), pts.cpu().tolist()))
    assert results[0][0] == rows_w and results[1] == results[0]
    # areas only: no point list
    _lib.check(L.cerb_inst_shape(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), shape.data_ptr(), st))
    _lib.check(L.cerb_inst_hull_rows(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), offs.data_ptr(), ext.data_ptr(), None, shape.data_ptr(), st))
    assert shape.cpu().tolist() == rows_w
    _, child, n_child, types, parent, n_parent, shift = cases.relation_cases()[0]
    ctab = _device_table(torch.from_numpy(child).cuda(), n_child)
    plab = torch.from_numpy(parent).cuda()
    ctype = torch.from_numpy(np.asarray(types)).to(torch.int32).cuda()
    parent_of = torch.full((n_child,), 99, dtype=torch.int32, device="cuda")
    prow = torch.full((n_parent, 10), -77, dtype=torch.int64, device="cuda")
    want = ref.relate(ref.inst_table(child, n_child), types, parent, shift, n_parent)
    for _ in range(2):
        _lib.check(L.cerb_inst_relate(ctab.data_ptr(), n_child, ctype.data_ptr(), plab.data_ptr(), plab.stride(0), parent.shape[0], parent.shape[1], shift,
                                      n_parent, parent_of.data_ptr(), prow.data_ptr(), st))
        assert (parent_of.cpu().tolist(), prow.cpu().tolist()) == want


REL_CASES = cases.relation_cases()


@pytest.mark.parametrize("case", REL_CASES, ids=[c[0] for c in REL_CASES])
def test_relate_cases(case):
    from cerberus_amd import inst_features as ft

    name, child, n_child, types, parent, n_parent, shift = case
    ctab = _device_table(torch.from_numpy(child).cuda(), n_child)
    want_of, want_rows = ref.relate(ref.inst_table(child, n_child), types, parent, shift, n_parent)
    parent_of, rows = ft.relate(ctab, parent, n_parent, types, shift)
    assert parent_of.dtype == torch.int32 and rows.dtype == torch.int64 and tuple(rows.shape) == (n_parent, 10)
    assert parent_of.cpu().tolist() == want_of, name
    assert rows.cpu().tolist() == want_rows, name


POINT_CASES = cases.point_cases()


@pytest.mark.parametrize("case", POINT_CASES, ids=[c[0] for c in POINT_CASES])
def test_knn_cases(case):
    from cerberus_amd import inst_features as ft

    name, pts = case
    dev = torch.from_numpy(pts).cuda()
    for k in range(1, 9):
        want_idx, want_d2 = ref.knn(pts, k)
        idx, d2 = ft.knn(dev, k)
        assert idx.dtype == torch.int32 and d2.dtype == torch.int64 and tuple(idx.shape) == (len(pts), k)
        assert idx.cpu().tolist() == want_idx, (name, k)
        assert d2.cpu().tolist() == want_d2, (name, k)


def test_centroids_q4():
    from cerberus_amd import inst_features as ft

    name, m, n = SHAPE_CASES[0]
    table = _device_table(torch.from_numpy(m).cuda(), n)
    assert [tuple(r) for r in ft.centroids_q4(table).cpu().tolist()] == ref.centroids_q4(_want(name, m, n)[0])


def _check_derived(name, tab_w, rows_w, got):
    """got: {column: float64 sequence by row}"""
    from cerberus_amd.inst_features import DERIVED

    worst = 0.0
    for i, (t, s) in enumerate(zip(tab_w, rows_w)):
        if t[0] == 0:
            assert all(math.isnan(got[k][i]) for k in DERIVED), (name, i + 1)
            continue
        ex = ref.derived_exact(t, s)
        for k in DERIVED:
            if ex["_gap"] < 1e-9 and k in ("eccentricity", "orientation"):
                continue
            g, e = float(got[k][i]), ex[k]
            dev = 0.0 if g == e else abs(g - e) / abs(e) if e != 0 else float("inf")
            worst = max(worst, dev)
            assert dev <= cases.DERIVED_BAR, (name, i + 1, k, g, e, dev)
    return worst


def test_derived_columns():
    from cerberus_amd import inst_features as ft

    worst = 0.0
    for name, m, n in SHAPE_CASES:
        tab_w, rows_w, _ = _want(name, m, n)
        lab = torch.from_numpy(m).cuda()
        table = _device_table(lab, n)
        got = ft.derived(table, ft.shape_table(lab, table))
        assert list(got) == list(ft.DERIVED) and all(v.dtype == torch.float64 and v.is_cuda for v in got.values())
        worst = max(worst, _check_derived(name, tab_w, rows_w, {k: v.cpu().tolist() for k, v in got.items()}))
    print("largest relative deviation of the device's derived columns: %r (bar %r)" % (worst, cases.DERIVED_BAR))


def _want_tissue_tables(nuclei, gland, lumen, per_id, shift, k):
    """the integer columns of tissue_features from the restatement: {tissue: {column: list}}"""
    out = {}
    tabs = {}
    for t, m in (("nuclei", nuclei), ("gland", gland), ("lumen", lumen)):
        n = int(m.max())
        tab = ref.inst_table(m, n)
        rows, _ = ref.shape_rows(m, n)
        tabs[t] = tab
        cols = {"id": list(range(1, n + 1)), "area": [r[0] for r in tab], "y1": [r[3] for r in tab], "x1": [r[5] for r in tab],
                "y2": [r[4] for r in tab], "x2": [r[6] for r in tab]}
        for c, nm in enumerate(("m20", "m02", "m11", "crack", "border_px", "hull_area2", "hull_pts", "rows")):
            cols[nm] = [r[c] for r in rows]
        out[t] = cols
        out[t + "/rows"] = rows
    n_g = int(gland.max())
    types = [int(per_id[i + 1]) for i in range(int(nuclei.max()))]
    po, rows = ref.relate(tabs["nuclei"], types, gland, shift, n_g)
    out["nuclei"]["gland_id"] = po
    out["gland"]["n_nuclei"], out["gland"]["nuclei_area"] = [r[0] for r in rows], [r[1] for r in rows]
    for c in range(8):
        out["gland"]["n_nuclei_class%d" % c] = [r[2 + c] for r in rows]
    po, rows = ref.relate(tabs["lumen"], None, gland, 0, n_g)
    out["lumen"]["gland_id"] = po
    out["gland"]["n_lumina"], out["gland"]["lumen_area"] = [r[0] for r in rows], [r[1] for r in rows]
    present = [i for i in range(n_g) if tabs["gland"][i][0] > 0]
    q4 = ref.centroids_q4(tabs["gland"])
    idx, d2 = ref.knn([q4[i] for i in present], k)
    ids = [[-1] * k for _ in range(n_g)]
    dist = [[None] * k for _ in range(n_g)]
    for row, i in enumerate(present):
        ids[i] = [present[j] + 1 if j >= 0 else -1 for j in idx[row]]
        dist[i] = [d if d >= 0 else None for d in d2[row]]
    for j in range(k):
        out["gland"]["knn_id%d" % (j + 1)] = [r[j] for r in ids]
    out["gland/knn_d2"] = dist
    out["tabs"] = tabs
    return out


def _check_tissue_tables(got, want, k):
    """got: {tissue: {column: list}} (from the API or from the CSVs)"""
    for t in ("nuclei", "gland", "lumen"):
        for col, w in want[t].items():
            assert list(got[t][col]) == w, (t, col)
        _check_derived(t, want["tabs"][t], want[t + "/rows"], got[t])
    g = got["gland"]
    for i, a in enumerate(want["gland"]["area"]):
        if a > 0:
            assert g["lumen_fraction"][i] == want["gland"]["lumen_area"][i] / a
        for j in range(k):
            d2 = want["gland/knn_d2"][i][j]
            v = g["knn_dist%d" % (j + 1)][i]
            if d2 is None:
                assert math.isnan(v)
            else:
                assert abs(v - math.sqrt(d2 / 256.0)) <= 2.0 ** -52 * v  # one correctly rounded division and square root on each side


def _host(tables):
    return {t: {c: v.cpu().tolist() for c, v in cols.items()} for t, cols in tables.items()}


def test_tissue_features_end_to_end():
    from cerberus_amd import inst_features as ft

    nuclei, gland, lumen, type_map, per_id = cases.tissue_triple()
    want = _want_tissue_tables(nuclei, gland, lumen, per_id, 0, 3)
    _REF["triple"] = want
    got = ft.tissue_features(nuclei, gland, lumen, nuclei_type=type_map, shift=0, k=3)
    assert list(got) == ["nuclei", "gland", "lumen"]
    assert all(v.is_cuda for cols in got.values() for v in cols.values())
    _check_tissue_tables(_host(got), want, 3)
    assert sum(want["gland"]["n_nuclei"]) > 10 and sum(want["gland"]["n_lumina"]) > 2 and max(want["gland"]["n_nuclei_class3"]) > 0
    # classes as a vector indexed by id: the same tables
    by_id = ft.tissue_features(nuclei, gland, lumen, nuclei_type=torch.from_numpy(per_id.astype(np.int64)), shift=0, k=3)
    assert _host(by_id)["gland"]["n_nuclei_class3"] == want["gland"]["n_nuclei_class3"]
    # a missing tissue is left out, with the columns that need it
    only = ft.tissue_features(None, gland, None, k=1)
    assert list(only) == ["gland"] and "n_nuclei" not in only["gland"] and "knn_id1" in only["gland"]


def _read_csv(path):
    with open(path, newline="") as fh:
        rows = list(csv.reader(fh))
    cols = {}
    for c, name in enumerate(rows[0]):
        vals = [r[c] for r in rows[1:]]
        cols[name] = [float(v) if ("." in v or "n" in v or "e" in v) else int(v) for v in vals]
    return cols


def _run_cli(args):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "compute_features.py")] + args + ["--gpu="], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads(p.stdout.strip().splitlines()[-1])


def _same_tables(from_csv, api):
    for t, cols in api.items():
        assert list(from_csv[t]) == list(cols), t
        for c, v in cols.items():
            w = from_csv[t][c]
            assert len(w) == len(v)
            assert all((a == b) or (isinstance(a, float) and math.isnan(a) and math.isnan(b)) for a, b in zip(w, v)), (t, c)


def test_compute_features_pred_dir(tmp_path):
    import scipy.io as sio

    from cerberus_amd import inst_features as ft

    pd = tmp_path / "out"
    triples = {"a": cases.tissue_triple(), "b": cases.tissue_triple(96, 112, seed=9)}
    for name, (nuclei, gland, lumen, _, per_id) in triples.items():
        for t, m in (("nuclei", nuclei), ("gland", gland.astype(np.float64)), ("lumen", lumen.astype(np.float64))):
            (pd / ("%s_mat" % t)).mkdir(parents=True, exist_ok=True)
            ids = np.unique(m[m > 0]).astype(np.int64)
            sio.savemat(str(pd / ("%s_mat" % t) / (name + ".mat")), {"inst_map": m, "id": ids, "type": per_id[ids] if t == "nuclei" else np.full(ids.size, -1)})
    res = _run_cli(["--pred_dir=%s" % pd, "--knn=3"])
    assert [r["name"] for r in res["images"]] == ["a", "b"] and res["knn"] == 3
    for name, (nuclei, gland, lumen, _, per_id) in triples.items():
        api = _host(ft.tissue_features(nuclei, gland, lumen, nuclei_type=per_id.astype(np.int64), shift=0, k=3))
        got = {t: _read_csv(str(pd / "features" / ("%s_%s.csv" % (name, t)))) for t in ("nuclei", "gland", "lumen")}
        _same_tables(got, api)
        row = [r for r in res["images"] if r["name"] == name][0]
        assert (row["nuclei"], row["gland"], row["lumen"], row["shift"]) == (int(nuclei.max()), int(gland.max()), int(lumen.max()), 0)
    if "triple" in _REF:  # and the CSV of the first triple against the restatement itself
        _check_tissue_tables({t: _read_csv(str(pd / "features" / ("a_%s.csv" % t))) for t in ("nuclei", "gland", "lumen")}, _REF["triple"], 3)


def test_compute_features_npz(tmp_path):
    from cerberus_amd import inst_features as ft

    nuclei, gland, lumen, type_map, per_id = cases.tissue_triple(127, 121, seed=5)
    gland, lumen = np.ascontiguousarray(gland[::2, ::2]), np.ascontiguousarray(lumen[::2, ::2])  # ceil(h / 2) x ceil(w / 2)
    assert gland.shape == (64, 61)
    p = tmp_path / "slide7.npz"
    np.savez_compressed(str(p), **{"Nuclei": nuclei, "Gland": gland, "Lumen": lumen, "type_Nuclei-TYPE": type_map, "pclass": np.zeros((4, 4), np.uint8)})
    res = _run_cli(["--npz=%s" % p])
    assert res["images"][0]["name"] == "slide7" and res["images"][0]["shift"] == 1 and res["knn"] == 4
    api = _host(ft.tissue_features(nuclei, gland, lumen, nuclei_type=type_map, shift=1, k=4))
    got = {t: _read_csv(str(tmp_path / "features" / ("slide7_%s.csv" % t))) for t in ("nuclei", "gland", "lumen")}
    _same_tables(got, api)
    want = _want_tissue_tables(nuclei, gland, lumen, per_id, 1, 4)
    _check_tissue_tables(got, want, 4)
