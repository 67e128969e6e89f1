"""The restatement tests/inst_features_ref.py held against closed forms and scipy, the derived formulas of cerberus_amd.inst_features against an
evaluation in fractions.Fraction, and the argument refusals of compute_features.py.  No GPU."""
import functools
import math
import sys

import numpy as np
import pytest

import inst_features_cases as cases
import inst_features_ref as ref
from conftest import ROOT


@functools.lru_cache(maxsize=None)
def _all_rows():
    """{case: (map, n_inst, table rows, shape rows, hulls)} computed once"""
    out = {}
    for name, m, n in cases.shape_cases():
        rows, hulls = ref.shape_rows(m, n)
        out[name] = (m, n, ref.inst_table(m, n), rows, hulls)
    return out


@pytest.mark.parametrize("a,b", [(1, 1), (1, 7), (6, 1), (2, 2), (5, 3), (70, 4), (3, 9)])
def test_rectangle_closed_forms(a, b):
    """an a x b rectangle (a wide, b tall) away from the map's border"""
    m = np.zeros((b + 3, a + 4), np.int32)
    m[1:1 + b, 2:2 + a] = 1
    rows, hulls = ref.shape_rows(m, 1)
    m20, m02, m11, crack, border, area2, npts, nrows = rows[0]
    assert m20 == b * sum(i * i for i in range(a))
    assert m02 == a * sum(i * i for i in range(b))
    assert m11 == (a * (a - 1) // 2) * (b * (b - 1) // 2)
    assert crack == 2 * (a + b)
    assert border == a * b - max(a - 2, 0) * max(b - 2, 0)
    assert area2 == 2 * (a - 1) * (b - 1)
    assert npts == (1 if a == b == 1 else 2 if min(a, b) == 1 else 4) and nrows == b
    assert hulls[0][0] == (2, 1)  # the top-left vertex first
    ex = ref.derived_exact(ref.inst_table(m, 1)[0], rows[0])
    assert ex["solidity"] == 1.0 and ex["extent"] == 1.0 and ex["hull_area"] == a * b


def test_hull_order_is_counter_clockwise_on_the_screen():
    m = np.zeros((6, 6), np.int32)
    m[1:4, 1:5] = 1
    _, hulls = ref.shape_rows(m, 1)
    assert hulls[0] == [(1, 1), (1, 3), (4, 3), (4, 1)]  # top-left, down the left side, along the bottom, up the right side


def test_hull_area_against_scipy():
    from scipy.spatial import ConvexHull

    checked = 0
    for name, (m, n, tab, rows, hulls) in _all_rows().items():
        for i in range(n):
            if rows[i][6] < 3:
                assert rows[i][5] == 0, name  # a point or a line
                continue
            ys, xs = np.nonzero(m == i + 1)
            hull = ConvexHull(np.stack([xs, ys], 1).astype(np.float64))
            assert rows[i][5] == int(round(2 * hull.volume)), (name, i + 1)  # (in 2-D `volume` is the area)
            assert rows[i][6] == len(hull.vertices), (name, i + 1)
            assert sorted(hulls[i]) == sorted((int(xs[v]), int(ys[v])) for v in hull.vertices), (name, i + 1)
            checked += 1
    assert checked >= 20


def test_named_hull_cases():
    r = _all_rows()
    assert r["single_pixel"][3][0][5:8] == [0, 1, 1]
    assert r["horizontal_line"][3][0][5:8] == [0, 2, 1]
    assert r["vertical_line"][3][0][5:8] == [0, 2, 25]
    assert [row[5:7] for row in r["diagonal_lines"][3]] == [[0, 2], [0, 2], [0, 2]]
    assert r["two_pieces"][3][0][7] == 7 and r["two_pieces"][1] == 2
    assert r["ring"][3][0][5] == 2 * 8 * 10 and r["ring"][3][0][6] == 4


def test_knn_against_ckdtree():
    from scipy.spatial import cKDTree

    for name, pts in cases.point_cases():
        n = len(pts)
        tree = cKDTree(pts.astype(np.float64))
        small = int(np.abs(pts).max()) < 2 ** 20
        for k in range(1, 9):
            idx, d2 = ref.knn(pts, k)
            dist, _ = tree.query(pts.astype(np.float64), k=k + 1)
            dist = np.asarray(dist).reshape(n, k + 1)[:, 1:]  # (the point itself, or a duplicate of it, comes first at distance 0)
            for i in range(n):
                for j in range(k):
                    if d2[i][j] < 0:
                        assert idx[i][j] == -1 and j >= n - 1 and np.isinf(dist[i, j]), (name, k, i, j)
                        continue
                    assert idx[i][j] not in (i, -1) and idx[i][j] not in idx[i][:j]
                    # the tie rule: ascending by (d2, index)
                    assert j == 0 or (d2[i][j - 1], idx[i][j - 1]) < (d2[i][j], idx[i][j])
                    assert d2[i][j] == sum((int(a) - int(b)) ** 2 for a, b in zip(pts[i], pts[idx[i][j]]))
                    if small:  # d2 < 2^42 and dist * dist carries a relative error below 2^-51: the nearest integer is d2 itself
                        assert int(np.rint(dist[i, j] * dist[i, j])) == d2[i][j], (name, k, i, j)
                    else:
                        assert abs(dist[i, j] - math.sqrt(d2[i][j])) <= 4e-16 * dist[i, j], (name, k, i, j)


def test_relation_restatement_on_the_named_cases():
    by_name = {c[0]: c for c in cases.relation_cases()}
    _, child, n_child, types, parent, n_parent, shift = by_name["c_shape"]
    tab = ref.inst_table(child, n_child)
    assert child[tab[0][2] // tab[0][0], tab[0][1] // tab[0][0]] == 0  # the centroid lies in the hollow
    assert ref.relate(tab, types, parent, shift, n_parent) == ([0], [[0] * 10])
    _, child, n_child, types, parent, n_parent, shift = by_name["shift1_outside"]
    tab = ref.inst_table(child, n_child)
    po, rows = ref.relate(tab, types, parent, shift, n_parent)
    assert po[n_child - 1] == 0 and tab[n_child - 1][0] == 1 and sum(po) == rows[0][0] > 0
    assert sum(rows[0][2:]) == rows[0][0]
    _, child, n_child, types, parent, n_parent, shift = by_name["shift1_ceil"]
    po, rows = ref.relate(ref.inst_table(child, n_child), types, parent, shift, n_parent)
    assert po[n_child - 1] == int(parent[20, 18]) or not 1 <= parent[20, 18] <= n_parent
    _, child, n_child, types, parent, n_parent, shift = by_name["parent_ids_out_of_range"]
    po, _ = ref.relate(ref.inst_table(child, n_child), types, parent, shift, n_parent)
    assert max(po) <= n_parent and min(po) >= 0 and (parent > n_parent).any() and (parent < 0).any()


def _deviation():
    """(largest relative deviation of cerberus_amd.inst_features.derived_formulas in numpy float64 from the Fraction evaluation, per column;
    the (case, id) pairs excluded from eccentricity / orientation)"""
    from cerberus_amd.inst_features import DERIVED, derived_formulas

    worst = dict((k, 0.0) for k in DERIVED)
    excluded = []
    for name, (m, n, tab, rows, hulls) in _all_rows().items():
        t = np.array(tab, np.float64).reshape(n, 16)
        s = np.array(rows, np.float64).reshape(n, 8)
        with np.errstate(all="ignore"):
            got = derived_formulas(np, t, s)
        for i in range(n):
            if tab[i][0] == 0:
                assert all(np.isnan(got[k][i]) for k in ("mu20", "solidity", "extent", "circularity")), name
                continue
            ex = ref.derived_exact(tab[i], rows[i])
            round_ = ex["_gap"] < 1e-9
            if round_:
                excluded.append((name, i + 1))
            for k in DERIVED:
                if round_ and k in ("eccentricity", "orientation"):
                    continue
                g, e = float(got[k][i]), ex[k]
                assert np.isfinite(g), (name, i + 1, k)
                dev = 0.0 if g == e else abs(g - e) / abs(e) if e != 0 else float("inf")
                worst[k] = max(worst[k], dev)
    return worst, excluded


def test_derived_formulas_against_fractions():
    worst, excluded = _deviation()
    print("largest relative deviation per column:", worst)
    print("excluded from eccentricity / orientation:", excluded)
    rows = _all_rows()
    for name, inst in excluded:  # at most the disc and the squares are (nearly) circular
        t = rows[name][2][inst - 1]
        bw, bh = t[6] - t[5], t[4] - t[3]
        assert name == "disc9" or (bw == bh and t[0] == bw * bh), (name, inst)
    assert max(worst.values()) <= cases.DERIVED_MEASURED, worst
    assert cases.DERIVED_BAR == 16 * cases.DERIVED_MEASURED


def test_shift_for():
    from cerberus_amd.inst_features import shift_for

    assert shift_for((41, 37), (41, 37)) == 0
    assert shift_for((41, 37), (21, 19)) == 1 and shift_for((41, 37), (20, 18)) == 1 and shift_for((40, 36), (20, 18)) == 1
    for bad in ((10, 9), (41, 18), (82, 74), (14, 12)):
        with pytest.raises(ValueError, match="ratio"):
            shift_for((41, 37), bad)


def test_knn_refuses_by_name():
    from cerberus_amd.inst_features import knn

    with pytest.raises(ValueError, match="grid-binned search"):
        knn(np.zeros((2 ** 17 + 1, 2), np.int64), 4)
    for k in (0, 9):
        with pytest.raises(ValueError, match="k must lie"):
            knn(np.zeros((4, 2), np.int64), k)


def test_compute_features_refusals(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import compute_features
    from cerberus_amd.cli import FEATURES_OPTIONS, parse

    a = parse("compute_features.py", FEATURES_OPTIONS, ["--pred_dir=out"])
    assert a["--knn"] == "4" and a["--npz"] is None
    with pytest.raises(SystemExit) as e:
        compute_features.main(["--help"])
    assert e.value.code == 0 and "--npz" in capsys.readouterr().out
    for argv, msg in (([], "exactly one"), (["--pred_dir=a", "--npz=b"], "exactly one"), (["--pred_dir=a", "--knn=x"], "integer"),
                      (["--pred_dir=a", "--knn=9"], "0 .. 8"), (["--pred_dir=%s" % (tmp_path / "none")], "no such directory"),
                      (["--npz=%s" % (tmp_path / "none.npz")], "no such file"), (["--pred_dir=%s" % tmp_path], "no .mat files")):
        with pytest.raises(SystemExit) as e:
            compute_features.main(argv)
        assert msg in str(e.value.code), (argv, e.value.code)
    # maps whose grids do not fit are refused by name, before anything touches a GPU
    p = str(tmp_path / "slide.npz")
    np.savez(p, Nuclei=np.zeros((40, 40), np.int32), Gland=np.zeros((10, 10), np.int32), Lumen=np.zeros((10, 10), np.int32))
    with pytest.raises(SystemExit) as e:
        compute_features.main(["--npz=%s" % p])
    assert "slide" in str(e.value.code) and "ratio" in str(e.value.code)
    np.savez(p, Nuclei=np.zeros((40, 40), np.int32), Gland=np.zeros((20, 20), np.int32), Lumen=np.zeros((40, 40), np.int32))
    with pytest.raises(SystemExit) as e:
        compute_features.main(["--npz=%s" % p])
    assert "differ in shape" in str(e.value.code)
    np.savez(p, pclass=np.zeros((4, 4), np.int32))
    with pytest.raises(SystemExit) as e:
        compute_features.main(["--npz=%s" % p])
    assert "none of the keys" in str(e.value.code)
