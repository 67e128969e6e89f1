"""The polygon fill's restatement (tests/poly_fill_ref.py) against closed forms, against an independent crossing count in exact rationals, and on the
round trip label map -> outer contour (oracle.cv2_standin) -> filled set; the annotation loaders of cerberus_amd/rasterize.py on files written here;
the new options of compute_stats.py and compute_features.py.  No GPU."""
import json
import math
import pickle
import sys

import numpy as np
import pytest

import poly_fill_ref as ref
from conftest import ROOT


def _filled(h, w, pts, **kw):
    prio = np.zeros((h, w), np.uint32)
    ref.fill_contour(prio, np.asarray(pts, np.int64), 1, **kw)
    return prio != 0


@pytest.mark.parametrize("a,b", [(1, 1), (5, 3), (12, 7), (1, 9)])
def test_axis_aligned_rectangle(a, b):
    for order in (1, -1):  # either orientation
        rect = [(3, 2), (3 + a, 2), (3 + a, 2 + b), (3, 2 + b)][::order]
        got = _filled(16, 24, rect)
        assert int(got.sum()) == (a + 1) * (b + 1) and got[2:3 + b, 3:4 + a].all()
        inner = _filled(16, 24, rect, interior_only=True)  # rows and columns are half-open: the interior alone is a x b
        assert int(inner.sum()) == a * b and inner[2:2 + b, 3:3 + a].all()


@pytest.mark.parametrize("n", [1, 2, 7, 20])
def test_right_triangle(n):
    got = _filled(n + 3, n + 3, [(0, 0), (n, 0), (0, n)])
    assert int(got.sum()) == (n + 1) * (n + 2) // 2
    ys, xs = np.nonzero(got)
    assert (xs + ys <= n).all()


def test_bow_tie_and_pentagram_follow_even_odd():
    bow = [(0, 0), (10, 10), (10, 0), (0, 10)]
    got = _filled(11, 11, bow)
    assert got[5, 1] and got[5, 9] and not got[1, 5] and not got[9, 5] and got[5, 5]  # left and right triangles; the crossing is on the outline
    star = [(50 + round(40 * math.sin(math.radians(144 * k))), 50 - round(40 * math.cos(math.radians(144 * k)))) for k in range(5)]
    got = _filled(100, 100, star)
    centre = ref.crossings_int(50, 50, star)
    assert centre > 0 and centre % 2 == 0 and not got[50, 50]  # wound twice: outside by even-odd
    for k in range(5):  # the five tips, three quarters of the way out
        x, y = 50 + round(30 * math.sin(math.radians(144 * k))), 50 - round(30 * math.cos(math.radians(144 * k)))
        assert got[y, x] and ref.crossings_int(x, y, star) % 2 == 1
    assert np.array_equal(ref.interior_np(100, 100, star), ref.interior_int(100, 100, star))


def test_restatement_equals_the_crossing_count_in_rationals_on_random_polygons():
    rs = np.random.RandomState(3)
    h, w = 21, 26
    for case in range(40):
        k = int(rs.randint(3, 10))
        pts = rs.randint(-6, [w + 6, h + 6], (k, 2)).astype(np.int64)
        if case % 5 == 0:
            pts[1] = pts[0]  # a repeated point
        if case % 7 == 0:
            pts[:, 1] = pts[:, 1] // 4 * 4  # vertices sharing rows: horizontal edges, vertices on the same pixel row
        assert np.array_equal(ref.interior_np(h, w, pts), ref.interior_int(h, w, pts)), case
    # fewer than three points: no interior; the filled set is the stroke
    assert not ref.interior_np(9, 9, [(1, 1), (7, 7)]).any() and int(_filled(9, 9, [(1, 1), (7, 7)]).sum()) == 7
    assert int(_filled(9, 9, [(4, 4)]).sum()) == 1
    # collinear points: an empty interior
    assert not ref.interior_np(20, 20, [(1, 1), (5, 3), (9, 5), (13, 7)]).any()


def test_a_vertex_on_a_pixel_row_counts_once_and_the_skip_rule_is_the_stamps():
    diamond = [(10, 2), (18, 10), (10, 18), (2, 10)]
    got = ref.interior_np(21, 21, diamond)
    assert got[10, 2:18].all() and not got[10, 18] and not got[18].any() and not got[2].any()
    assert int(_filled(21, 21, diamond).sum()) == 2 * 8 * 8 + 2 * 8 + 1  # the lattice points of |x - 10| + |y - 10| <= 8
    m = 1 << 20
    prio = np.zeros((40, 40), np.uint32)
    pts = np.array([[5, 5], [30, 8], [m, 30], [5, 20], [30, 22], [m + 1, 30]], np.int64)
    ref.fill_group(prio, pts, [0, 3], [3, 3])
    assert set(np.unique(prio).tolist()) == {0, 1}  # the contour one beyond the range painted nothing
    assert np.array_equal(ref.labels(prio, [7, 9], -1), np.where(prio == 1, 7, -1))


@pytest.fixture(scope="module")
def components():
    """hole-free 8-connected components of random 24 x 24 masks: [(mask of the component alone, x0, y0 of its first pixel in raster order)]"""
    from scipy import ndimage

    rs = np.random.RandomState(11)
    out = []
    for _ in range(60):
        mask = ndimage.binary_fill_holes(rs.rand(24, 24) < rs.uniform(0.3, 0.6))  # the background is then 4-connected to the outside
        lab, n = ndimage.label(mask, structure=np.ones((3, 3), int))  # 8-connected pieces
        for i in range(1, n + 1):
            comp = lab == i
            y0 = int(np.nonzero(comp.any(1))[0][0])
            out.append((comp, int(np.nonzero(comp[y0])[0][0]), y0))
    return out


@pytest.mark.parametrize("method", ["simple", "none"])
def test_round_trip_of_outer_contours(components, method):
    """The filled set of the outer contour of an 8-connected, hole-free instance is the instance: every component, none skipped, no mismatch."""
    from oracle import cv2_standin as cv

    assert len(components) >= 200
    m = cv.CHAIN_APPROX_SIMPLE if method == "simple" else cv.CHAIN_APPROX_NONE
    wrong = 0
    for comp, x0, y0 in components:
        pts = np.asarray(cv._trace_outer(comp.astype(np.uint8), x0, y0, m), np.int64).reshape(-1, 2)
        wrong += int((_filled(24, 24, pts) != comp).sum() != 0)
    assert wrong == 0


def test_fill_windows_keep_the_plane_under_a_gibibyte():
    from cerberus_amd.rasterize import fill_windows

    assert fill_windows(700, 900) == [(0, 0, 900, 700)] and fill_windows(32768, 32768) == [(0, 0, 32768, 32768)]
    for h, w in ((40000, 40000), (1000, 100000), (70000, 5)):
        wins = fill_windows(h, w)
        assert len(wins) > 1 and all(4 * (x1 - x0) * (y1 - y0) < (1 << 30) and max(x1 - x0, y1 - y0) <= 32768 for x0, y0, x1, y1 in wins)
        cover = sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1 in wins)
        assert cover == h * w and wins[0][:2] == (0, 0) and wins[-1][2:] == (w, h)
    assert fill_windows(96, 128, (32, 64)) == [(x, y, x + 64, y + 32) for y in (0, 32, 64) for x in (0, 64)]
    with pytest.raises(ValueError, match="window"):
        fill_windows(10, 10, (0, 4))


def test_annotation_loaders(tmp_path):
    from cerberus_amd.rasterize import dict_group, dict_tissues, load_annotations

    sq = np.array([[2, 2], [9, 2], [9, 8], [2, 8]], np.int32)
    tri = np.array([[12, 3], [18, 3], [12, 9]], np.int32)
    dat = {"Nuclei": {"ab": {"contour": sq, "type": 3, "box": np.zeros(4)}, "cd": {"contour": tri, "type": 1}}, "Gland": {},
           "proc_resolution": {"resolution": 0.5, "units": "mpp"}, "proc_dimensions": np.array([30, 40])}
    p = tmp_path / "s.dat"
    with open(str(p), "wb") as fh:
        pickle.dump(dat, fh, protocol=4)
    got, holes = load_annotations(str(p))
    assert holes == 0 and dict_tissues(got) == ["Nuclei", "Gland"] and np.array_equal(got["Nuclei"]["cd"]["contour"], tri)
    group, types = dict_group(got["Nuclei"])
    assert group["ids"].tolist() == [1, 2] and group["counts"].tolist() == [4, 3] and group["offsets"].tolist() == [0, 4] and types.tolist() == [0, 3, 1]
    assert dict_group(got["Gland"])[1] is None and len(dict_group(got["Gland"])[0]["counts"]) == 0
    # the reference's save_json layout
    p = tmp_path / "s.json"
    p.write_text(json.dumps({"mag": 40, "instances": {"Nuclei": {"7": {"box": [1, 2, 3, 4], "contour": sq.tolist(), "type": 2}, "9": {"contour": tri.tolist(), "type": None}}}}))
    got, holes = load_annotations(str(p))
    assert holes == 0 and got["mag"] == 40 and dict_tissues(got) == ["Nuclei"] and list(got["Nuclei"]) == ["7", "9"]
    assert np.array_equal(got["Nuclei"]["7"]["contour"], sq) and got["Nuclei"]["7"]["type"] == 2 and "type" not in got["Nuclei"]["9"]
    # GeoJSON: closing duplicates dropped, a hole dropped and counted, a MultiPolygon under one id, the tissue from the classification or the caller
    def ring(a):
        return [[float(x) + 0.2, float(y) - 0.3] for x, y in a] + [[float(a[0][0]) + 0.2, float(a[0][1]) - 0.3]]

    hole = [[4, 4], [6, 4], [6, 6]]
    feats = [{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [ring(sq), ring(hole)]}, "properties": {"classification": {"name": "Gland"}}},
             {"type": "Feature", "geometry": {"type": "MultiPolygon", "coordinates": [[ring(tri)], [ring(sq + 20), ring(hole)]]}, "properties": {}},
             {"type": "Feature", "id": "q1", "geometry": {"type": "Polygon", "coordinates": [ring(tri + 5)]}}]
    p = tmp_path / "s.geojson"
    p.write_text(json.dumps({"type": "FeatureCollection", "features": feats}))
    got, holes = load_annotations(str(p), tissue="Nuclei")
    assert holes == 2 and dict_tissues(got) == ["Gland", "Nuclei"] and list(got["Nuclei"]) == [1, "q1"]
    assert np.array_equal(got["Gland"][1]["contour"], sq) and got["Gland"][1]["contour"].dtype == np.int64  # rounded, the closing point gone
    multi = got["Nuclei"][1]
    assert np.array_equal(multi["contour"], tri) and len(multi["more_contours"]) == 1 and np.array_equal(multi["more_contours"][0], sq + 20)
    group, types = dict_group(got["Nuclei"])
    assert group["ids"].tolist() == [1, 1, 2] and group["counts"].tolist() == [3, 4, 3] and types is None
    with pytest.raises(ValueError, match="name the tissue"):
        load_annotations(str(p))
    # everything else is refused by name
    p.write_text(json.dumps({"type": "FeatureCollection", "features": [{"type": "Feature", "geometry": {"type": "LineString", "coordinates": [[0, 0], [1, 1]]}}]}))
    with pytest.raises(ValueError, match="LineString"):
        load_annotations(str(p), tissue="Nuclei")
    p.write_text(json.dumps({"type": "Feature", "geometry": None}))
    with pytest.raises(ValueError, match="FeatureCollection"):
        load_annotations(str(p), tissue="Nuclei")
    (tmp_path / "s.xml").write_text("<a/>")
    with pytest.raises(ValueError, match=r"\.xml"):
        load_annotations(str(tmp_path / "s.xml"))
    (tmp_path / "t.json").write_text(json.dumps([1, 2]))
    with pytest.raises(ValueError, match="instances"):
        load_annotations(str(tmp_path / "t.json"))


def test_new_options_and_their_exclusions(tmp_path, capsys):
    sys.path.insert(0, ROOT)
    import compute_features
    import compute_stats
    from cerberus_amd.cli import FEATURES_OPTIONS, STATS_OPTIONS, parse

    a = parse("compute_stats.py", STATS_OPTIONS, ["--pred_dat=s.dat", "--true_ann", "t.geojson", "--tissue=gland"])
    assert a["--pred_dat"] == "s.dat" and a["--true_ann"] == "t.geojson" and a["--pred_dir"] is None and a["--tissue"] == "gland" and a["--types"] is None
    assert [o[0] for o in STATS_OPTIONS][:5] == ["--gpu", "--pred_dir", "--true_dir", "--tissue", "--types"]  # appended, nothing moved
    with pytest.raises(SystemExit) as e:
        compute_stats.main(["--help"])
    out = capsys.readouterr().out
    assert e.value.code == 0 and "--pred_dat" in out and "--true_ann" in out
    for argv, msg in ((["--pred_dat=a.dat", "--true_ann=b.dat", "--pred_dir=x"], "do not go with"), (["--pred_dat=a.dat", "--true_ann=b.dat", "--true_dir=x"], "do not go with"),
                      (["--pred_dat=a.dat"], "together"), (["--true_ann=b.dat"], "together"), (["--pred_dat=a.dat", "--true_ann=b.dat", "--types=1"], "at least 2"),
                      (["--pred_dat=%s" % (tmp_path / "no.dat"), "--true_ann=%s" % (tmp_path / "no.json")], "no such file")):
        with pytest.raises(SystemExit) as e:
            compute_stats.main(argv)
        assert msg in str(e.value.code), (argv, e.value.code)
    (tmp_path / "a.dat").write_bytes(b"")
    (tmp_path / "b.txt").write_bytes(b"")
    with pytest.raises(SystemExit) as e:
        compute_stats.main(["--pred_dat=%s" % (tmp_path / "a.dat"), "--true_ann=%s" % (tmp_path / "b.txt")])
    assert ".geojson" in str(e.value.code)
    a = parse("compute_features.py", FEATURES_OPTIONS, ["--dat=s.dat", "--knn", "2"])
    assert a["--dat"] == "s.dat" and a["--knn"] == "2" and a["--npz"] is None and [o[0] for o in FEATURES_OPTIONS][:4] == ["--gpu", "--pred_dir", "--npz", "--knn"]
    for argv, msg in ((["--dat=a", "--npz=b"], "exactly one"), (["--dat=a", "--pred_dir=b"], "exactly one"), (["--dat=%s" % (tmp_path / "none.dat")], "no such file")):
        with pytest.raises(SystemExit) as e:
            compute_features.main(argv)
        assert msg in str(e.value.code), (argv, e.value.code)
