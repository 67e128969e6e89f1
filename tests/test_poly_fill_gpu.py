"""The polygon fill on the device (csrc/overlay.hip: cerb_overlay_fill / _labels; cerberus_amd/rasterize.py) against the sequential restatement of its
definition (tests/poly_fill_ref.py).  Everything is integer: every comparison is exact equality, there is no tolerance.

Pictures are 200 x 200 at most; each case is the smallest that can break one part of the kernel: the half-open row rule, the exact ceiling, the 64 x 64
cells of a clipped box (63 .. 66 columns and rows, 3 x 3 cells), the edge batches of 64, the helper waves of a call with one large contour, more than
two 64-contour groups, the clip at all four borders and the coordinate range."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

import poly_fill_cases as cases
import poly_fill_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    return torch


def _stream():
    return C.c_void_p(_torch().cuda.current_stream().cuda_stream)


def _plane(h, w, calls, stamp=True, reverse=False):
    """clear + fill (+ stamp of width 1) per call [(points, offsets, counts, first_ordinal, mul, div, origin)] through the C entries -> the plane"""
    torch = _torch()
    from cerberus_amd import _lib

    L = _lib.lib()
    nb = int(L.cerb_overlay_workspace_bytes(h, w))
    ws = torch.full((nb // 4,), -1, dtype=torch.int32, device="cuda")
    st = _stream()
    _lib.check(L.cerb_overlay_clear(ws.data_ptr(), nb, h, w, st))
    keep = []
    for pts, offs, cnts, first, mul, div, org in (calls[::-1] if reverse else calls):
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(pts, np.int32).reshape(-1, 2))).cuda()
        if p.numel() == 0:
            p = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
        o = torch.from_numpy(np.asarray(offs, np.int64)).cuda()
        c = torch.from_numpy(np.asarray(cnts, np.int32)).cuda()
        keep += [p, o, c]
        if stamp and reverse:
            _lib.check(L.cerb_overlay_stamp(p.data_ptr(), o.data_ptr(), c.data_ptr(), len(cnts), mul, div, org[0], org[1], 1, first, ws.data_ptr(), nb, h, w, st))
        _lib.check(L.cerb_overlay_fill(p.data_ptr(), o.data_ptr(), c.data_ptr(), len(cnts), mul, div, org[0], org[1], first, ws.data_ptr(), nb, h, w, st))
        if stamp and not reverse:
            _lib.check(L.cerb_overlay_stamp(p.data_ptr(), o.data_ptr(), c.data_ptr(), len(cnts), mul, div, org[0], org[1], 1, first, ws.data_ptr(), nb, h, w, st))
    return ws.cpu().numpy().view(np.uint32).reshape(h, w)


def _ref_plane(h, w, calls, stamp=True):
    prio = np.zeros((h, w), np.uint32)
    for pts, offs, cnts, first, mul, div, org in calls:
        ref.fill_group(prio, pts, offs, cnts, first, mul, div, org, interior_only=not stamp)
    return prio


def _call(polys, first=0, mul=1, div=1, org=(0, 0)):
    """one call from a list of point lists"""
    cnts = np.array([len(p) for p in polys], np.int64)
    pts = np.concatenate([np.asarray(p, np.int64).reshape(-1, 2) for p in polys]) if len(polys) else np.zeros((0, 2), np.int64)
    return (pts, np.cumsum(cnts) - cnts, cnts, first, mul, div, org)


def _both(h, w, calls):
    """filled set and interior alone, each equal to the restatement -> the filled plane"""
    got, want = _plane(h, w, calls), _ref_plane(h, w, calls)
    assert np.array_equal(got, want), int((got != want).sum())
    inner, want_inner = _plane(h, w, calls, stamp=False), _ref_plane(h, w, calls, stamp=False)
    assert np.array_equal(inner, want_inner), int((inner != want_inner).sum())
    return got


def test_counts_zero_to_three_repeated_and_collinear_points():
    polys = [[], [(5, 5)], [(10, 4), (20, 9)], [(30, 3), (44, 6), (33, 17)],      # 0, 1, 2, 3 points
             [(5, 20), (5, 20), (18, 20), (18, 33), (18, 33), (5, 33)],            # repeated points
             [(25, 22), (31, 25), (37, 28), (43, 31)], [(3, 40), (3, 40), (3, 40)]]  # collinear: the outline only; one point three times
    got = _both(48, 50, [_call(polys)])
    assert not (got == 1).any() and int((got == 2).sum()) == 1 and (got == 3).any() and (got == 4).sum() > 40
    assert int((got == 5).sum()) == 14 * 14 and int((got == 7).sum()) == 1
    inner = _plane(48, 50, [_call(polys)], stamp=False)
    assert set(np.unique(inner).tolist()) == {0, 4, 5}  # only the triangle and the square have an interior


def test_vertices_on_pixel_rows_and_edges_through_lattice_points():
    diamond = [(20, 2), (36, 18), (20, 34), (4, 18)]
    slim = [(50, 1), (60, 21), (40, 41), (46, 19)]            # slopes 2, -1, 11/3 ..: edges through lattice points and between them
    hexa = [(70, 5), (80, 5), (90, 15), (80, 25), (70, 25), (60, 15)]  # horizontal edges, vertices sharing rows
    got = _both(45, 95, [_call([diamond, slim, hexa])])
    assert int((got == 1).sum()) == 2 * 16 * 16 + 2 * 16 + 1  # every lattice point of the diamond, each once


def test_one_pixel_notch_and_a_u_with_a_one_pixel_gap():
    notch = [(2, 2), (10, 2), (10, 6), (11, 6), (11, 2), (20, 2), (20, 12), (2, 12)]  # (a slit one pixel wide: its two walls are outline)
    u = [(30, 2), (34, 2), (34, 14), (36, 14), (36, 2), (40, 2), (40, 18), (30, 18)]    # the gap between the arms is column 35 alone
    got = _both(22, 44, [_call([notch, u])])
    assert (got[2:14, 35] == 0).all() and (got[3:14, 34] == 2).all() and (got[3:14, 36] == 2).all() and (got[15:18, 35] == 2).all()


@pytest.mark.parametrize("side", [63, 64, 65, 66])
def test_clipped_boxes_round_the_cell_size(side):
    """an interior box of `side` columns (rows): 1 or 2 cells across (down), the second one 1 or 2 pixels wide"""
    wide = [(3, 2), (3 + side, 2), (3 + side - 9, 9), (3, 7)]
    tall = [(2, 3), (9, 3 + side - 9), (2, 3 + side), (0, 40)]
    _both(12, side + 8, [_call([wide])])
    _both(side + 8, 12, [_call([tall])])
    # the same boxes cut to that size by the picture's border
    big = [(-20, -30), (150, -10), (170, 160), (60, 90), (-40, 170)]
    _both(side, 40, [_call([big])])
    _both(40, side, [_call([big])])


def test_a_contour_over_three_by_three_cells():
    rs = np.random.RandomState(5)
    ang = np.sort(rs.uniform(0, 2 * np.pi, 70))
    rad = rs.uniform(40, 85, 70)
    star = np.stack([95 + rad * np.cos(ang), 92 + rad * np.sin(ang)], 1).round().astype(np.int64)  # 70 edges: two batches
    got = _both(190, 200, [_call([star])])
    ys, xs = np.nonzero(got)
    assert xs.max() - xs.min() > 128 and ys.max() - ys.min() > 128


def test_a_five_thousand_point_ring_as_the_only_contour():
    """one contour, one group: the call's 64 waves share the 4 x 4 cells of its clipped box, each walking 79 batches of edges"""
    t = np.arange(5000) * (2 * np.pi / 5000)
    r = 150 + 6 * np.sin(9 * t)
    ring = np.stack([120 + r * np.cos(t), 90 + r * np.sin(t)], 1).round().astype(np.int64)  # about 300 px across, mostly repeated points
    got = _both(200, 200, [_call([ring])])
    assert got[90, 120] == 1 and (got == 0).any()


def test_a_hundred_and_thirty_tiny_contours():
    rs = np.random.RandomState(6)
    polys = [(rs.randint(0, [90, 70]) + rs.randint(-4, 5, (int(rs.randint(3, 7)), 2))) for _ in range(130)]
    got = _both(70, 90, [_call(polys)])
    assert got.max() > 128 and len(np.unique(got)) > 100


def test_borders_outside_and_the_coordinate_range():
    h, w = 40, 50
    across = [[(-10, 10), (15, 5), (12, 30)], [(40, 8), (70, 20), (38, 33)], [(20, -9), (33, 12), (8, 14)], [(22, 30), (35, 55), (5, 47)],
              [(-30, -30), (-5, -8), (-20, 4)], [(60, 5), (80, 9), (70, 30)], [(5, 50), (30, 45), (20, 90)], [(-50, -50), (120, -40), (100, 130), (-60, 90)]]
    for poly in across:
        _both(h, w, [_call([poly])])
    _both(h, w, [_call(across)])
    m = 1 << 20
    kept, beyond = [(5, 5), (30, 8), (m, 30)], [(5, 20), (30, 22), (m + 1, 30)]
    neg_kept, neg_beyond = [(8, 30), (-m, 3), (20, 33)], [(8, 36), (-m - 1, 3), (20, 39)]
    tall = [(10, -m), (40, 20), (12, m)]
    got = _both(h, w, [_call([kept, beyond, neg_kept, neg_beyond, tall])])
    assert set(np.unique(got).tolist()) == {0, 1, 3, 5}  # a vertex at exactly +-2^20 is kept; one beyond skips the contour, interior and outline


@pytest.mark.parametrize("mul,div", [(2, 1), (1, 2), (1, 3), (2, 3)])
def test_point_transform_truncates_toward_zero(mul, div):
    rs = np.random.RandomState(7)
    h, w = 60, 70
    polys = [(rs.randint(-10, [w + 10, h + 10]) + rs.randint(-12, 13, (int(rs.randint(3, 9)), 2))) * div // mul + rs.randint(0, div, 2) for _ in range(40)]
    org = (4 * div + 1, 6 * div + 2)  # q = p mul - org is negative near the top-left corner
    call = _call(polys, 0, mul, div, org)
    t = call[0] * mul - np.asarray(org)
    assert (t < 0).any() and (div == 1 or ((t < 0) & (t % div != 0)).any())  # truncation differs from floor there
    got = _both(h, w, [call])
    assert len(np.unique(got)) > 20


def test_windows_through_the_origin_equal_the_map_filled_at_once():
    torch = _torch()
    from cerberus_amd.rasterize import fill_contours_device

    rs = np.random.RandomState(8)
    h, w = 96, 128
    polys = [(rs.randint(0, [w // 2, h // 2]) + rs.randint(-12, 13, (int(rs.randint(3, 8)), 2))) for _ in range(30)]  # (drawn with mul = 2)
    call = _call(polys, 0, 2, 1, (3, 5))
    whole = _both(h, w, [call])
    for y0 in range(0, h, 32):
        for x0 in range(0, w, 64):
            part = _plane(32, 64, [_call(polys, 0, 2, 1, (3 + x0, 5 + y0))])
            assert np.array_equal(part, whole[y0:y0 + 32, x0:x0 + 64]), (x0, y0)
    group = {"points": call[0], "offsets": call[1], "counts": call[2], "mul": 2, "div": 1, "origin": (3, 5)}
    at_once = fill_contours_device((h, w), [group])
    assert at_once.is_cuda and at_once.dtype == torch.int32 and np.array_equal(at_once.cpu().numpy(), whole.astype(np.int32))
    assert np.array_equal(fill_contours_device((h, w), [group], window=(32, 64)).cpu().numpy(), whole.astype(np.int32))
    assert np.array_equal(fill_contours_device((h, w), [group], window=(40, 50)).cpu().numpy(), whole.astype(np.int32))  # windows that end short
    with pytest.raises(ValueError, match="div == 1"):
        fill_contours_device((h, w), [dict(group, div=2)], window=(32, 64))


def test_painters_order_shared_planes_and_shared_table_values():
    torch = _torch()
    from cerberus_amd.rasterize import fill_contours_device

    a, b = [(5, 5), (40, 8), (30, 40), (8, 30)], [(20, 15), (55, 12), (50, 44), (25, 50)]
    ab, ba = _both(60, 64, [_call([a, b])]), _both(60, 64, [_call([b, a])])
    overlap = (ab == 2) & (ba == 2)
    assert overlap.any() and np.array_equal(ab > 0, ba > 0) and not np.array_equal(ab, ba)  # the later contour lies on top, whichever it is
    # two groups sharing a plane through first_ordinal, stamped in either order of execution
    c = [(2, 45), (30, 35), (60, 58)]
    calls = [_call([a], 0), _call([b, c], 1, 2, 2, (0, 0))]
    want = _ref_plane(60, 64, calls)
    assert np.array_equal(_plane(60, 64, calls), want) and np.array_equal(_plane(60, 64, calls, reverse=True), want) and want.max() == 3
    # ids, types and a value shared by two contours (the rings of a MultiPolygon), through the public wrapper and the restatement
    groups = [{"points": _call([a, b])[0], "offsets": [0, 4], "counts": [4, 4], "ids": [7, 7], "types": [2, 5]},
              {"points": np.asarray(c), "offsets": [0], "counts": [3], "ids": [3]}]
    got, cls = fill_contours_device((60, 64), groups, background=-1)
    want, want_cls = ref.fill((60, 64), groups, background=-1)
    assert np.array_equal(got.cpu().numpy(), want) and set(np.unique(want).tolist()) == {-1, 3, 7}
    assert cls.dtype == torch.uint8 and np.array_equal(cls.cpu().numpy(), want_cls) and set(np.unique(want_cls).tolist()) == {0, 2, 5}
    # default ids number on over the groups; device arrays are taken as they are
    dev = [dict(g, points=torch.from_numpy(np.asarray(g["points"], np.int32)).cuda(), counts=torch.tensor(g["counts"], dtype=torch.int32, device="cuda")) for g in groups]
    for g in dev:
        g.pop("ids"), g.pop("types", None)
    plain = fill_contours_device((60, 64), dev)
    assert np.array_equal(plain.cpu().numpy(), ref.fill((60, 64), [{k: v for k, v in g.items() if k not in ("ids", "types")} for g in groups])[0])
    assert set(np.unique(plain.cpu().numpy()).tolist()) == {0, 1, 2, 3}


def test_one_pixel_and_one_row_maps():
    big = [(-5, -5), (300, -4), (290, 9), (-6, 7)]
    assert _both(1, 1, [_call([big])])[0, 0] == 1
    assert _both(1, 1, [_call([[(0, 0), (0, 0), (0, 0)]])])[0, 0] == 1 and not _plane(1, 1, [_call([[(3, 0), (9, 0), (5, 4)]])]).any()
    row = _both(1, 200, [_call([[(10, -3), (150, -2), (140, 5), (70, 1), (20, 6)]])])
    assert row.any() and not row.all()
    col = _both(200, 1, [_call([[(-3, 10), (-2, 150), (5, 140), (1, 70), (6, 20)]])])
    assert col.any() and not col.all()


def test_labels_padded_stride_background_and_refusals():
    torch = _torch()
    from cerberus_amd import _lib

    L = _lib.lib()
    h, w = 16, 24
    nb = 4 * h * w
    st = _stream()
    tri = torch.tensor([[1, 1], [20, 3], [6, 14]], dtype=torch.int32, device="cuda")
    offs, cnts = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 3, dtype=torch.int32, device="cuda")
    table = torch.tensor([41, 9], dtype=torch.int32, device="cuda")
    ws = torch.zeros(h * w, dtype=torch.int32, device="cuda")
    P, O, N, WS, T = tri.data_ptr(), offs.data_ptr(), cnts.data_ptr(), ws.data_ptr(), table.data_ptr()
    _lib.check(L.cerb_overlay_clear(WS, nb, h, w, st))
    _lib.check(L.cerb_overlay_fill(P, O, N, 1, 1, 1, 0, 0, 0, WS, nb, h, w, st))
    _lib.check(L.cerb_overlay_stamp(P, O, N, 1, 1, 1, 0, 0, 1, 0, WS, nb, h, w, st))
    prio = ws.cpu().numpy().view(np.uint32).reshape(h, w).copy()
    assert np.array_equal(prio, _ref_plane(h, w, [_call([tri.cpu().numpy()])])) and prio.any()
    # a padded destination: the bytes between rows stay as they were; a non-zero background; a plane entry beyond the table is background
    stride = 4 * w + 12
    dst = torch.full((h, stride), 0x5A, dtype=torch.uint8, device="cuda")
    _lib.check(L.cerb_overlay_labels(T, 2, -7, WS, nb, dst.data_ptr(), stride, h, w, st))
    out = dst.cpu().numpy()
    assert (out[:, 4 * w:] == 0x5A).all()
    assert np.array_equal(np.ascontiguousarray(out[:, :4 * w]).view(np.int32), ref.labels(prio, [41, 9], -7))
    _lib.check(L.cerb_overlay_labels(None, 0, 5, WS, nb, dst.data_ptr(), stride, h, w, st))
    assert (np.ascontiguousarray(dst.cpu().numpy()[:, :4 * w]).view(np.int32) == 5).all()
    # every refusal: an error, no launch, nothing written
    ws.fill_(0x01020304)
    dst.fill_(0x77)
    D = dst.data_ptr()

    def fill(points=P, offsets=O, counts=N, n=1, mul=1, div=1, first=0, wsp=WS, wsb=nb, hh=h, ww=w, ox=0):
        return L.cerb_overlay_fill(points, offsets, counts, n, mul, div, ox, 0, first, wsp, wsb, hh, ww, st)

    def labels(tp=T, n=2, wsp=WS, wsb=nb, dp=D, ds=stride, hh=h, ww=w):
        return L.cerb_overlay_labels(tp, n, 0, wsp, wsb, dp, ds, hh, ww, st)

    bad = [fill(points=None), fill(offsets=None), fill(counts=None), fill(wsp=None), fill(wsp=WS + 2), fill(n=-1), fill(mul=0), fill(mul=17), fill(div=0),
           fill(div=4097), fill(wsb=nb - 1), fill(hh=32769, wsb=1 << 40), fill(ww=0), fill(first=-1), fill(first=(1 << 32) - 2), fill(n=(1 << 32) - 1),
           fill(ox=(1 << 40) + 1),
           labels(tp=None), labels(wsp=None), labels(dp=None), labels(dp=D + 2), labels(wsp=WS + 1), labels(n=-1), labels(n=(1 << 32) - 1), labels(wsb=nb - 1),
           labels(ds=4 * w - 4), labels(ds=4 * w + 2), labels(hh=32769, wsb=1 << 40), labels(ww=0)]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert L.cerb_last_error().startswith(b"cerb_overlay_labels")
    torch.cuda.synchronize()
    assert (ws.cpu().numpy() == 0x01020304).all() and (dst.cpu().numpy() == 0x77).all()
    assert fill() == 0 and fill(n=0) == 0 and labels() == 0 and labels(tp=None, n=0) == 0 and L.cerb_version() >= 4


@pytest.fixture(scope="module")
def nuclei_parts():
    """the engineered nuclei map on the device, its class map, and its instance arrays (cerb_inst_table, cerb_inst_contour_*) as one part"""
    torch = _torch()
    from cerberus_amd.postproc import inst_contours_device, inst_table_device

    lab, n = cases.nuclei_map()
    assert n == 42 and cases.is_round_trip_map(lab, n) and cases.touching_pairs(lab) > 10
    types = cases.slide_triple()[3]
    dev = torch.from_numpy(lab).cuda()
    tab = inst_table_device(dev, torch.from_numpy(types).cuda())
    cnts, pts, offs = inst_contours_device(dev, tab)
    assert len(cnts) == n and (cnts >= 3).all()
    return lab, types, ("Nuclei", tab.cpu().numpy(), cnts, pts, offs, True, 1.0)


def test_round_trip_on_the_device(nuclei_parts):
    """label map -> cerb_inst_table / cerb_inst_contour_* -> fill: the map itself, ids included -- at full resolution, and stored at half resolution
    (the slide driver's gland and lumen parts: mul = 2 on the way in, div = 2 on the way out)"""
    from cerberus_amd.inst_info import majority_type
    from cerberus_amd.rasterize import fill_contours_device, label_maps_from_parts

    lab, types, part = nuclei_parts
    _, tab, cnts, pts, offs = part[:5]
    got = fill_contours_device(lab.shape, [{"points": pts, "offsets": offs, "counts": cnts}])
    assert np.array_equal(got.cpu().numpy(), lab)
    maps = label_maps_from_parts([part], None, lab.shape)
    assert list(maps) == ["Nuclei"] and np.array_equal(maps["Nuclei"][0].cpu().numpy(), lab)
    want_cls = np.concatenate([[0], majority_type(tab)]).astype(np.uint8)[lab]
    assert np.array_equal(maps["Nuclei"][1].cpu().numpy(), want_cls) and want_cls.max() > 0
    half = label_maps_from_parts([("Gland",) + part[1:5] + (False, 0.5)], None, lab.shape, ds=2)
    assert np.array_equal(half["Gland"][0].cpu().numpy(), lab) and half["Gland"][1] is None
    # an instance info_from_table drops (fewer than 3 contour points) fills nothing and keeps its id
    cut = cnts.copy()
    cut[4] = 2
    less = label_maps_from_parts([("Lumen", tab, cut, pts, offs, False, 1.0)], None, lab.shape)["Lumen"][0].cpu().numpy()
    assert np.array_equal(less, np.where(lab == 5, 0, lab))


def test_compute_stats_pred_dat(tmp_path, nuclei_parts, capsys):
    sys.path.insert(0, ROOT)
    import compute_stats
    from cerberus_amd.inst_info import build_from_parts, majority_type, write_dat
    from cerberus_amd.inst_metrics import InstanceStats
    from cerberus_amd.rasterize import label_maps_from_dict, load_annotations
    from cerberus_amd.wsi import wsi_meta

    lab, types, part = nuclei_parts
    dat = str(tmp_path / "slide.dat")
    write_dat(build_from_parts([part], wsi_meta(lab.shape, 0.5)), dat)
    back = label_maps_from_dict(load_annotations(dat)[0])
    assert list(back) == ["Nuclei"] and np.array_equal(back["Nuclei"][0].cpu().numpy(), lab) and len(back["Nuclei"][1]) == 43
    same = str(tmp_path / "same.npz")
    np.savez(same, **{"Nuclei": lab, "type_Nuclei-TYPE": types})
    res = compute_stats.main(["--pred_dat=%s" % dat, "--true_ann=%s" % same, "--gpu="])
    capsys.readouterr()
    assert res["images"] == 1 and res["pooled"]["pq"] == 1.0 and res["pooled"]["aji"] == 1.0 and res["pooled"]["dice2"] == 1.0 and res["pooled"]["dq"] == 1.0
    assert os.path.exists(str(tmp_path / "slide_stats.csv"))
    typed = compute_stats.main(["--pred_dat=%s" % dat, "--true_ann=%s" % same, "--types=7", "--gpu="])
    present = set(majority_type(part[1]).tolist())  # a class no instance has scores 0
    assert len(present - {0}) >= 3 and all(typed["pooled"]["pq_class%d" % g] == (1.0 if g in present else 0.0) for g in range(1, 7))
    # against a shifted copy: InstanceStats on the two maps themselves
    moved = np.zeros_like(lab)
    moved[3:, 2:] = lab[:-3, :-2]
    other = str(tmp_path / "moved.npz")
    np.savez(other, Nuclei=moved)
    res = compute_stats.main(["--pred_dat=%s" % dat, "--true_ann=%s" % other, "--tissue=nuclei", "--gpu="])
    direct = InstanceStats(0)
    direct.update(moved, lab)
    scal = direct.scalars()
    assert all(res["pooled"][k] == scal["all-%s" % k] for k in compute_stats.FIGURES) and 0.2 < res["pooled"]["pq"] < 1.0
    assert res["counters"] == direct.counters()["all"]
    # polygons on the true side: the same dictionary as .json and as .geojson, the shifted one in --pred_dir mode
    d = load_annotations(dat)[0]
    as_json = str(tmp_path / "same.json")
    with open(as_json, "w") as fh:
        json.dump({"mag": None, "instances": {"Nuclei": {k: {"contour": np.asarray(v["contour"]).tolist(), "type": int(v["type"])} for k, v in d["Nuclei"].items()}}}, fh)
    res = compute_stats.main(["--pred_dat=%s" % dat, "--true_ann=%s" % as_json, "--types=7", "--gpu="])
    assert res["pooled"]["pq"] == 1.0 and res["mpq"] == typed["mpq"] and res["pooled"] == typed["pooled"]
    import scipy.io as sio

    pd, td = tmp_path / "out", tmp_path / "ann"
    (pd / "nuclei_mat").mkdir(parents=True)
    td.mkdir()
    sio.savemat(str(pd / "nuclei_mat" / "t1.mat"), {"inst_map": moved})
    feats = [{"type": "Feature", "geometry": {"type": "Polygon", "coordinates": [[[float(x), float(y)] for x, y in np.asarray(v["contour"])] + [[float(v["contour"][0][0]), float(v["contour"][0][1])]]]}}
             for v in d["Nuclei"].values()]
    (td / "t1.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": feats}))
    res = compute_stats.main(["--pred_dir=%s" % pd, "--true_dir=%s" % td, "--gpu="])
    direct = InstanceStats(0)
    direct.update(lab, moved)
    assert all(res["pooled"][k] == direct.scalars()["all-%s" % k] for k in compute_stats.FIGURES)


def test_compute_features_dat_equals_npz(tmp_path, capsys):
    torch = _torch()
    sys.path.insert(0, ROOT)
    import compute_features
    from cerberus_amd.inst_info import build_from_parts, write_dat
    from cerberus_amd.postproc import inst_contours_device, inst_table_device
    from cerberus_amd.wsi import wsi_meta

    nuclei, gland, lumen, types = cases.slide_triple()
    for m in (gland, lumen):
        assert cases.is_round_trip_map(m, int(m.max()))
    parts = []
    for tissue, m, tmap, ds_factor in (("Nuclei", nuclei, types, 1.0), ("Gland", gland, None, 0.5), ("Lumen", lumen, None, 0.5)):
        dev = torch.from_numpy(m).cuda()
        tab = inst_table_device(dev, None if tmap is None else torch.from_numpy(tmap).cuda())
        cnts, pts, offs = inst_contours_device(dev, tab)
        parts.append((tissue, tab.cpu().numpy(), cnts, pts, offs, tmap is not None, ds_factor))
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    write_dat(build_from_parts(parts, wsi_meta(nuclei.shape, 0.5)), str(tmp_path / "a" / "slide.dat"))
    np.savez(str(tmp_path / "b" / "slide.npz"), **{"Nuclei": nuclei, "Gland": gland, "Lumen": lumen, "type_Nuclei-TYPE": types})
    from_dat = compute_features.main(["--dat=%s" % (tmp_path / "a" / "slide.dat"), "--knn=2", "--gpu="])
    from_npz = compute_features.main(["--npz=%s" % (tmp_path / "b" / "slide.npz"), "--knn=2", "--gpu="])
    capsys.readouterr()
    assert from_dat["images"] == from_npz["images"] and from_dat["images"][0]["shift"] == 1 and from_dat["images"][0]["nuclei"] == 42
    for t in ("nuclei", "gland", "lumen"):
        a, b = (tmp_path / "a" / "features" / ("slide_%s.csv" % t)).read_text(), (tmp_path / "b" / "features" / ("slide_%s.csv" % t)).read_text()
        assert a == b and len(a.splitlines()) > 4, t
