"""The contour rasteriser on the device (csrc/overlay.hip: cerb_overlay_clear / _stamp / _resolve; cerberus_amd/viz.py) against the sequential numpy
restatement of its definition (tests/overlay_ref.py).  Everything is integer: every comparison is exact equality, there is no tolerance.

Shapes are the smallest at which the kernel can go wrong: odd sizes, boxes on both sides of the lane / wave switch (a clipped box of 64 pixels),
1-pixel-high and 1-pixel-wide images, more than one 64-contour group, coordinates at the edge of the +-2^20 range and the largest side (32768)."""
import ctypes as C

import numpy as np
import pytest

import overlay_ref as ref

pytestmark = pytest.mark.gpu

SMALL = 64  # overlay.hip: OV_SMALL, the largest clipped box one lane walks


def _torch():
    import torch

    return torch


def _plane(h, w, calls):
    """clear + the stamp calls [(points, offsets, counts, width, first_ordinal, mul, div, origin)] through the C entries -> the priority plane (numpy uint32)."""
    torch = _torch()
    from cerberus_amd import _lib

    L = _lib.lib()
    nb = int(L.cerb_overlay_workspace_bytes(h, w))
    assert nb == 4 * h * w
    ws = torch.full((nb // 4,), -1, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(L.cerb_overlay_clear(ws.data_ptr(), nb, h, w, st))
    keep = []
    for pts, offs, cnts, width, first, mul, div, org in calls:
        p = torch.from_numpy(np.ascontiguousarray(np.asarray(pts, np.int32).reshape(-1, 2))).cuda()
        o = torch.from_numpy(np.asarray(offs, np.int64)).cuda()
        c = torch.from_numpy(np.asarray(cnts, np.int32)).cuda()
        keep += [p, o, c]
        _lib.check(L.cerb_overlay_stamp(p.data_ptr(), o.data_ptr(), c.data_ptr(), len(cnts), mul, div, org[0], org[1], width, first, ws.data_ptr(), nb, h, w, st))
    return ws.cpu().numpy().view(np.uint32).reshape(h, w)


def _ref_plane(h, w, calls, full=True):
    prio = np.zeros((h, w), np.uint32)
    for pts, offs, cnts, width, first, mul, div, org in calls:
        ref.paint_group(prio, pts, offs, cnts, width, first, mul, div, org, full=full)
    return prio


def _one(a, b, width, first=0):
    return (np.array([a, b], np.int64), [0], [2], width, first, 1, 1, (0, 0))


H0, W0 = 37, 53
DIRECTIONS = {"horizontal": ((5, 11), (40, 11)), "vertical": ((20, 3), (20, 30)), "diagonal": ((4, 4), (30, 30)), "antidiagonal": ((40, 5), (12, 33)),
              "slope2": ((10, 2), (25, 32)), "slope1in7": ((3, 20), (45, 26)), "reversed": ((45, 26), (3, 20))}


@pytest.mark.parametrize("width", [1, 2, 3, 12, 255])
def test_single_segments_of_every_direction_equal_the_restatement(width):
    for name, (a, b) in DIRECTIONS.items():
        call = [_one(a, b, width)]
        got, want = _plane(H0, W0, call), _ref_plane(H0, W0, call)
        assert np.array_equal(got, want), (name, width, int((got != want).sum()))
        assert want.any()


@pytest.mark.parametrize("width", [1, 2, 3, 12, 255])
def test_endpoints_on_the_border_just_outside_and_far_outside(width):
    cases = [((0, 0), (W0 - 1, H0 - 1)), ((0, H0 - 1), (W0 - 1, 0)), ((-1, 5), (W0, 20)), ((10, -1), (30, H0)), ((-3, -2), (W0 + 1, H0 + 2)),
             ((W0 + 2, 4), (W0 + 9, 30)), ((-40, -40), (-5, -6))]
    for a, b in cases:
        call = [_one(a, b, width)]
        assert np.array_equal(_plane(H0, W0, call), _ref_plane(H0, W0, call)), (a, b, width)
    m = 1 << 20
    for a, b in (((-m, -m), (m, m)), ((-m, m), (m, -m + 37)), ((-m, 20), (m, 45)), ((31, -m), (29, m))):
        call = [_one(a, b, width)]
        got, want = _plane(64, 64, call), _ref_plane(64, 64, call)
        assert np.array_equal(got, want) and want.any(), (a, b, width)


def test_a_contour_with_one_point_beyond_the_range_is_skipped_whole():
    m = 1 << 20
    tri_ok = np.array([[5, 5], [30, 8], [m, 30]], np.int64)
    tri_bad = np.array([[5, 20], [30, 22], [m + 1, 30]], np.int64)
    tri_neg = np.array([[8, 30], [-m - 1, 3], [20, 33]], np.int64)
    pts = np.concatenate([tri_ok, tri_bad, tri_neg])
    call = [(pts, [0, 3, 6], [3, 3, 3], 3, 0, 1, 1, (0, 0))]
    got, want = _plane(H0, W0, call), _ref_plane(H0, W0, call)
    assert np.array_equal(got, want)
    assert set(np.unique(got).tolist()) == {0, 1}  # the two contours that leave the range painted nothing, not even their in-range edges


def test_counts_of_zero_one_and_two():
    pts = np.array([[9, 9], [20, 12], [30, 25], [4, 30]], np.int64)
    for width, disk in ((1, 1), (2, 5), (3, 9)):
        call = [(pts, [0, 0, 1, 3], [0, 1, 2, 1], width, 0, 1, 1, (0, 0))]
        got, want = _plane(H0, W0, call), _ref_plane(H0, W0, call)
        assert np.array_equal(got, want)
        assert int((got == 1).sum()) == 0 and int((got == 2).sum()) == disk and int((got == 4).sum()) == disk and (got == 3).any()


def test_both_traversal_paths_round_the_switch_size():
    """w = 1 expands a box by 1: a horizontal segment of length L has a clipped box of (L + 3) x 3 pixels; an 8 x 8 box is exactly 64."""
    for a, b in (((10, 10), (28, 10)), ((10, 10), (29, 10)), ((10, 10), (15, 15)), ((10, 10), (16, 15)), ((10, 10), (16, 16)), ((3, 3), (3, 3))):
        area = (abs(b[0] - a[0]) + 3) * (abs(b[1] - a[1]) + 3)
        call = [_one(a, b, 1)]
        assert np.array_equal(_plane(H0, W0, call), _ref_plane(H0, W0, call)), (a, b, area)
    areas = sorted((abs(b[0] - a[0]) + 3) * (abs(b[1] - a[1]) + 3) for a, b in (((10, 10), (28, 10)), ((10, 10), (29, 10)), ((10, 10), (15, 15)), ((10, 10), (16, 15))))
    assert areas == [63, 64, 66, 72] and SMALL == 64
    # 1-pixel-high and 1-pixel-wide images: long boxes that are one row / one column
    for (h, w), a, b in (((1, 200), (-5, 0), (230, 0)), ((1, 200), (3, -2), (150, 3)), ((200, 1), (0, -5), (0, 230)), ((200, 1), (-2, 10), (3, 190)),
                         ((1, 40), (2, 0), (30, 0)), ((40, 1), (0, 2), (0, 30))):
        for width in (1, 2, 5):
            call = [_one(a, b, width)]
            got, want = _plane(h, w, call), _ref_plane(h, w, call)
            assert np.array_equal(got, want) and want.any(), (h, w, a, b, width)


@pytest.fixture(scope="module")
def random_contours():
    """200 closed contours of 3..40 points on 97 x 131, some reaching outside, a few empty, stored with gaps and out of order in the point list."""
    rs = np.random.RandomState(20)
    n, h, w = 200, 97, 131
    counts = rs.randint(3, 41, n)
    counts[rs.choice(n, 12, replace=False)] = 0
    order = rs.permutation(n)
    offsets, pts, cur = np.zeros(n, np.int64), [], 0
    for i in order:
        gap = int(rs.randint(0, 4))
        pts.append(rs.randint(-1000, 1000, (gap, 2)))  # never read
        cur += gap
        offsets[i] = cur
        c = int(counts[i])
        centre = rs.randint(-10, [w + 10, h + 10])
        if i % 25 == 0:  # a long one across the picture
            pp = rs.randint(-30, [w + 30, h + 30], (c, 2))
        else:
            pp = centre + rs.randint(-6, 7, (c, 2))
        pts.append(pp)
        cur += c
    pts = np.concatenate(pts).astype(np.int64)
    return h, w, pts, offsets, counts.astype(np.int64)


def test_two_hundred_random_contours_two_stamp_calls_sharing_one_plane(random_contours):
    h, w, pts, offsets, counts = random_contours
    calls = [(pts, offsets[:60], counts[:60], 12, 0, 1, 1, (0, 0)), (pts, offsets[60:], counts[60:], 2, 60, 1, 1, (0, 0))]
    got, want = _plane(h, w, calls), _ref_plane(h, w, calls, full=False)
    assert np.array_equal(got, want), int((got != want).sum())
    assert got.max() > 60 and ((got > 0) & (got <= 60)).any() and (got == 0).any()  # (both calls show, and so does the picture)
    # the second call in front of the first gives the same plane: the result does not depend on the order of execution
    assert np.array_equal(_plane(h, w, calls[::-1]), want)


def test_many_contours_one_wave_per_group():
    """A stamp call shares a 64-contour group among several waves while it has fewer than 2048 groups, and gives it one wave from there on: 2048 x 64
    + 37 one-point contours of width 1 (each paints exactly its own pixel -- test_overlay_host.py's hand answer) and, in a second call on the same
    plane, 300 groups of triangles.  The disks' plane is the largest ordinal per pixel."""
    h, w = 97, 131
    rs = np.random.RandomState(31)
    n = 2048 * 64 + 37
    pts = rs.randint(-3, [w + 3, h + 3], (n, 2)).astype(np.int64)
    want = np.zeros((h, w), np.uint32)
    inside = (pts[:, 0] >= 0) & (pts[:, 0] < w) & (pts[:, 1] >= 0) & (pts[:, 1] < h)
    np.maximum.at(want, (pts[inside, 1], pts[inside, 0]), (np.arange(n, dtype=np.uint32) + 1)[inside])
    disks = (pts, np.arange(n, dtype=np.int64), np.ones(n, np.int64), 1, 0, 1, 1, (0, 0))
    assert np.array_equal(_plane(h, w, [disks]), want) and (want > 2048 * 64).any()
    m = 300 * 64
    tri = (rs.randint(0, [w, h], (m, 1, 2)) + rs.randint(-4, 5, (m, 3, 2))).reshape(-1, 2).astype(np.int64)
    tris = (tri, np.arange(m, dtype=np.int64) * 3, np.full(m, 3, np.int64), 2, n, 1, 1, (0, 0))
    got = _plane(h, w, [disks, tris])
    ref.paint_group(want, tri[-3 * 400:], np.arange(400, dtype=np.int64) * 3, np.full(400, 3, np.int64), 2, n + m - 400)
    top = want > n + m - 400  # the last 400 triangles lie on top of everything before them
    assert top.any() and np.array_equal(got[top], want[top]) and got.max() == want.max()


@pytest.mark.parametrize("mul,div", [(1, 1), (2, 1), (1, 4), (2, 8), (1, 8)])
def test_point_transform_truncates_toward_zero(random_contours, mul, div):
    h, w, pts, offsets, counts = random_contours
    big = (pts * div + div // 2) // mul  # stored coordinates: the picture's, scaled up by div / mul
    org = (5 * div + 1, 7 * div + 3)     # q = p mul - org is negative for the contours near the top-left corner
    calls = [(big, offsets[:70], counts[:70], 2, 0, mul, div, org)]
    got, want = _plane(h, w, calls), _ref_plane(h, w, calls, full=False)
    assert np.array_equal(got, want) and want.any()
    used = np.concatenate([big[o:o + c] for o, c in zip(offsets[:70], counts[:70])])
    t = used * mul - np.asarray(org)
    assert (t < 0).any()
    if div > 1:  # truncation differs from floor for the negative quotients that are not whole
        assert ((t < 0) & (t % div != 0)).any()


@pytest.mark.parametrize("up", [1, 2, 3])
def test_resolve_upscales_and_respects_padded_row_strides(random_contours, up):
    torch = _torch()
    from cerberus_amd import _lib

    L = _lib.lib()
    _, _, pts, offsets, counts = random_contours
    sh, sw = 33, 45
    h, w = sh * up, sw * up
    rs = np.random.RandomState(up)
    img = rs.randint(0, 256, (sh, sw, 3)).astype(np.uint8)
    colours = rs.randint(0, 1 << 24, len(counts)).astype(np.uint32)
    group = {"points": pts, "offsets": offsets, "counts": counts, "colours": colours, "width": 2, "mul": 1, "div": 1, "origin": (0, 0)}
    want = ref.draw(img, [group], up, full=False)
    s_stride, d_stride = sw * 3 + 7, w * 3 + 5
    src = torch.full((sh, s_stride), 0xA5, dtype=torch.uint8, device="cuda")
    src[:, :sw * 3] = torch.from_numpy(img.reshape(sh, -1)).cuda()
    dst = torch.full((h, d_stride), 0x5A, dtype=torch.uint8, device="cuda")
    nb = int(L.cerb_overlay_workspace_bytes(h, w))
    ws = torch.empty(nb // 4, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p, o, c = (torch.from_numpy(a).cuda() for a in (pts.astype(np.int32), offsets, counts.astype(np.int32)))
    col = torch.from_numpy(colours.view(np.int32)).cuda()
    _lib.check(L.cerb_overlay_clear(ws.data_ptr(), nb, h, w, st))
    _lib.check(L.cerb_overlay_stamp(p.data_ptr(), o.data_ptr(), c.data_ptr(), len(counts), 1, 1, 0, 0, 2, 0, ws.data_ptr(), nb, h, w, st))
    _lib.check(L.cerb_overlay_resolve(src.data_ptr(), s_stride, sh, sw, up, col.data_ptr(), len(counts), ws.data_ptr(), nb, dst.data_ptr(), d_stride, h, w, st))
    out = dst.cpu().numpy()
    assert np.array_equal(out[:, :w * 3].reshape(h, w, 3), want)
    assert (out[:, w * 3:] == 0x5A).all() and (src.cpu().numpy()[:, sw * 3:] == 0xA5).all()  # the bytes between rows stay untouched
    # the public wrapper draws the same picture from host or device arrays
    from cerberus_amd.viz import draw_contours_device

    assert np.array_equal(draw_contours_device(img, [group], up).cpu().numpy(), want)
    dev_group = dict(group, points=p, offsets=o, counts=c, colours=col)
    assert np.array_equal(draw_contours_device(torch.from_numpy(img).cuda(), [dev_group], up).cpu().numpy(), want)


def test_largest_side():
    call = [_one((0, 0), (32767, 7), 3)]
    got, want = _plane(8, 32768, call), _ref_plane(8, 32768, call)
    assert np.array_equal(got, want) and want[7, 32767] == 1 and want[0, 0] == 1
    got = _plane(32768, 8, [_one((0, 0), (7, 32767), 3)])
    assert np.array_equal(got, _ref_plane(32768, 8, [_one((0, 0), (7, 32767), 3)]))


def test_every_refusal_returns_an_error_and_writes_nothing():
    torch = _torch()
    from cerberus_amd import _lib

    L = _lib.lib()
    h, w = 16, 24
    nb = 4 * h * w
    assert L.cerb_overlay_workspace_bytes(h, w) == nb and L.cerb_overlay_workspace_bytes(32769, 4) == 0 and L.cerb_overlay_workspace_bytes(0, 4) == 0
    ws = torch.full((h * w,), 0x01020304, dtype=torch.int32, device="cuda")
    dst = torch.full((h, w, 3), 0x77, dtype=torch.uint8, device="cuda")
    src = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    pts = torch.tensor([[1, 1], [10, 10], [3, 12]], dtype=torch.int32, device="cuda")
    offs, cnts = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.full((1,), 3, dtype=torch.int32, device="cuda")
    col = torch.zeros(1, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, O, N, WS, S, D, CO = pts.data_ptr(), offs.data_ptr(), cnts.data_ptr(), ws.data_ptr(), src.data_ptr(), dst.data_ptr(), col.data_ptr()

    def stamp(points=P, offsets=O, counts=N, n=1, mul=1, div=1, width=3, first=0, wsp=WS, wsb=nb, hh=h, ww=w):
        return L.cerb_overlay_stamp(points, offsets, counts, n, mul, div, 0, 0, width, first, wsp, wsb, hh, ww, st)

    def resolve(srcp=S, ss=w * 3, sh=h, sw=w, up=1, cp=CO, n=1, wsp=WS, wsb=nb, dp=D, dstride=w * 3, hh=h, ww=w):
        return L.cerb_overlay_resolve(srcp, ss, sh, sw, up, cp, n, wsp, wsb, dp, dstride, hh, ww, st)

    bad = [stamp(points=None), stamp(offsets=None), stamp(counts=None), stamp(wsp=None), stamp(n=-1), stamp(mul=0), stamp(mul=17), stamp(div=0), stamp(div=4097),
           stamp(width=0), stamp(width=256), stamp(wsb=nb - 1), stamp(hh=32769, wsb=1 << 40), stamp(ww=0), stamp(first=-1), stamp(first=(1 << 32) - 2),
           stamp(n=(1 << 32) - 1),
           resolve(srcp=None), resolve(wsp=None), resolve(dp=None), resolve(cp=None), resolve(up=0), resolve(up=9), resolve(sh=h - 1), resolve(sw=w + 1),
           resolve(up=2), resolve(wsb=nb - 1), resolve(n=-1), resolve(n=(1 << 32) - 1), resolve(ss=w * 3 - 1), resolve(dstride=w * 3 - 1),
           resolve(hh=32769, sh=32769, wsb=1 << 40),
           L.cerb_overlay_clear(None, nb, h, w, st), L.cerb_overlay_clear(WS, nb - 1, h, w, st), L.cerb_overlay_clear(WS, 1 << 40, 32769, w, st),
           L.cerb_overlay_clear(WS, nb, 0, w, st)]
    assert all(rc != 0 for rc in bad), [i for i, rc in enumerate(bad) if rc == 0]
    assert L.cerb_last_error().startswith(b"cerb_overlay_")
    torch.cuda.synchronize()
    assert (ws.cpu().numpy() == 0x01020304).all() and (dst.cpu().numpy() == 0x77).all()
    # and the same arguments without the fault are accepted
    assert L.cerb_overlay_clear(WS, nb, h, w, st) == 0 and stamp() == 0 and resolve() == 0 and stamp(n=0) == 0 and resolve(cp=None, n=0) == 0
    assert L.cerb_version() >= 3


def test_dictionary_overlay_on_the_fixture_of_test_overlay_rendering():
    """visualize_instances_dict_device on the dictionary of tests/test_host_logic.py::test_overlay_rendering: the restatement's picture, and that test's
    colour and draw-order assertions."""
    import cerberus_amd
    from cerberus_amd.viz import DEFAULT_VIZ_INFO, visualize_instances_dict_device

    img = np.full((60, 80, 3), 10, np.uint8)
    sq = np.array([[10, 10], [10, 40], [50, 40], [50, 10]], np.int32)
    tri = np.array([[60, 5], [60, 25], [75, 25]], np.int32)
    d = {"Nuclei": {1: {"contour": sq, "type": 3}, 2: {"contour": tri}}, "Lumen": {7: {"contour": sq + 2}}}
    out = visualize_instances_dict_device(img, d)
    assert isinstance(out, np.ndarray) and out.shape == img.shape and out.dtype == np.uint8 and np.array_equal(img, np.full((60, 80, 3), 10, np.uint8))
    assert np.array_equal(out, ref.draw(img, ref.dict_groups(d, DEFAULT_VIZ_INFO), 1, full=True))
    assert tuple(out[25, 10]) == DEFAULT_VIZ_INFO["nuclei"]["type_colour"][3]   # left edge of the typed square, drawn last
    assert tuple(out[15, 60]) == DEFAULT_VIZ_INFO["nuclei"]["inst_colour"]      # untyped triangle
    assert tuple(out[30, 30]) == (10, 10, 10)                                   # interior untouched (outline only)
    assert (out == np.array(DEFAULT_VIZ_INFO["lumen"]["inst_colour"], np.uint8)).all(axis=2).sum() > 50
    assert tuple(out[12, 20]) == DEFAULT_VIZ_INFO["nuclei"]["type_colour"][3]   # where the lumen's 12-px stroke lies under the nuclei's 3-px one
    assert cerberus_amd.visualize_instances_dict_device is visualize_instances_dict_device


def test_slide_overlay_from_parts_equals_the_dictionary_drawn_by_the_restatement(tmp_path):
    """A small .npy slide labelled through WSIRunner.postprocess; overlay_from_parts on its parts at ds = 4, on the reader's thumbnail, against the
    restatement fed with build_from_parts' contours after (c / 4).astype(int) -- the reference's own arithmetic (misc/viz_utils.py:164-168)."""
    torch = _torch()
    from cerberus_amd import tissue
    from cerberus_amd.inst_info import build_from_parts
    from cerberus_amd.reader import WSIReader
    from cerberus_amd.viz import DEFAULT_VIZ_INFO, overlay_from_parts
    from cerberus_amd.wsi import WSIRunner, collect_wsi_inst_arrays, synth_slide

    from cerberus_amd import synth_maps as synth

    H, W = 500, 768
    np.save(str(tmp_path / "s1.npy"), synth_slide(H, W, seed=5).cpu().numpy())
    # the slide's canvases as the slide tests of tests/test_drivers_gpu.py make them (the seeded test weights find next to nothing in seeded pixels):
    # probability maps with a few hundred nuclei, glands and lumina, class maps in coarse blocks
    rs = np.random.RandomState(12)
    maps = {"Nuclei-INST": synth.nuclei_maps(512, W, 31, 250.0, noise=0.02), "Gland-INST": synth.blob_maps(512, W, 9, 14, 20.0, 70.0, rim=4.0, sharp=1.0, noise=0.02, holes=0.3),
            "Lumen-INST": synth.blob_maps(512, W, 11, 30, 8.0, 30.0, rim=2.0, sharp=1.0, noise=0.02),
            "Nuclei-TYPE": np.kron(rs.randint(0, 7, (32, W // 16)), np.ones((16, 16), np.int64)).astype(np.uint8),
            "Gland-TYPE": np.kron(rs.randint(0, 3, (32, W // 16)), np.ones((16, 16), np.int64)).astype(np.uint8)}
    full = {k: torch.from_numpy(np.ascontiguousarray(v[:H])).cuda() for k, v in maps.items()}
    inst, _ = WSIRunner.postprocess(full, wsi_mode=True)
    parts = collect_wsi_inst_arrays(inst, full, (H, W))
    assert sorted(p[0] for p in parts) == ["Gland", "Lumen", "Nuclei"] and {p[0]: p[6] for p in parts}["Gland"] == 0.5
    thumb = tissue.thumbnail(WSIReader.open(input_img=str(tmp_path / "s1.npy")), 0.5, "mpp", 4)
    assert thumb.shape == (H // 4, W // 4, 3)
    got = overlay_from_parts(thumb, parts[::-1], ds=4, line_width=2)
    assert got.is_cuda and got.dtype == torch.uint8
    dat = build_from_parts(parts, {})
    n_inst = sum(len(dat[t]) for t in ("Gland", "Lumen", "Nuclei"))
    assert n_inst > 20
    shrunk = {t: {k: dict(v, contour=(v["contour"] / 4).astype("int")) for k, v in dat[t].items()} for t in ("Gland", "Lumen", "Nuclei")}
    want = ref.draw(thumb, ref.dict_groups(shrunk, DEFAULT_VIZ_INFO, width=2, min_points=3), 1, full=False)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != thumb).any()
