"""Host side of the device overlays: the restatement itself (tests/overlay_ref.py: int64 numpy against Python integers at the extremes, hand
answers), inst_info.majority_type against info_from_table, the packing of slide parts and of prebuilt dictionaries, and the command-line refusals.
No GPU."""
import os
import sys

import numpy as np
import pytest

import overlay_ref as ref

from conftest import ROOT


def test_numpy_predicate_equals_the_python_integer_predicate_at_the_extremes():
    rs = np.random.RandomState(1)
    m = 1 << 20
    segs = [(-m, -m, m, m, 255), (m, -m, -m, m, 255), (-m, 0, m, 1, 255), (m, m, m, m, 255), (-m, m, -m, -m, 1), (0, 0, 0, 0, 2), (-m, -m, m, m - 1, 1)]
    for _ in range(200):
        big = rs.rand() < 0.5
        lo, hi = (-m, m + 1) if big else (-40, 41)
        segs.append(tuple(int(v) for v in rs.randint(lo, hi, 4)) + (int(rs.choice([1, 2, 3, 12, 254, 255])),))
    corners = np.array([[0, 0], [32767, 0], [0, 32767], [32767, 32767]])
    for ax, ay, bx, by, w in segs:
        near = np.array([[ax, ay], [bx, by], [(ax + bx) // 2, (ay + by) // 2]])[:, None, :] + rs.randint(-130, 131, (1, 40, 2))
        px = np.concatenate([near.reshape(-1, 2), corners, rs.randint(0, 32768, (40, 2))]).astype(np.int64)
        got = ref.covered_np(px[:, 0], px[:, 1], ax, ay, bx, by, w)
        want = np.array([ref.covered_int(int(x), int(y), ax, ay, bx, by, w) for x, y in px])
        assert np.array_equal(got, want), (ax, ay, bx, by, w)
    # the largest intermediate values stay inside int64: |u|, |v| < 2^22
    assert 255 * 255 * 2 * (1 << 42) < 1 << 62 and 4 * 2 * (1 << 44) < 1 << 62


def _painted(h, w, pts, width, full=True):
    prio = np.zeros((h, w), np.uint32)
    ref.paint_contour(prio, np.asarray(pts, np.int64), width, 1, full=full)
    return prio > 0


def test_hand_answers():
    hor = _painted(8, 10, [[2, 3], [6, 3]], 1)
    assert hor.sum() == 5 and hor[3, 2:7].all()
    w2, w3 = _painted(8, 10, [[2, 3], [6, 3]], 2), _painted(8, 10, [[2, 3], [6, 3]], 3)
    assert w2.sum() == 5 * 3 + 2 and w3.sum() == 5 * 3 + 6  # the band plus the caps: a plus (r = 1) adds 1 pixel per end, the 3 x 3 disk (r = 1.5) adds 3
    assert w2[:, 4].sum() == 3 and w3[:, 4].sum() == 3 and _painted(8, 10, [[2, 3], [6, 3]], 4)[:, 4].sum() == 5  # even widths paint w + 1 across, odd ones w
    for width, n in ((1, 1), (2, 5), (3, 9)):
        disk = _painted(9, 9, [[4, 4]], width)
        assert disk.sum() == n and disk[4, 4] and np.array_equal(disk, _painted(9, 9, [[4, 4], [4, 4]], width))
    plus = _painted(9, 9, [[4, 4]], 2)
    assert plus[3, 4] and plus[5, 4] and plus[4, 3] and plus[4, 5] and not plus[3, 3]
    # the closing segment exists: the third side of a triangle
    tri = _painted(20, 20, [[2, 2], [15, 2], [15, 12]], 1)
    assert tri[7, 8] or tri[6, 8] or tri[7, 9]
    assert tri.sum() > 14 + 11 + 5
    # a later contour wins, whatever it covers
    prio = np.zeros((12, 12), np.uint32)
    ref.paint_group(prio, [[1, 5], [10, 5], [5, 1], [5, 10]], [0, 2], [2, 2], 1)
    assert prio[5, 5] == 2 and prio[5, 4] == 1 and prio[4, 5] == 2
    out = ref.resolve(np.zeros((12, 12, 3), np.uint8), prio, [ref.colour_word((255, 0, 0)), ref.colour_word((1, 2, 3))])
    assert tuple(out[5, 5]) == (1, 2, 3) and tuple(out[5, 4]) == (255, 0, 0) and tuple(out[0, 0]) == (0, 0, 0)
    # a contour that leaves the range is skipped as a whole
    assert not _painted(12, 12, [[1, 1], [8, 1], [(1 << 20) + 1, 5]], 3).any() and _painted(12, 12, [[1, 1], [8, 1], [1 << 20, 5]], 3).any()
    # the point transform truncates toward zero
    assert ref.transform([[-7, 7], [-8, 9]], 1, 4).tolist() == [[-1, 1], [-2, 2]] and ref.transform([[3, 3]], 2, 4, (9, 1)).tolist() == [[0, 1]]


def test_box_limited_painter_equals_the_full_image_painter():
    rs = np.random.RandomState(4)
    for _ in range(60):
        k = int(rs.randint(1, 7))
        pts = rs.randint(-25, 70, (k, 2))
        width = int(rs.choice([1, 2, 3, 12, 60]))
        assert np.array_equal(_painted(41, 47, pts, width, full=True), _painted(41, 47, pts, width, full=False))


def test_majority_type_equals_info_from_table():
    from cerberus_amd.inst_info import info_from_table, majority_type

    rs = np.random.RandomState(7)
    n = 400
    tab = np.zeros((n, 16), np.int64)
    votes = rs.randint(0, 4, (n, 8)) * rs.randint(0, 2, (n, 8))  # many zeros and many ties
    votes[:40] = 0
    votes[:40, 0] = rs.randint(1, 50, 40)          # background only
    votes[40:80, 0] = 9                            # background ahead of a second class: the second class wins
    votes[40:80, 1:] = rs.randint(0, 3, (40, 7))
    votes[80:100] = 5                              # an eight-way tie
    votes[100:120, 0] = 0                          # no background vote
    tab[:, 8:16] = votes
    tab[:, 0] = np.maximum(votes.sum(axis=1), 1)
    tab[:, 1:7] = rs.randint(0, 100, (n, 6))
    cnts = np.full(n, 3, np.int32)
    pts = rs.randint(0, 100, (3 * n, 2)).astype(np.int32)
    offs = np.arange(n, dtype=np.int64) * 3
    info = info_from_table(tab, cnts, pts, offs, True)
    assert len(info) == n
    got = majority_type(tab)
    assert got.shape == (n,) and got.tolist() == [info[i + 1]["type"] for i in range(n)]
    assert set(got[:40].tolist()) == {0} and (got[40:80] != 0).any() and set(got[80:100].tolist()) == {1}
    assert majority_type(np.zeros((0, 16), np.int64)).shape == (0,)


def _parts():
    rs = np.random.RandomState(9)

    def part(tissue, n, has_type, ds_factor):
        tab = np.zeros((n, 16), np.int64)
        tab[:, 0] = rs.randint(1, 90, n)
        tab[1, 0] = 0  # dropped: no area
        if has_type:
            tab[:, 8:16] = rs.randint(0, 5, (n, 8))
        cnts = rs.randint(3, 9, n).astype(np.int32)
        cnts[2] = 2  # dropped: fewer than 3 points
        offs = np.cumsum(cnts, dtype=np.int64) - cnts
        pts = rs.randint(0, 300, (int(cnts.sum()), 2)).astype(np.int32)
        return (tissue, tab, cnts, pts, offs, has_type, ds_factor)

    return [part("Nuclei", 9, True, 1.0), part("Lumen", 5, False, 0.5), part("Gland", 6, True, 0.5)]


def test_packing_of_parts_follows_the_dictionary():
    from cerberus_amd.inst_info import build_from_parts
    from cerberus_amd.viz import DEFAULT_VIZ_INFO, colour_word, contour_colours, pack_parts

    parts = _parts()
    groups = pack_parts(parts, ds=4, origin=(8, 12))
    assert [g["width"] for g in groups] == [12, 12, 3] and [g["mul"] for g in groups] == [2, 2, 1]  # Gland, Lumen, Nuclei whatever the order of parts
    assert all(g["div"] == 4 and g["origin"] == (8, 12) for g in groups)
    assert all(g["width"] == 2 for g in pack_parts(parts, line_width=2))
    dat = build_from_parts(parts, {})
    for g, tissue in zip(groups, ("Gland", "Lumen", "Nuclei")):
        part = [p for p in parts if p[0] == tissue][0]
        assert g["counts"][1] == 0 and g["counts"][2] == 0 and (g["counts"] > 0).sum() == len(dat[tissue]) == len(part[2]) - 2
        kept = np.nonzero(g["counts"])[0]
        vi = DEFAULT_VIZ_INFO[tissue.lower()]
        for i, d in zip(kept.tolist(), dat[tissue].values()):
            mine = np.asarray(g["points"][g["offsets"][i]:g["offsets"][i] + g["counts"][i]], np.int64) * g["mul"]
            assert np.array_equal(mine, d["contour"])  # the dictionary's coordinates
            want = vi["type_colour"].get(d["type"], vi["inst_colour"]) if "type" in d else vi["inst_colour"]
            assert int(g["colours"][i]) == colour_word(want)
    assert contour_colours("Lumen", parts[1][1], False).tolist() == [colour_word((255, 0, 255))] * 5
    assert colour_word((1, 2, 3)) == 1 | 2 << 8 | 3 << 16 and groups[0]["colours"].dtype == np.uint32


def test_packing_of_tile_origins_and_of_prebuilt_dictionaries():
    from cerberus_amd.inst_info import build_from_parts
    from cerberus_amd.viz import DEFAULT_VIZ_INFO, colour_word, pack_parts

    nuc = _parts()[0]
    origin = np.stack([np.arange(9) * 100, np.arange(9) * 7], axis=1)
    part = nuc + (origin,)
    (g,) = pack_parts([part])
    dat = build_from_parts([part], {})["Nuclei"]
    kept = np.nonzero(g["counts"])[0]
    assert g["mul"] == 1 and len(kept) == len(dat) == 7
    for i, d in zip(kept.tolist(), dat.values()):
        assert np.array_equal(g["points"][g["offsets"][i]:g["offsets"][i] + g["counts"][i]], d["contour"])
    # the same with a point list that is not the concatenation of the runs
    shuffled = (nuc[0], nuc[1], nuc[2], np.concatenate([np.zeros((4, 2), np.int32), nuc[3]]), nuc[4] + 4) + nuc[5:] + (origin,)
    (g2,) = pack_parts([shuffled])
    for i in kept.tolist():
        assert np.array_equal(g2["points"][g2["offsets"][i]:g2["offsets"][i] + g2["counts"][i]], g["points"][g["offsets"][i]:g["offsets"][i] + g["counts"][i]])
    # prebuilt per-region dictionaries: drawn after the tissue's parts, same width, type colour where there is a type
    sq = np.array([[10, 10], [10, 40], [50, 40], [50, 10]])
    extra = {"Gland": {"k1": {"contour": sq, "type": 2}, "k2": {"contour": sq[:2]}, "k3": {"contour": sq + 1}}, "Nuclei": {}}
    groups = pack_parts([nuc], extra=extra, ds=8)
    assert len(groups) == 2 and groups[0]["width"] == 12 and groups[0]["div"] == 8 and groups[1]["width"] == 3
    assert groups[0]["counts"].tolist() == [4, 0, 4] and groups[0]["offsets"].tolist() == [0, 4, 6] and np.array_equal(groups[0]["points"][6:], sq + 1)
    vi = DEFAULT_VIZ_INFO["gland"]
    assert groups[0]["colours"].tolist() == [colour_word(vi["type_colour"][2]), colour_word(vi["inst_colour"]), colour_word(vi["inst_colour"])]


def test_new_names_are_exported():
    import cerberus_amd
    from cerberus_amd import viz

    for name in ("draw_contours_device", "contour_colours", "overlay_from_parts", "visualize_instances_dict_device"):
        assert getattr(cerberus_amd, name) is getattr(viz, name)


def test_option_tables_carry_the_new_flags():
    from cerberus_amd.cli import TILE_OPTIONS, WSI_DRIVER_OPTIONS, parse

    a = parse("run_infer_tile.py", TILE_OPTIONS, ["--synthetic"])
    assert a["--overlay"] == "host"
    assert parse("run_infer_tile.py", TILE_OPTIONS, ["--overlay=device"])["--overlay"] == "device"
    b = parse("run_infer_wsi.py", WSI_DRIVER_OPTIONS, [])
    assert b["--save_overlay"] is False and b["--overlay_ds"] == "8"
    c = parse("run_infer_wsi.py", WSI_DRIVER_OPTIONS, ["--save_overlay", "--overlay_ds=4"])
    assert c["--save_overlay"] is True and c["--overlay_ds"] == "4"
    for opts, flags in ((TILE_OPTIONS, ("--overlay",)), (WSI_DRIVER_OPTIONS, ("--save_overlay", "--overlay_ds"))):
        for flag in flags:
            assert "(not in the reference)" in [o for o in opts if o[0] == flag][0][3]


def test_command_line_refusals_fire_without_a_device(tmp_path):
    sys.path.insert(0, ROOT)
    import run_infer_tile
    import run_infer_wsi

    slides = tmp_path / "slides"
    slides.mkdir()
    (slides / "s1.txt").write_text("synthetic:700x900:5")
    common = ["--synthetic", "--input_dir=%s" % slides, "--output_dir=%s" % (tmp_path / "out"), "--logging_dir=%s" % (tmp_path / "log")]
    with pytest.raises(ValueError, match="synthetic slide spec"):
        run_infer_wsi.main(common + ["--wsi_file_ext=.txt", "--save_overlay"])
    for bad in ("0", "-3", "2.5", "x"):
        with pytest.raises(ValueError, match="--overlay_ds"):
            run_infer_wsi.main(common + ["--wsi_file_ext=.txt", "--save_overlay", "--overlay_ds=%s" % bad])
    # a thumbnail side above 32768: the smallest divisor that fits is named (a strip of 70000 x 8 pixels)
    big = tmp_path / "big"
    big.mkdir()
    np.save(str(big / "huge.npy"), np.zeros((8, 70000, 3), np.uint8))
    with pytest.raises(ValueError, match=r"--overlay_ds=3"):
        run_infer_wsi.main(["--synthetic", "--input_dir=%s" % big, "--wsi_file_ext=.npy", "--output_dir=%s" % (tmp_path / "out"), "--logging_dir=%s" % (tmp_path / "log"),
                            "--save_overlay", "--overlay_ds=2"])
    with pytest.raises(SystemExit, match="--overlay takes host or device"):
        run_infer_tile.main(["--synthetic", "--input_dir=%s" % slides, "--output_dir=%s" % (tmp_path / "out"), "--overlay=gpu"])
    assert not os.path.exists(str(tmp_path / "out"))
