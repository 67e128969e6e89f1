"""The pyramidal JPEG-tiled TIFF without a GPU: the restatement of the tile streams (tests/tiff_pyramid_ref.py) against PIL / libjpeg-turbo tile by
tile, and cerberus_amd.tiff_pyramid.PyramidWriter fed the restatement's tiles against libtiff (through PIL) and the project's own reader.  The GPU tests
(tests/test_tiff_pyramid_gpu.py) then hold the kernels to the restatement."""
import functools
import os
import sys

import numpy as np
import pytest

import jpeg_enc_ref as er
import tiff_pyramid_ref as tr

CASES = tr.cases()
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _scans(i):
    _, img, tile, q, ss = CASES[i]
    return tr.tile_scans(tr.pad_edge(img, tile), tile, q, ss)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_every_tile_scan_of_the_restatement_is_pils(i):
    _, img, tile, q, ss = CASES[i]
    tiles = tr.crops(tr.pad_edge(img, tile), tile)
    assert len(tiles) == len(_scans(i)) >= 1
    for k, (crop, scan) in enumerate(zip(tiles, _scans(i))):
        assert scan == er.scan_of(er.pil_encode(crop, q, ss, restart_rows=1)), (k, len(scan))


def test_the_cases_cover_stuffing_odd_lengths_and_a_wrapped_restart_number():
    scans = [s for i in range(len(CASES)) for s in _scans(i)]
    assert any(b"\xff\x00" in s for s in scans)
    assert any((41 + len(s) + 2) & 1 for s in scans) and any(not (41 + len(s) + 2) & 1 for s in scans)
    assert any(s.count(b"\xff\xd0") >= 2 and b"\xff\xd7" in s for s in scans)  # RST0 .. RST7, RST0 again
    _, img, tile, q, ss = CASES[4]
    data, offsets, counts = tr.tile_streams(tr.pad_edge(img, tile), tile, q, ss)
    assert len(counts) == 12 and not (offsets & 1).any() and offsets[-1] == len(data) and (np.diff(offsets) - counts).max() == 1
    for o, c in zip(offsets[:-1], counts):
        assert data[o:o + 41] == tr.prefix(tile, ss) and data[o + c - 2:o + c] == b"\xff\xd9" and (c % 2 == 0 or data[o + c] == 0)


def _levels_and_tiles():
    _, img, tile, q, ss = CASES[4]  # 150 x 200 at tile 64: levels 150 x 200, 75 x 100, 38 x 50
    lv = tr.levels(img, tile)
    return img, tile, q, ss, lv, [tr.tile_streams(tr.pad_edge(a, tile), tile, q, ss) for a in lv]


def _write(path, order=None, **kw):
    from cerberus_amd.tiff_pyramid import PyramidWriter

    img, tile, q, ss, lv, streams = _levels_and_tiles()
    w = PyramidWriter(str(path), img.shape[1], img.shape[0], tile, q, ss, **kw)
    assert w.sizes == [(a.shape[1], a.shape[0]) for a in lv]
    jobs = [(k, t) for k, (_, _, counts) in enumerate(streams) for t in range(len(counts))]
    if order is None:
        for k, (data, offsets, counts) in enumerate(streams):  # a level at a time, as the encoder hands them over
            w.add_tiles(k, list(range(len(counts))), data, offsets, counts)
    else:
        for j in order(len(jobs)):  # tile by tile
            k, t = jobs[j]
            data, offsets, counts = streams[k]
            w.add_tiles(k, [t], data, offsets[t:t + 1], counts[t:t + 1])
    assert not os.path.exists(str(path)) and os.path.exists(str(path) + ".part")
    w.close()
    assert os.path.exists(str(path)) and not os.path.exists(str(path) + ".part")
    return lv, tile, q, ss


def _frames(path):
    from PIL import Image

    im = Image.open(str(path))
    out = []
    for k in range(im.n_frames):
        im.seek(k)
        out.append(np.asarray(im.convert("RGB")).copy())
    return out


def test_writer_file_opens_in_libtiff_and_in_the_reader_to_pils_pixels(tmp_path):
    import struct

    from cerberus_amd.reader import TiffReader

    path = tmp_path / "p.tif"
    lv, tile, q, ss = _write(path, mpp=0.5)
    raw = open(str(path), "rb").read()
    assert raw[:4] == b"II\x2b\x00" and struct.unpack("<HH", raw[4:8]) == (8, 0)  # BigTIFF
    frames = _frames(path)
    assert [f.shape for f in frames] == [a.shape for a in lv] == [(150, 200, 3), (75, 100, 3), (38, 50, 3)]
    want = [tr.expected_pixels(a, tile, q, ss) for a in lv]
    for k, (f, wnt) in enumerate(zip(frames, want)):
        assert np.array_equal(f, wnt), (k, int((f != wnt).sum()))
    r = TiffReader(str(path))
    assert r.big and [tuple(d) for d in r.info.level_dimensions] == [(200, 150), (100, 75), (50, 38)]
    assert tuple(float(v) for v in r.info.mpp) == (0.5, 0.5)
    for k, f in enumerate(frames):
        p = r.levels[k]
        assert (p.compression, p.photometric, p.tw, p.th, p.subfile & 1) == (7, 6, tile, tile, 1 if k else 0)
        assert np.array_equal(r._read_level(k, 0, 0, p.w, p.h), f), k


def test_tiles_added_in_a_shuffled_order_give_the_same_pixels(tmp_path):
    _write(tmp_path / "a.tif")
    _write(tmp_path / "b.tif", order=lambda n: np.random.RandomState(4).permutation(n))
    fa, fb = _frames(tmp_path / "a.tif"), _frames(tmp_path / "b.tif")
    assert len(fa) == len(fb) == 3 and all(np.array_equal(a, b) for a, b in zip(fa, fb))


def test_writer_refuses_an_incomplete_level_and_a_bad_tile_size(tmp_path):
    from cerberus_amd.tiff_pyramid import PyramidWriter

    img, tile, q, ss, lv, streams = _levels_and_tiles()
    path = tmp_path / "short.tif"
    w = PyramidWriter(str(path), img.shape[1], img.shape[0], tile, q, ss)
    w.add_tiles(0, list(range(12)), *streams[0])
    w.add_tiles(1, [0, 1, 2], streams[1][0], streams[1][1][:4], streams[1][2][:3])
    w.add_tiles(2, [0], *streams[2])
    with pytest.raises(ValueError, match=r"level 1 lacks 1 of its 4 tiles"):
        w.close()
    assert not os.path.exists(str(path)) and not os.path.exists(str(path) + ".part")
    for bad in (24, 528, 8, 0):
        with pytest.raises(ValueError, match="multiple of 16 in 16 .. 512"):
            PyramidWriter(str(tmp_path / "bad.tif"), 100, 100, bad, 75, 2)
    with pytest.raises(ValueError, match="quality"):
        PyramidWriter(str(tmp_path / "bad.tif"), 100, 100, 64, 0, 2)
    assert not os.path.exists(str(tmp_path / "bad.tif.part"))


def test_the_writer_needs_no_torch():
    import subprocess

    from conftest import ROOT

    code = "import sys; import cerberus_amd.tiff_pyramid as t; t.PyramidWriter; assert 'torch' not in sys.modules, 'torch was imported'"
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]


def test_level_sizes_and_the_halved_widths():
    from cerberus_amd.tiff_pyramid import level_sizes
    from cerberus_amd.viz import DEFAULT_VIZ_INFO, half_width_viz_info, pyramid_windows

    assert level_sizes(200, 150, 64) == [(200, 150), (100, 75), (50, 38)]
    assert level_sizes(64, 64, 64) == [(64, 64)] and level_sizes(65, 3, 64) == [(65, 3), (33, 2)]
    hv = half_width_viz_info()
    assert [hv[k]["line_width"] for k in ("gland", "lumen", "nuclei")] == [6, 6, 1] and DEFAULT_VIZ_INFO["gland"]["line_width"] == 12
    assert hv["nuclei"]["type_colour"] == DEFAULT_VIZ_INFO["nuclei"]["type_colour"]
    wins = pyramid_windows(40000, 1000, 256, 512)
    assert wins == [(0, 0, 32768, 512), (32768, 0, 40000, 512), (0, 512, 32768, 1000), (32768, 512, 40000, 1000)]
    assert all(x0 % 512 == 0 and y0 % 512 == 0 for x0, y0, _, _ in wins)


def test_the_option_parses_and_defaults_to_off(tmp_path):
    from cerberus_amd.cli import WSI_DRIVER_OPTIONS, WSI_OUTPUT_OPTIONS, parse

    assert WSI_OUTPUT_OPTIONS[-1][:3] == ("--save_overlay_tiff", False, False)
    assert parse("run_infer_wsi.py", WSI_DRIVER_OPTIONS, [])["--save_overlay_tiff"] is False
    a = parse("run_infer_wsi.py", WSI_DRIVER_OPTIONS, ["--save_overlay_tiff"])
    assert a["--save_overlay_tiff"] is True and a["--save_overlay"] is False and a["--overlay_encode"] == "host"
    import run_infer_wsi

    (tmp_path / "in").mkdir()
    (tmp_path / "in" / "s.txt").write_text("synthetic:600x700:3")
    with pytest.raises(ValueError, match=r"--save_overlay_tiff: s\.txt is a synthetic slide spec"):
        run_infer_wsi.main(["--synthetic", "--input_dir=%s" % (tmp_path / "in"), "--output_dir=%s" % (tmp_path / "out"), "--wsi_file_ext=.txt", "--save_overlay_tiff"])
