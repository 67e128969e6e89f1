"""Tile streams, windows and the pyramid on the MI355X: cerb_jpeg_enc_tiles (csrc/jpeg_encode.hip) through tiff_pyramid.TileEncoder against the numpy
restatement (tests/tiff_pyramid_ref.py) byte for byte, the capacity rule and the refusals through the C ABI, windows of the contour rasteriser against the
whole picture, viz.slide_overlay_pyramid end to end against PIL's pixels, and `run_infer_wsi.py --save_overlay_tiff`."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import tiff_pyramid_ref as tr
from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = tr.cases()
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _want(i):
    _, img, tile, q, ss = CASES[i]
    return tr.tile_streams(tr.pad_edge(img, tile), tile, q, ss)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_tile_streams_equal_the_restatement_byte_for_byte(i):
    import torch

    from cerberus_amd.tiff_pyramid import TileEncoder

    _, img, tile, q, ss = CASES[i]
    padded = tr.pad_edge(img, tile)
    data, offsets, counts = _want(i)
    enc = TileEncoder("cuda", padded.shape[1], padded.shape[0], tile)
    got, got_off, got_cnt = enc.encode(torch.from_numpy(padded).cuda(), q, ss).tiles()
    assert np.array_equal(got_off, offsets) and np.array_equal(got_cnt, counts)
    assert not (got_off & 1).any() and int(got_off[-1]) == len(data)
    got = bytes(got)
    assert len(got) == len(data) and got == data
    for o, c, nxt in zip(got_off[:-1], got_cnt, got_off[1:]):
        assert nxt - o - c in (0, 1) and (nxt - o - c == 0 or got[o + c] == 0)


def _through_the_abi(padded, tile, q, ss, cap=None, ws_short=0, w=None, out_fill=0xAA):
    """cerb_jpeg_enc_coefs + cerb_jpeg_enc_tiles -> (return code, out with 64 bytes behind the capacity, offsets, counts)"""
    import torch

    from cerberus_amd import _lib
    from cerberus_amd.tiff_pyramid import tile_prefix

    L = _lib.lib()
    h, pw = padded.shape[:2]
    w = pw if w is None else w
    planes, coefs = (int(L.cerb_jpeg_enc_workspace_bytes(pw, h, ss, k)) for k in (0, 1))
    ws_b, full = (int(L.cerb_jpeg_enc_tiles_workspace_bytes(pw, h, tile if 16 <= tile <= 512 and tile % 16 == 0 else 16, ss, k)) for k in (0, 1))
    cap = full if cap is None else cap
    n = max(1, (pw // tile) * (h // tile))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pic = torch.from_numpy(padded).cuda()
    pl = torch.empty((planes,), dtype=torch.uint8, device="cuda")
    co = torch.empty((coefs // 2,), dtype=torch.int16, device="cuda")
    ws = torch.empty((ws_b,), dtype=torch.uint8, device="cuda")
    out = torch.full((cap + 64,), out_fill, dtype=torch.uint8, device="cuda")
    off = torch.full((n + 1,), -1, dtype=torch.int64, device="cuda")
    cnt = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    _lib.check(L.cerb_jpeg_enc_coefs(pic.data_ptr(), pic.stride(0), pw, h, q, ss, co.data_ptr(), None, pl.data_ptr(), pl.numel(), st))
    prefix = tile_prefix(tile, ss) if 16 <= tile <= 512 else b"\0" * 41
    rc = L.cerb_jpeg_enc_tiles(co.data_ptr(), w, h, tile, ss, prefix, len(prefix), ws.data_ptr(), ws.numel() - ws_short, out.data_ptr(), cap, off.data_ptr(),
                               cnt.data_ptr(), st)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), off.cpu().numpy(), cnt.cpu().numpy()


def test_half_the_capacity_reports_the_full_total_and_writes_nothing_behind_it():
    _, img, tile, q, ss = CASES[4]
    data, offsets, counts = _want(4)
    cap = len(data) // 2
    rc, out, off, cnt = _through_the_abi(tr.pad_edge(img, tile), tile, q, ss, cap=cap)
    assert rc == 0 and np.array_equal(off, offsets) and np.array_equal(cnt, counts) and int(off[-1]) == len(data)
    assert out[:cap].tobytes() == data[:cap] and (out[cap:] == 0xAA).all()
    rc, out, off, cnt = _through_the_abi(tr.pad_edge(img, tile), tile, q, ss)  # and with the capacity that never truncates: everything, nothing behind
    assert rc == 0 and out[:len(data)].tobytes() == data and (out[-64:] == 0xAA).all()


def test_refusals_come_before_any_launch():
    from cerberus_amd import _lib

    L = _lib.lib()
    _, img, tile, q, ss = CASES[4]
    padded = tr.pad_edge(img, tile)  # 192 x 256
    for kw, word in ((dict(w=200), "multiples of tile"), (dict(tile=24), "tile must be a multiple of 16"), (dict(tile=528), "tile must be a multiple of 16"),
                     (dict(ws_short=1), "workspace is too small")):
        args = dict(tile=tile)
        args.update(kw)
        rc, out, off, cnt = _through_the_abi(padded, args.pop("tile"), q, ss, **args)
        assert rc == 1 and word in L.cerb_last_error().decode(), (kw, L.cerb_last_error())
        assert (out == 0xAA).all() and (off == -1).all() and (cnt == -1).all()  # nothing ran
    assert L.cerb_jpeg_enc_tiles_workspace_bytes(200, 192, 64, 2, 0) == 0 and L.cerb_jpeg_enc_tiles_workspace_bytes(256, 192, 24, 2, 1) == 0
    assert L.cerb_jpeg_enc_tiles_workspace_bytes(256, 192, 64, 2, 0) > 0 and L.cerb_jpeg_enc_tiles_workspace_bytes(256, 192, 64, 2, 1) > 0


def _picture(h, w, seed):
    import jpeg_ref

    return jpeg_ref.image(h, w, seed)


def test_windows_drawn_through_the_origin_assemble_to_the_whole_picture():
    import torch

    from cerberus_amd.viz import draw_contours_device

    img = torch.from_numpy(_picture(96, 128, 11)).cuda()
    groups = tr.contours()
    whole = draw_contours_device(img, groups)
    assert (whole != img).any(dim=2).sum().item() > 500  # strokes are on it
    got = torch.zeros_like(whole)
    for y0 in range(0, 96, 32):
        for x0 in range(0, 128, 64):
            got[y0:y0 + 32, x0:x0 + 64] = draw_contours_device(img[y0:y0 + 32, x0:x0 + 64], [dict(g, origin=(x0, y0)) for g in groups])
    assert torch.equal(got, whole), int((got != whole).any(dim=2).sum().item())


def _slide_parts(scale=1):
    """the contours of tiff_pyramid_ref as the instance arrays of a slide: nuclei as a `parts` entry, glands as ready dictionaries in `extra`"""
    g = tr.contours()
    nuc = np.concatenate([g[2]["points"], g[1]["points"] + (150, 120)]) * scale
    cnts = np.concatenate([g[2]["counts"], g[1]["counts"]]).astype(np.int32)
    offs = np.cumsum(cnts, dtype=np.int64) - cnts
    tab = np.ones((len(cnts), 8), np.int64)
    parts = [("Nuclei", tab, cnts, nuc, offs, False, 1.0)]
    gl = g[0]
    extra = {"Gland": {"g%d" % i: {"contour": (gl["points"][o:o + c] * (3, 2) + (20, 60)) * scale} for i, (o, c) in enumerate(zip(gl["offsets"], gl["counts"]))}}
    return parts, extra


def test_slide_overlay_pyramid_end_to_end_equals_pils_pixels_level_by_level(tmp_path):
    from PIL import Image

    from cerberus_amd.reader import ArrayReader, TiffReader
    from cerberus_amd.viz import draw_contours_device, half_width_viz_info, pack_parts, slide_overlay_pyramid

    slide = _picture(300, 420, 12)
    parts, extra = _slide_parts()
    path = str(tmp_path / "s.tif")
    sizes = slide_overlay_pyramid(ArrayReader(slide), 0.5, parts, extra, path, tile=64, window_rows=128)
    assert sizes == [(420, 300), (210, 150), (105, 75), (53, 38)]
    level = draw_contours_device(slide, pack_parts(parts, extra, half_width_viz_info(), ds=1)).cpu().numpy()
    assert (level != slide).any(axis=2).sum() > 1000
    im = Image.open(path)
    assert im.n_frames == len(sizes)
    r = TiffReader(path)
    assert r.big and [tuple(d) for d in r.info.level_dimensions] == sizes
    for k in range(len(sizes)):
        if k:
            level = tr.box2(level)
        im.seek(k)
        got, want = np.asarray(im.convert("RGB")), tr.expected_pixels(level, 64)
        assert got.shape == want.shape == (sizes[k][1], sizes[k][0], 3)
        assert np.array_equal(got, want), (k, int((got != want).any(axis=2).sum()))
    assert not os.path.exists(path + ".part")


def test_a_slide_that_does_not_fit_is_refused_with_the_bytes(tmp_path, monkeypatch):
    import torch

    from cerberus_amd.reader import ArrayReader
    from cerberus_amd.viz import slide_overlay_pyramid

    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (1 << 20, 1 << 30))
    with pytest.raises(ValueError, match=r"needs \d+ bytes on the device with the smallest window \(128 rows\).*1048576 are free"):
        slide_overlay_pyramid(ArrayReader(_picture(300, 420, 12)), 0.5, [], None, str(tmp_path / "s.tif"), tile=64)
    assert os.listdir(str(tmp_path)) == []


def test_run_infer_wsi_save_overlay_tiff_writes_the_pyramid_and_the_same_dat(tmp_path):
    import joblib
    from PIL import Image

    from cerberus_amd.reader import TiffReader
    from cerberus_amd.wsi import synth_slide

    slides = tmp_path / "slides"
    slides.mkdir()
    Image.fromarray(synth_slide(530, 610, seed=5).cpu().numpy()).save(str(slides / "s1.png"))
    outs = {}
    for mode, flags in (("plain", []), ("tiff", ["--save_overlay_tiff"])):
        outs[mode] = tmp_path / ("out_" + mode)
        cmd = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % slides, "--wsi_file_ext=.png", "--output_dir=%s" % outs[mode],
               "--logging_dir=%s" % (tmp_path / ("log_" + mode)), "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256"] + flags
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
    assert not (outs["plain"] / "overlay").exists() and not (outs["tiff"] / "overlay" / "s1.jpg").exists()
    path = str(outs["tiff"] / "overlay" / "s1.tif")
    r = TiffReader(path)
    assert r.big and tuple(r.info.level_dimensions[0]) == (610, 530) and [tuple(d) for d in r.info.level_dimensions[1:]] == [(305, 265), (153, 133)]
    im = Image.open(path)
    assert im.n_frames == 3 and im.size == (610, 530)
    log = "".join(open(str(p)).read() for p in (tmp_path / "log_tiff").iterdir())
    assert "Overlay TIFF Time" in log
    # the dictionary does not depend on the flag.  (Its keys are fresh uuids in every run, so two files are never equal byte for byte -- not even two
    # runs of the same command line: the instances themselves are compared, field by field and bit for bit, as tests/test_jpeg_encode_cli_gpu.py does.)
    da, db = (joblib.load(str(outs[m] / "dat" / "s1.dat")) for m in ("plain", "tiff"))
    assert sorted(da) == sorted(db)

    def canon(insts):
        return sorted(tuple((f, v.dtype.str + str(v.shape), v.tobytes()) if isinstance(v, np.ndarray) else (f, repr(v), b"") for f, v in sorted(d.items()))
                      for d in insts.values())

    n = 0
    for t in ("Nuclei", "Gland", "Lumen"):
        assert canon(da[t]) == canon(db[t]), t
        n += len(da[t])
    print("instances:", n)
