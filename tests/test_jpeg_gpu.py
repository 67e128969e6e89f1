"""The device half of the JPEG path on the MI355X (csrc/jpeg_kernels.hip through cerberus_amd/jpeg_device.py and wsi.SlabUploader): PIL's bytes, bit for
bit -- every comparison is array_equal -- and no tile of these inputs falls back to PIL unless the test says so."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import jpeg_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _device_decode(items, tw, th, window, dst_rows, dst_stride, byte_off=0):
    """items [(hdr, coefs, gx0, gy0)] through cerb_jpeg_decode_window into a 0xAA-filled destination of dst_rows x dst_stride bytes whose window starts
    byte_off bytes in -> the whole destination as a numpy array"""
    import torch

    from cerberus_amd import _lib
    from cerberus_amd import jpeg_device as jd

    buf = torch.from_numpy(jd.pack_stream_buffer(items)).cuda()
    scratch = torch.empty((max(8, jd.workspace_bytes(len(items), tw, th)[1]),), dtype=torch.uint8, device="cuda")
    dst = torch.full((dst_rows * dst_stride + 64,), 0xAA, dtype=torch.uint8, device="cuda")
    x0, y0, x1, y1 = window
    st = torch.cuda.current_stream()
    _lib.check(_lib.lib().cerb_jpeg_decode_window(buf.data_ptr(), buf.numel(), len(items), tw, th, scratch.data_ptr(), scratch.numel(),
                                                  dst.data_ptr() + byte_off, dst_stride, x0, y0, x1, y1, C.c_void_p(st.cuda_stream)))
    torch.cuda.synchronize()
    return dst.cpu().numpy()


def _check_window(flat, want, dst_rows, dst_stride, byte_off):
    """the window's pixels are `want`, every other byte is still 0xAA"""
    h, w = want.shape[:2]
    body = flat[byte_off: byte_off + dst_rows * dst_stride].reshape(dst_rows, dst_stride)
    assert np.array_equal(body[:h, : w * 3].reshape(h, w, 3), want), int((body[:h, : w * 3].reshape(h, w, 3) != want).sum())
    mask = np.ones(flat.shape, bool)
    for r in range(h):
        mask[byte_off + r * dst_stride: byte_off + r * dst_stride + w * 3] = False
    assert (flat[mask] == 0xAA).all()


CASES = jpeg_ref.cases()


@pytest.mark.parametrize("byte_off", [0, 5], ids=["aligned", "unaligned"])
def test_device_half_equals_pil_on_the_host_tests_streams(byte_off):
    """every stream of tests/test_jpeg_host.py (sizes 16 x 16 .. 240 x 240, odd ones, 4:4:4 / 4:2:2 / 4:2:0, restarts, tables, photometric 2, R G B ids),
    into a destination whose rows are wider than the window and prefilled with 0xAA; once with a 4-byte aligned destination (the 12-byte stores) and
    once 5 bytes in (the byte stores)"""
    from cerberus_amd import jpeg_device as jd

    for name, data, tabs, ph in CASES:
        rc, hdr, co = jd.decode_stream(data, tabs, ph)
        assert rc == jd.OK
        want = jpeg_ref.pil_pixels(data, tabs, ph)
        h, w = want.shape[:2]
        stride = (w * 3 + 3) // 4 * 4 + 24
        flat = _device_decode([(hdr, co, 0, 0)], w, h, (0, 0, w, h), h + 2, stride, byte_off)
        _check_window(flat, want, h + 2, stride, byte_off)


@pytest.mark.parametrize("window", [(0, 0, 192, 128), (5, 7, 150, 101), (64, 64, 65, 65)])
def test_window_placement_over_a_grid_of_tiles(window):
    """3 x 2 tiles of 64 x 64, 4:2:0: the window's pixels are the crop of the PIL-decoded mosaic, nothing else is written"""
    from cerberus_amd import jpeg_device as jd

    img = jpeg_ref.image(128, 192, 33)
    items, mosaic = [], np.zeros((128, 192, 3), np.uint8)
    for ty in range(2):
        for tx in range(3):
            data = jpeg_ref.encode(img[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64], 90, 2)
            rc, hdr, co = jd.decode_stream(data)
            assert rc == jd.OK
            items.append((hdr, co, tx * 64, ty * 64))
            mosaic[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64] = jpeg_ref.pil_pixels(data)
    x0, y0, x1, y1 = window
    stride = (x1 - x0) * 3 + 17
    flat = _device_decode(items, 64, 64, window, y1 - y0 + 1, stride, 4)
    _check_window(flat, mosaic[y0:y1, x0:x1], y1 - y0 + 1, stride, 4)


def test_decode_window_of_a_tiff_level_equals_the_reader(tmp_path):
    import torch

    from cerberus_amd import jpeg_device as jd
    from cerberus_amd.reader import TiffReader

    r = TiffReader(jpeg_ref.write_jpeg_tiff(str(tmp_path / "s.tif"), [jpeg_ref.image(200, 330, 41)]))
    p = r.levels[0]
    assert jd.level_supported(r, 0)
    jd.reset_counters()
    for win in ((0, 0, p.w, p.h), (13, 21, 301, 187)):
        x0, y0, x1, y1 = win
        dst = torch.full((y1 - y0, x1 - x0 + 3, 3), 0xAA, dtype=torch.uint8, device="cuda")[:, : x1 - x0]
        back = jd.decode_window(r, 0, x0, y0, x1, y1, dst, torch.cuda.current_stream())
        torch.cuda.synchronize()
        assert back == []
        assert np.array_equal(dst.cpu().numpy(), r._read_level(0, x0, y0, x1, y1))
    c = jd.counters()
    assert c["fallback"] == 0 and c["native"] == 24 + 15


def _slab(rows, H, chunk_bytes, device_jpeg, monkeypatch):
    import torch

    from cerberus_amd.wsi import SlabUploader

    if device_jpeg:
        monkeypatch.setenv("CERB_JPEG_DECODE", "device")
    else:
        monkeypatch.delenv("CERB_JPEG_DECODE", raising=False)
    up = SlabUploader(rows, 0, H, chunk_bytes=chunk_bytes)
    assert (up.jpeg is not None) == bool(device_jpeg)
    up.upload_until(H)
    torch.cuda.synchronize()
    out = up.slab.cpu().numpy()
    assert up.k >= 3, up.k  # at least three chunks
    up.close()
    return out


def test_slab_uploader_device_jpeg_equals_the_default_path(tmp_path, monkeypatch):
    from cerberus_amd import jpeg_device as jd
    from cerberus_amd.reader import TiffReader

    path = jpeg_ref.write_jpeg_tiff(str(tmp_path / "s.tif"), [jpeg_ref.image(200, 330, 41)])
    r = TiffReader(path)
    rows = r.rows(1.0, "baseline")
    want = _slab(rows, 200, 64 * 330 * 3, False, monkeypatch)
    jd.reset_counters()
    got = _slab(TiffReader(path).rows(1.0, "baseline"), 200, 64 * 330 * 3, True, monkeypatch)
    assert np.array_equal(got, want)
    assert jd.counters()["fallback"] == 0 and jd.counters()["native"] >= 24


def _two_level_tiff(tmp_path):
    base = jpeg_ref.image(300, 428, 51)
    return jpeg_ref.write_jpeg_tiff(str(tmp_path / "two.tif"), [base, np.ascontiguousarray(base[::4, ::4])], ss=1, mpp=0.25)


def test_slab_uploader_device_jpeg_under_the_integer_reduction(tmp_path, monkeypatch):
    """a file stored at 0.25 mpp read at 0.5: level 0's tiles are decoded on the device into the staging buffer and cerb_resample_box runs unchanged"""
    from cerberus_amd import jpeg_device as jd
    from cerberus_amd.reader import TiffReader

    path = _two_level_tiff(tmp_path)
    rows = TiffReader(path).rows(0.5, "mpp")
    H = rows.shape[0]
    assert rows.device_plan().k == 2
    want = _slab(rows, H, 4096, False, monkeypatch)
    jd.reset_counters()
    got = _slab(TiffReader(path).rows(0.5, "mpp"), H, 4096, True, monkeypatch)
    assert np.array_equal(got, want)
    assert np.array_equal(want, TiffReader(path).read_bounds((0, 0, rows.shape[1], H), 0.5, "mpp"))
    assert jd.counters()["fallback"] == 0 and jd.counters()["native"] >= 35


def test_a_progressive_tile_falls_back_alone(tmp_path, monkeypatch):
    from cerberus_amd import jpeg_device as jd
    from cerberus_amd.reader import TiffReader

    path = jpeg_ref.write_jpeg_tiff(str(tmp_path / "s.tif"), [jpeg_ref.image(200, 330, 41)], progressive_at=9)
    want = _slab(TiffReader(path).rows(1.0, "baseline"), 200, 64 * 330 * 3, False, monkeypatch)
    assert np.array_equal(want, TiffReader(path)._read_level(0, 0, 0, 330, 200))
    jd.reset_counters()
    # one chunk per tile row of 64: every tile is decoded exactly once
    got = _slab(TiffReader(path).rows(1.0, "baseline"), 200, 64 * 330 * 3, True, monkeypatch)
    assert np.array_equal(got, want)
    assert jd.counters() == {"native": 23, "fallback": 1}


def test_run_infer_wsi_jpeg_decode_device_writes_the_same_dat(tmp_path):
    import joblib

    d = tmp_path / "in"
    d.mkdir()
    jpeg_ref.write_jpeg_tiff(str(d / "s1.tif"), [jpeg_ref.image(512, 512, 61)], tile=128)
    outs = []
    for mode in ("host", "device"):
        out = tmp_path / mode
        r = subprocess.run([sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % d, "--wsi_file_ext=.tif", "--output_dir=%s" % out,
                            "--batch_size=4", "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps", "--jpeg_decode=%s" % mode],
                           capture_output=True, text=True, timeout=600, cwd=ROOT, env={k: v for k, v in os.environ.items() if k != "CERB_JPEG_DECODE"})
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(out)
    za, zb = np.load(str(outs[0] / "s1.npz")), np.load(str(outs[1] / "s1.npz"))
    assert set(za.files) == set(zb.files)
    for k in za.files:
        assert np.array_equal(za[k], zb[k]), k
    da, db = joblib.load(str(outs[0] / "dat" / "s1.dat")), joblib.load(str(outs[1] / "dat" / "s1.dat"))
    assert set(da.keys()) == set(db.keys())

    def same(a, b):
        if isinstance(a, dict) and a and all(isinstance(e, dict) and "box" in e for e in a.values()):  # instances under random uuid keys
            def flat(v):
                return sorted((tuple(np.asarray(e["box"]).ravel().tolist()), tuple(np.asarray(e["centroid"]).ravel().tolist()),
                               np.asarray(e["contour"]).tobytes(), repr(e.get("type")), repr(e.get("type_prob"))) for e in v.values())
            return flat(a) == flat(b)
        if isinstance(a, dict):
            return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
        if isinstance(a, np.ndarray):
            return np.array_equal(a, b)
        return a == b

    for k in da:
        assert same(da[k], db[k]), k
    assert sum(len(v) for v in da.values() if isinstance(v, dict)) > 4
