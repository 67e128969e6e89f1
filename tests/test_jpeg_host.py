"""The host half of the JPEG device path without a GPU: the C entropy decoder (csrc/jpeg_entropy.h through cerb_jpeg_decode_stream /
cerb_jpeg_read_tiles) feeding the numpy statement of the device arithmetic (tests/jpeg_ref.py) must equal PIL byte for byte; what it does not take
is "unsupported", what is broken is "corrupt", and nothing crashes -- also under the host sanitizers, in a stand-alone program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_ref
from conftest import GOLDEN, ROOT

from cerberus_amd import jpeg_device as jd

CASES = jpeg_ref.cases()


def _decode(data, tabs, ph, cap=None):
    rc, hdr, co = jd.decode_stream(data, tabs, ph, coef_cap=cap)
    assert rc == jd.OK, rc
    return jpeg_ref.decode(hdr, co)


@pytest.mark.parametrize("name,data,tabs,ph", CASES, ids=[c[0] for c in CASES])
def test_entropy_decoder_plus_numpy_arithmetic_equals_pil(name, data, tabs, ph):
    """sizes 16x16 .. 240x240 (odd ones included), 4:4:4 / 4:2:2 / 4:2:0, quality 30 and 95, restart interval 3, tables + abbreviated stream,
    photometric 2 (Adobe transform 0 forced, JFIF dropped), component ids R G B, Adobe transform 1: array_equal, no tolerance"""
    want = jpeg_ref.pil_pixels(data, tabs, ph)
    got = _decode(data, tabs, ph)
    assert got.shape == want.shape and np.array_equal(got, want), (name, int((got != want).sum()))


def test_fixture_streams_decode_to_the_fixture_pixels():
    z = np.load(os.path.join(GOLDEN, "jpeg_tiles.npz"))
    for name in z["names"]:
        tabs = z["tables_" + name].tobytes() or None
        got = _decode(z["stream_" + name].tobytes(), tabs, int(z["photometric_" + name]))
        assert np.array_equal(got, z["pixels_" + name]), name


def test_this_pil_returns_the_fixture_pixels():
    """If THIS fails and the test above passes, the libjpeg behind this machine's PIL decodes differently from the one the fixture was captured with
    (PIL %s): the tests that compare with the live PIL then fail for that reason, not because of the native decoder."""
    z = np.load(os.path.join(GOLDEN, "jpeg_tiles.npz"))
    for name in z["names"]:
        tabs = z["tables_" + name].tobytes() or None
        live = jpeg_ref.pil_pixels(z["stream_" + name].tobytes(), tabs, int(z["photometric_" + name]))
        assert np.array_equal(live, z["pixels_" + name]), "%s: this PIL / libjpeg decodes differently from PIL %s" % (name, z["pil_version"])


def _sof_patch(data, hv):
    """the first component's sampling byte of the frame header replaced"""
    d = bytearray(data)
    for m, a, b in jpeg_ref.segments(data):
        if m == 0xC0:
            d[a + 4 + 6 + 1] = hv
    return bytes(d)


def test_streams_outside_the_accepted_set_are_unsupported():
    img = jpeg_ref.image(64, 64, 1)
    assert jd.decode_stream(jpeg_ref.encode(img, progressive=True))[0] == jd.UNSUPPORTED
    assert jd.decode_stream(jpeg_ref.encode(img, mode="L"))[0] == jd.UNSUPPORTED
    assert jd.decode_stream(_sof_patch(jpeg_ref.encode(img, subsampling=0), 0x12))[0] == jd.UNSUPPORTED  # 4:4:0
    assert jd.decode_stream(_sof_patch(jpeg_ref.encode(img, subsampling=0), 0x41))[0] == jd.UNSUPPORTED  # 4:1:1
    cmyk = __import__("io").BytesIO()
    from PIL import Image

    Image.fromarray(np.dstack([img, img[..., :1]]), "CMYK").save(cmyk, format="JPEG")
    assert jd.decode_stream(cmyk.getvalue())[0] == jd.UNSUPPORTED


def test_truncations_and_corruptions_are_corrupt_or_decode():
    """16 seeded prefix truncations and 64 seeded single-byte corruptions of a 64 x 64 stream: "corrupt" or a full decode, never a crash.  One more
    outcome exists by the decoder's own rules and only for a corrupted byte INSIDE the marker segments: the byte can turn the frame into one the
    decoder must call unsupported (SOF0 -> SOF2, another sampling factor) or into a larger frame than the caller's capacity -- accepted there and
    nowhere else; a corrupted byte of the entropy-coded data must give corrupt or a full decode."""
    data = jpeg_ref.encode(jpeg_ref.image(64, 64, 7), 90, 2, restart=3)
    scan = jpeg_ref.segments(data)[-1][2]
    cap = 3 * 64 * 64
    full = 64 * 64 * 3 // 2
    rng = np.random.RandomState(5)
    for cut in sorted(rng.randint(0, len(data), 16)):
        rc, _, co = jd.decode_stream(data[:cut], coef_cap=cap)
        assert rc in (jd.CORRUPT, jd.OK), (cut, rc)
        assert rc == jd.CORRUPT or (co.size == full and cut > scan)
    seen = set()
    for pos, val in zip(rng.randint(0, len(data), 64), rng.randint(1, 256, 64)):
        bad = bytearray(data)
        bad[pos] ^= int(val)
        rc, _, co = jd.decode_stream(bytes(bad), coef_cap=cap)
        seen.add(rc)
        if pos >= scan:
            assert rc in (jd.CORRUPT, jd.OK), (pos, rc)
        else:
            assert rc in (jd.CORRUPT, jd.OK, jd.UNSUPPORTED, jd.TOO_LARGE), (pos, rc)
        assert rc != jd.OK or co.size > 0
    assert jd.OK in seen and jd.CORRUPT in seen
    # the named kinds of damage
    assert jd.decode_stream(data[: scan + 40], coef_cap=cap)[0] == jd.CORRUPT                                   # truncated inside the scan
    assert jd.decode_stream(data[:scan + 10] + b"\xff\xd9" + data[scan + 12:], coef_cap=cap)[0] == jd.CORRUPT  # a marker where data was expected
    nodht = b"\xff\xd8" + b"".join(data[a:b] for m, a, b in jpeg_ref.segments(data) if m != 0xC4) + data[scan:]
    assert jd.decode_stream(nodht, coef_cap=cap)[0] == jd.CORRUPT                                               # a missing table


def test_window_call_equals_per_tile_calls_and_names_the_corrupt_tile(tmp_path, monkeypatch):
    import ctypes as C

    from cerberus_amd.reader import TiffReader

    img = jpeg_ref.image(128, 192, 21)  # 3 x 2 tiles of 64
    path = jpeg_ref.write_jpeg_tiff(str(tmp_path / "s.tif"), [img])
    r = TiffReader(path)
    p = r.levels[0]
    tiles = jd.window_tiles(p, 0, 0, p.w, p.h)
    assert len(tiles) == 6
    nbytes = jd.workspace_bytes(len(tiles), p.tw, p.th)[0]
    for threads in ("1", "4"):
        monkeypatch.setenv("CERB_DECODE_THREADS", threads)
        buf = np.zeros(nbytes + 16, np.uint8)
        buf = buf[(-buf.ctypes.data) % 16:][:nbytes]
        used, uns = jd.read_tiles_host(r, 0, tiles, buf.ctypes.data, nbytes)
        assert uns == [] and used <= nbytes
        base = -(-len(tiles) * C.sizeof(jd.JpegHdr) // 256) * 256
        coefs = buf[base:used].view(np.int16)
        mosaic = np.zeros((p.h, p.w, 3), np.uint8)
        for i, (ty, tx) in enumerate(tiles):
            hdr = jd.JpegHdr.from_buffer_copy(buf[i * 464:(i + 1) * 464].tobytes())
            data = os.pread(r.fh.fileno(), p.counts[i], p.offsets[i])
            rc, h1, c1 = jd.decode_stream(data, None, p.photometric)
            assert rc == jd.OK and hdr.status == jd.OK and (hdr.gx0, hdr.gy0) == (tx * 64, ty * 64)
            assert bytes(hdr)[4:40] == bytes(h1)[4:40] and bytes(hdr)[80:] == bytes(h1)[80:]
            mine = coefs[hdr.coef_off: hdr.coef_off + c1.size]
            assert np.array_equal(mine, c1)
            mosaic[ty * 64:(ty + 1) * 64, tx * 64:(tx + 1) * 64] = jpeg_ref.decode(hdr, mine)
        assert np.array_equal(mosaic, r._read_level(0, 0, 0, p.w, p.h))
    # tile 4 damaged in the file: the call fails and names it
    bad = str(tmp_path / "bad.tif")
    shutil.copy(path, bad)
    with open(bad, "r+b") as fh:
        fh.seek(p.offsets[4] + p.counts[4] // 2)
        fh.write(b"\xff\xd9" * 8)
    rb = TiffReader(bad)
    with pytest.raises(ValueError) as e:
        jd.read_tiles_host(rb, 0, tiles, buf.ctypes.data, nbytes)
    assert "bad.tif" in str(e.value) and "tile 4" in str(e.value)


def test_entropy_decoder_under_the_host_sanitizers(tmp_path):
    """tests/tools/jpeg_entropy_main.c (its own main, includes jpeg_entropy.h) compiled with -fsanitize=address,undefined and run as a child process over
    intact streams, 16 truncations and 64 corruptions each; exit status 0 is the pass.  Nothing sanitised is loaded into this interpreter, and the
    sanitizer runtimes are linked statically: the program does not care what else the environment loads beside it."""
    cc = shutil.which(os.environ.get("CC", "gcc"))
    assert cc, "no C compiler"
    exe = str(tmp_path / "jpeg_entropy_main")
    r = subprocess.run([cc, "-O1", "-g", "-std=c99", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                        "-o", exe,
                        os.path.join(ROOT, "tests", "tools", "jpeg_entropy_main.c")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    d = tmp_path / "streams"
    d.mkdir()
    n = 0
    for name, data, tabs, ph in CASES:
        if name.startswith("240x240") and "q30" not in name:
            continue
        (d / (name + ".jpg")).write_bytes(data)
        if tabs:
            (d / (name + ".jpg.tables")).write_bytes(tabs)
        n += 1
    img = jpeg_ref.image(64, 64, 1)
    (d / "progressive.jpg").write_bytes(jpeg_ref.encode(img, progressive=True))
    (d / "grey.jpg").write_bytes(jpeg_ref.encode(img, mode="L"))
    (d / "restart.jpg").write_bytes(jpeg_ref.encode(jpeg_ref.image(64, 64, 7), 90, 2, restart=3))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-1000:], r.stderr[-3000:])
    assert r.stdout.startswith("%d files" % (n + 3))
