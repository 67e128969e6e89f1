"""The JPEG encoder's definition without a GPU: the numpy restatement (tests/jpeg_enc_ref.py) of what csrc/jpeg_encode.hip computes must equal PIL /
libjpeg-turbo -- coefficient for coefficient, table for table, and byte for byte in the scan against save(..., restart_marker_rows=1).  The device
tests (tests/test_jpeg_encode_gpu.py) then hold the kernels to the restatement."""
import os

import numpy as np
import pytest

import jpeg_enc_ref as er
from conftest import GOLDEN

from cerberus_amd import jpeg_device as jd

CASES = er.cases()
IDS = [c[0] for c in CASES]


def _pil_coefs(img, q, ss, restart_rows=0):
    rc, hdr, co = jd.decode_stream(er.pil_encode(img, q, ss, restart_rows))
    assert rc == jd.OK, rc
    return hdr, co


@pytest.mark.parametrize("name,img,q,ss", CASES, ids=IDS)
def test_restatement_equals_pil(name, img, q, ss):
    """1. coefficients and both tables equal the entropy decoder's reading of PIL's file, element for element; 2. the restatement's complete file opens
    in PIL to exactly the pixels PIL decodes from its own file; 3. its scan decodes to its own coefficients; 4. its entropy-coded bytes equal those of
    PIL's save(..., restart_marker_rows=1)"""
    h, w = img.shape[:2]
    co, ql, qc = er.coefficients(img, q, ss)
    hdr, pil_co = _pil_coefs(img, q, ss)
    assert np.array_equal(np.array(hdr.q[0][:], np.uint16), ql) and np.array_equal(np.array(hdr.q[1][:], np.uint16), qc)
    assert np.array_equal(np.array(hdr.q[2][:], np.uint16), qc)
    assert pil_co.shape == co.shape and np.array_equal(pil_co, co), int((pil_co != co).sum())
    mine = er.headers(h, w, q, ss) + er.scan(co, h, w, ss) + b"\xff\xd9"
    assert np.array_equal(er.pil_decode(mine), er.pil_decode(er.pil_encode(img, q, ss)))
    rc, h2, c2 = jd.decode_stream(mine)
    assert rc == jd.OK and (h2.width, h2.height, h2.h[0], h2.v[0]) == (w, h, 2 if ss == 2 else 1, 2 if ss == 2 else 1) and np.array_equal(c2, co)
    assert er.scan_of(mine) == er.scan_of(er.pil_encode(img, q, ss, restart_rows=1))


def _case(name):
    return CASES[IDS.index(name)]


def _symbols(blk):
    """(largest zero run in front of a non-zero AC term, in zig-zag order)"""
    run = best = 0
    for k in range(1, 64):
        if blk[er.ZIGZAG[k]] == 0:
            run += 1
        else:
            best, run = max(best, run), 0
    return best


def test_structured_pictures_take_the_paths_they_are_named_for():
    """black: EOB-only blocks; checker8: a DC difference of category 11; one_high_term: zero runs past 16 (ZRL); ff_bytes: stuffed FF bytes in the scan;
    240 x 240 at 4:4:4: RST0 .. RST7 three times over"""
    for ss in (0, 2):
        _, img, q, _ = _case("black_ss%d" % ss)
        co, _, _ = er.coefficients(img, q, ss)
        blocks = co.reshape(-1, 64)
        assert not blocks[:, 1:].any()
        _, img, q, _ = _case("checker8_q100_ss%d" % ss)
        co, _, _ = er.coefficients(img, q, ss)
        s, mr, mc = er.geometry(img.shape[0], img.shape[1], ss)
        y = co[: mr * s * mc * s * 64].reshape(mr * s, mc * s, 64)[..., 0].astype(np.int64)
        assert np.abs(np.diff(y, axis=1)).max() >= 1024  # bit length 11
        _, img, q, _ = _case("one_high_term_q100_ss%d" % ss)
        co, _, _ = er.coefficients(img, q, ss)
        assert max(_symbols(b) for b in co.reshape(-1, 64)) >= 16
        _, img, q, _ = _case("ff_bytes_ss%d" % ss)
        co, _, _ = er.coefficients(img, q, ss)
        assert b"\xff\x00" in er.scan(co, img.shape[0], img.shape[1], ss)
    _, img, q, ss = _case("240x240_ss0_q75")
    co, _, _ = er.coefficients(img, q, ss)
    sc = er.scan(co, 240, 240, ss)
    marks = [sc[i + 1] for i in range(len(sc) - 1) if sc[i] == 0xFF and 0xD0 <= sc[i + 1] <= 0xD7]
    assert marks == [0xD0 + r % 8 for r in range(29)]


def test_capacity_bound_holds_for_the_longest_codes():
    """the bound the kernels' slots come from: the longest DC code + 11 magnitude bits and 63 x (the longest AC code + 10) is 1660 bits, and no symbol
    of category <= 10 (AC) / <= 11 (DC) is missing from a table"""
    longest = 0
    for dc, ac in ((er.DC_LUMA, er.AC_LUMA), (er.DC_CHROMA, er.AC_CHROMA)):
        dcc, acc = er.huff_codes(*dc), er.huff_codes(*ac)
        assert sorted(dcc) == list(range(12)) and all(((r << 4) | s) in acc for r in range(16) for s in range(1, 11)) and 0x00 in acc and 0xF0 in acc
        longest = max(longest, max(n for _, n in dcc.values()) + 11 + 63 * (max(n for _, n in acc.values()) + 10))
    assert longest <= 1660 and (1660 + 7) // 8 == 208


def test_restatement_equals_the_fixture():
    z = np.load(os.path.join(GOLDEN, "jpeg_encode.npz"))
    assert len(z["names"]) >= 6
    for name in z["names"]:
        co, ql, qc = er.coefficients(z["picture_" + name], int(z["quality_" + name]), int(z["subsampling_" + name]))
        assert np.array_equal(co, z["coefs_" + name]) and np.array_equal(ql, z["qluma_" + name]) and np.array_equal(qc, z["qchroma_" + name]), name


def test_this_pil_writes_the_fixture_coefficients():
    """If THIS fails and the test above passes, the libjpeg behind this machine's PIL encodes differently from the one the fixture was captured with
    (PIL %s): the tests that compare with the live PIL then fail for that reason, not because of the native encoder."""
    z = np.load(os.path.join(GOLDEN, "jpeg_encode.npz"))
    for name in z["names"]:
        hdr, co = _pil_coefs(z["picture_" + name], int(z["quality_" + name]), int(z["subsampling_" + name]))
        assert np.array_equal(co, z["coefs_" + name]) and np.array_equal(np.array(hdr.q[0][:], np.uint16), z["qluma_" + name]), \
            "%s: this PIL / libjpeg encodes differently from PIL %s" % (name, z["pil_version"])


def test_package_header_writer_equals_the_restatements():
    from cerberus_amd import jpeg_encode as je

    for (h, w) in er.SIZES + [(5000, 5000), (32768, 1)]:
        for ss in (0, 2):
            for q in (1, 30, 50, 75, 100):
                assert je.headers(w, h, q, ss) == er.headers(h, w, q, ss)
    for q in (0, 101):
        with pytest.raises(ValueError, match="quality"):
            je.quant_tables(q)
