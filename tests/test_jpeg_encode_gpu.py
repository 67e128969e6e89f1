"""The JPEG encoder's kernels on the MI355X (csrc/jpeg_encode.hip) against the numpy restatement (tests/jpeg_enc_ref.py), all through the C ABI: equal
coefficients, tables, scan bytes and lengths -- every comparison is exact -- and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import jpeg_enc_ref as er
import jpeg_ref

pytestmark = pytest.mark.gpu

CASES = er.cases()
IDS = [c[0] for c in CASES]


@functools.lru_cache(maxsize=None)
def _want(i):
    """(coefficients, luma table, chroma table, scan) of case i from the restatement, computed once"""
    _, img, q, ss = CASES[i]
    co, ql, qc = er.coefficients(img, q, ss)
    return co, ql, qc, er.scan(co, img.shape[0], img.shape[1], ss)


def _sizes(w, h, ss):
    from cerberus_amd import _lib

    return [int(_lib.lib().cerb_jpeg_enc_workspace_bytes(w, h, ss, k)) for k in range(4)]


def _coefs(pic, q, ss, stream=None):
    """pic: uint8 device tensor [h, w, 3] (any row stride) -> (int16 coefficients, uint16 [128] tables) on the device, through cerb_jpeg_enc_coefs"""
    import torch

    from cerberus_amd import _lib

    h, w = pic.shape[:2]
    planes, coefs, _, _ = _sizes(w, h, ss)
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):  # (the fills below are queued on the stream the kernels run on)
        ws = torch.empty((planes,), dtype=torch.uint8, device="cuda")
        co = torch.full((coefs // 2,), 0x5A5A, dtype=torch.int16, device="cuda")
        qt = torch.zeros((128,), dtype=torch.int16, device="cuda")
        _lib.check(_lib.lib().cerb_jpeg_enc_coefs(pic.data_ptr(), pic.stride(0), w, h, q, ss, co.data_ptr(), qt.data_ptr(), ws.data_ptr(), ws.numel(),
                                                  C.c_void_p(st.cuda_stream)))
    return co, qt, ws


def _scan(co, w, h, ss, stream=None, cap=None):
    """coefficients -> (the scan buffer, 0xAA-filled behind the capacity, the device length word, keep-alive) through cerb_jpeg_enc_scan"""
    import torch

    from cerberus_amd import _lib

    _, _, scan_ws, scan_cap = _sizes(w, h, ss)
    cap = scan_cap if cap is None else cap
    st = stream or torch.cuda.current_stream()
    with torch.cuda.stream(st):
        ws = torch.empty((scan_ws,), dtype=torch.uint8, device="cuda")
        out = torch.full((cap + 64,), 0xAA, dtype=torch.uint8, device="cuda")
        n = torch.zeros((1,), dtype=torch.int64, device="cuda")
        _lib.check(_lib.lib().cerb_jpeg_enc_scan(co.data_ptr(), w, h, ss, ws.data_ptr(), ws.numel(), out.data_ptr(), cap, n.data_ptr(), C.c_void_p(st.cuda_stream)))
    return out, n, ws


def _device_scan(img, q, ss):
    import torch

    h, w = img.shape[:2]
    co, qt, _ = _coefs(torch.from_numpy(img).cuda(), q, ss)
    out, n, _ = _scan(co, w, h, ss)
    torch.cuda.synchronize()
    n = int(n.item())
    flat = out.cpu().numpy()
    assert (flat[_sizes(w, h, ss)[3]:] == 0xAA).all()  # nothing behind the capacity
    return co.cpu().numpy(), qt.cpu().numpy().view(np.uint16), flat[:n].tobytes(), n


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_kernels_equal_the_restatement(i):
    """every shape x sampling x quality and every structured picture: coefficients and tables array_equal, scan bytes and length equal, and the finished
    file opens in PIL to the pixels PIL decodes from its own file"""
    name, img, q, ss = CASES[i]
    co, ql, qc, scan = _want(i)
    got_co, got_qt, got_scan, n = _device_scan(img, q, ss)
    assert np.array_equal(got_qt[:64], ql) and np.array_equal(got_qt[64:], qc)
    assert got_co.shape == co.shape and np.array_equal(got_co, co), int((got_co != co).sum())
    assert n == len(scan)
    assert got_scan == scan
    from cerberus_amd import jpeg_encode as je

    h, w = img.shape[:2]
    mine = je.headers(w, h, q, ss) + got_scan + b"\xff\xd9"
    assert np.array_equal(er.pil_decode(mine), er.pil_decode(er.pil_encode(img, q, ss)))


def test_python_layer_returns_the_restatements_file():
    """Encoder.encode(...).bytes() and encode_device: the header writer of the package equals the restatement's, one encoder serves pictures of several
    sizes and both samplings, and a picture that compresses worse than the first copy allows for still arrives whole"""
    import torch

    from cerberus_amd import jpeg_encode as je

    enc = je.Encoder("cuda", 240, 240)
    second_fetch = False
    for i in (IDS.index("37x53_ss2_q75"), IDS.index("240x240_ss0_q100"), IDS.index("noise_q100_ss0"), IDS.index("17x9_ss0_q30")):
        name, img, q, ss = CASES[i]
        want = er.encode(img, q, ss)
        assert enc.encode(torch.from_numpy(img).cuda(), q, ss).bytes() == want, name
        second_fetch |= len(want) > enc._pinned.numel()
    assert second_fetch
    name, img, q, ss = CASES[IDS.index("64x200_ss2_q95")]
    assert je.encode_device(torch.from_numpy(img).cuda(), q, ss) == er.encode(img, q, ss)
    with pytest.raises(ValueError, match="quality"):
        enc.encode(torch.from_numpy(img).cuda(), 0, ss)
    with pytest.raises(ValueError, match="encoder made for"):
        enc.encode(torch.zeros((8, 300, 3), dtype=torch.uint8, device="cuda"))


@pytest.mark.parametrize("ss", [0, 2])
def test_strided_view_at_an_odd_byte_gives_the_bytes_of_its_contiguous_copy(ss):
    import torch

    img = jpeg_ref.image(37, 53, 91)
    h, w = img.shape[:2]
    stride = 3 * w + 38
    flat = torch.full((h * stride + 16,), 0x77, dtype=torch.uint8, device="cuda")
    view = flat[7:7 + h * stride].view(h, stride)[:, : 3 * w].unflatten(1, (w, 3))
    view.copy_(torch.from_numpy(img).cuda())
    assert view.data_ptr() % 2 == 1 and view.stride(0) == stride > 3 * w
    co, _, _ = _coefs(view, 75, ss)
    out, n, _ = _scan(co, w, h, ss)
    torch.cuda.synchronize()
    _, _, want, wn = _device_scan(img, 75, ss)
    assert int(n.item()) == wn and out.cpu().numpy()[:wn].tobytes() == want


@pytest.mark.parametrize("ss", [0, 2])
def test_encoder_coefficients_through_the_device_decoder_give_pils_pixels(ss):
    """closes the loop with the decoding half: cerb_jpeg_enc_coefs -> cerb_jpeg_decode_window == PIL's decode of PIL's own file"""
    import torch

    from cerberus_amd import _lib
    from cerberus_amd import jpeg_device as jd

    img = jpeg_ref.image(37, 53, 92)
    h, w = img.shape[:2]
    pil = er.pil_encode(img, 75, ss)
    rc, hdr, _ = jd.decode_stream(pil)  # (the header alone is taken from PIL's file: size, sampling, tables)
    assert rc == jd.OK
    co, qt, _ = _coefs(torch.from_numpy(img).cuda(), 75, ss)
    torch.cuda.synchronize()
    assert np.array_equal(qt.cpu().numpy().view(np.uint16)[:64], np.array(hdr.q[0][:], np.uint16))
    buf = torch.from_numpy(jd.pack_stream_buffer([(hdr, co.cpu().numpy(), 0, 0)])).cuda()
    scratch = torch.empty((max(8, jd.workspace_bytes(1, w, h)[1]),), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((h, w, 3), dtype=torch.uint8, device="cuda")
    _lib.check(_lib.lib().cerb_jpeg_decode_window(buf.data_ptr(), buf.numel(), 1, w, h, scratch.data_ptr(), scratch.numel(), dst.data_ptr(), 3 * w, 0, 0, w, h,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy(), er.pil_decode(pil))


def test_two_encodes_on_two_streams_give_identical_bytes():
    import torch

    img = jpeg_ref.image(240, 240, 93)
    pic = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    res = []
    for _ in range(2):
        st = torch.cuda.Stream()
        co, _, ws1 = _coefs(pic, 95, 2, st)
        res.append((_scan(co, 240, 240, 2, st), co, ws1))
    torch.cuda.synchronize()
    (a, na, _), (b, nb, _) = res[0][0], res[1][0]
    assert int(na.item()) == int(nb.item()) > 0 and torch.equal(a, b)
    co, _, _ = er.coefficients(img, 95, 2)
    assert a.cpu().numpy()[: int(na.item())].tobytes() == er.scan(co, 240, 240, 2)


def test_refusals_name_the_argument_and_launch_nothing():
    """bad sizes, quality, subsampling and workspaces: return code 1 with the message, and the outputs keep their fill"""
    import torch

    from cerberus_amd import _lib

    L = _lib.lib()
    pic = torch.zeros((16, 16, 3), dtype=torch.uint8, device="cuda")
    planes, coefs, scan_ws, scan_cap = _sizes(16, 16, 2)
    ws = torch.empty((max(planes, scan_ws),), dtype=torch.uint8, device="cuda")
    co = torch.full((coefs // 2,), 0x1234, dtype=torch.int16, device="cuda")
    out = torch.full((scan_cap,), 0xAA, dtype=torch.uint8, device="cuda")
    n = torch.full((1,), -7, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def coefs_call(w=16, h=16, q=75, ss=2, nws=None):
        return L.cerb_jpeg_enc_coefs(pic.data_ptr(), 48, w, h, q, ss, co.data_ptr(), None, ws.data_ptr(), ws.numel() if nws is None else nws, st)

    def scan_call(w=16, h=16, ss=2, nws=None):
        return L.cerb_jpeg_enc_scan(co.data_ptr(), w, h, ss, ws.data_ptr(), ws.numel() if nws is None else nws, out.data_ptr(), scan_cap, n.data_ptr(), st)

    for call, word in ((lambda: coefs_call(w=0), "width and height"), (lambda: coefs_call(h=32769), "width and height"), (lambda: coefs_call(q=0), "quality"),
                       (lambda: coefs_call(q=101), "quality"), (lambda: coefs_call(ss=1), "subsampling"), (lambda: coefs_call(nws=planes - 1), "workspace is too small"),
                       (lambda: scan_call(w=32769), "width and height"), (lambda: scan_call(h=0), "width and height"), (lambda: scan_call(ss=3), "subsampling"),
                       (lambda: scan_call(nws=scan_ws - 1), "workspace is too small")):
        with pytest.raises(_lib.CerberusHipError, match=word):
            _lib.check(call())
    for bad in ((0, 16, 2), (16, 32769, 2), (16, 16, 1)):
        assert all(v == 0 for v in _sizes(*bad))
    torch.cuda.synchronize()
    assert bool((co == 0x1234).all()) and bool((out == 0xAA).all()) and int(n.item()) == -7


@pytest.mark.parametrize("ss", [0, 2])
def test_noise_at_quality_100_stays_below_the_reported_capacity(ss):
    """uniform noise, quality 100 (every table entry 1): the longest scan an 8-bit picture of the size gives stays below cerb_jpeg_enc_workspace_bytes(.., 3),
    and a caller that gives less room gets the full length back and nothing written past what it gave"""
    import torch

    img = np.random.RandomState(12).randint(0, 256, (40, 120, 3)).astype(np.uint8)
    co, _, _ = er.coefficients(img, 100, ss)
    want = er.scan(co, 40, 120, ss)
    _, _, got, n = _device_scan(img, 100, ss)
    assert got == want and n < _sizes(120, 40, ss)[3]
    dco, _, _ = _coefs(torch.from_numpy(img).cuda(), 100, ss)
    out, dn, _ = _scan(dco, 120, 40, ss, cap=1000)
    torch.cuda.synchronize()
    flat = out.cpu().numpy()
    assert int(dn.item()) == len(want) > 1000 and flat[:1000].tobytes() == want[:1000] and (flat[1000:] == 0xAA).all()
