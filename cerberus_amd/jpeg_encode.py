"""Pictures that live on the device written as baseline JPEG files without the pixels ever crossing to the host: colour conversion, forward DCT,
quantisation, Huffman coding and packing run in HIP (cerb_jpeg_enc_coefs / cerb_jpeg_enc_scan, csrc/jpeg_encode.hip), the headers around the scan are
written here.  The coefficients equal PIL's Image.save(format="JPEG", quality=q, subsampling=s) one for one (include/cerberus_hip.h, "JPEG encoding");
the files differ from PIL's in two things only: every MCU row is a restart interval (DRI + RSTm markers), and the order / content of the header
segments.  Not in the reference.

    enc = Encoder(device, max_w, max_h)                 # owns the workspace and a pinned byte buffer; reused across pictures
    handle = enc.encode(picture_u8_cuda, quality=75, subsampling=2, stream=None)
    data = handle.bytes()                               # ONE host wait, for compressed bytes
    data = encode_device(picture_u8_cuda)               # one-shot

A picture is a uint8 device tensor [h, w, 3] whose last two strides are (3, 1); rows may be any distance apart (a view into a larger picture)."""
import ctypes as C

from . import _lib

ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
          29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
# Annex K: the quantisation tables in natural order and the four Huffman tables as (codes per length 1 .. 16, symbols) -- the DHT payloads
Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99)
Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32
_AC_COMMON = tuple(16 * r + s for r in range(16) for s in range(1, 11))
DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D),
           (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
            0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
            0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
            0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA))
AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
             (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
              0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
              0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA))
assert sorted(AC_LUMA[1]) == sorted(AC_CHROMA[1]) == sorted(_AC_COMMON + (0x00, 0xF0))


def quant_tables(quality):
    """the two Annex-K tables in natural order, scaled as libjpeg's jpeg_set_quality scales them"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality must lie in 1 .. 100, got %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(tuple(min(255, max(1, (b * scale + 50) // 100)) for b in base) for base in (Q_LUMA, Q_CHROMA))


def _segment(marker, payload):
    n = len(payload) + 2
    return bytes((0xFF, marker, n >> 8, n & 255)) + bytes(payload)


def headers(w, h, quality, subsampling):
    """everything in front of the scan: SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI (one MCU row), SOS"""
    s = 2 if subsampling == 2 else 1
    mcu_cols = -(-int(w) // (8 * s))
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes((i,)) + bytes(q[ZIGZAG[k]] for k in range(64)))
    out += _segment(0xC0, bytes((8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, (s << 4) | s, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes((tc_th,)) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, bytes((mcu_cols >> 8, mcu_cols & 255)))
    return out + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def workspace_bytes(w, h, subsampling=2):
    """(planes workspace, coefficient bytes, scan workspace, the most a scan can take) of cerb_jpeg_enc_workspace_bytes"""
    L = _lib.lib()
    return tuple(int(L.cerb_jpeg_enc_workspace_bytes(int(w), int(h), int(subsampling), k)) for k in range(4))


def _check_picture(picture):
    import torch

    if not (isinstance(picture, torch.Tensor) and picture.is_cuda and picture.dtype == torch.uint8 and picture.dim() == 3 and picture.shape[2] == 3
            and picture.stride(2) == 1 and picture.stride(1) == 3 and (picture.shape[0] == 1 or picture.stride(0) >= 3 * picture.shape[1])):
        raise ValueError("jpeg_encode: a picture is a uint8 device tensor [h, w, 3] with strides (row, 3, 1)")


class Handle(object):
    """One queued encode.  bytes() waits for it and returns the complete file."""

    def __init__(self, encoder, head, event, first):
        self._enc, self._head, self._event, self._first, self._data = encoder, head, event, first, None

    def bytes(self):
        if self._data is None:
            enc = self._enc
            self._event.synchronize()
            n = int(enc._len_host[0])
            if n > enc.scan_cap:  # (cannot happen: scan_cap is the bound of cerb_jpeg_enc_workspace_bytes(.., 3))
                raise _lib.CerberusHipError("jpeg_encode: the scan needs %d bytes, the buffer holds %d" % (n, enc.scan_cap))
            if n <= self._first:
                body = enc._pinned[:n].numpy().tobytes()
            else:  # a picture that compresses worse than the first copy allowed for: fetch the rest (a second, short wait)
                body = enc._scan[:n].cpu().numpy().tobytes()
            self._data = self._head + body + b"\xff\xd9"
            self._enc = None
        return self._data


class Encoder(object):
    """Workspace, coefficient and scan buffers on `device` for pictures up to max_w x max_h at either sampling, and the pinned buffer the compressed
    bytes arrive in.  One encode is in flight at a time: take handle.bytes() before the next encode()."""

    def __init__(self, device, max_w, max_h):
        import torch

        self.device = torch.device(device)
        self.max_w, self.max_h = int(max_w), int(max_h)
        sizes = [workspace_bytes(self.max_w, self.max_h, ss) for ss in (0, 2)]
        if not all(sizes[0]):
            raise ValueError("jpeg_encode: the picture's width and height must lie in 1 .. 32768, got %d x %d" % (self.max_w, self.max_h))
        planes, coefs, scan_ws, self.scan_cap = [max(a, b) for a, b in zip(*sizes)]
        self._planes = torch.empty((planes,), dtype=torch.uint8, device=self.device)
        self._coefs = torch.empty((coefs // 2,), dtype=torch.int16, device=self.device)
        self._qt = torch.empty((128,), dtype=torch.int16, device=self.device)
        self._scan_ws = torch.empty((scan_ws,), dtype=torch.uint8, device=self.device)
        self._scan = torch.empty((self.scan_cap,), dtype=torch.uint8, device=self.device)
        self._len = torch.zeros((1,), dtype=torch.int64, device=self.device)
        self._len_host = torch.zeros((1,), dtype=torch.int64).pin_memory()
        # the first copy brings 2 bits per sample of the largest picture: several times what quality 75 needs; more is fetched only when needed
        self._pinned = torch.empty((min(self.scan_cap, max(1 << 16, self.max_w * self.max_h * 3 // 4)),), dtype=torch.uint8).pin_memory()

    def device_bytes(self):
        return sum(t.numel() * t.element_size() for t in (self._planes, self._coefs, self._qt, self._scan_ws, self._scan, self._len))

    def coefficients(self, picture, quality=75, subsampling=2, stream=None):
        """kernels 1-2 alone -> (int16 coefficients, uint16 [2, 64] tables) as views of the encoder's buffers, queued on `stream`"""
        import torch

        _check_picture(picture)
        h, w = int(picture.shape[0]), int(picture.shape[1])
        if w > self.max_w or h > self.max_h:
            raise ValueError("jpeg_encode: a %d x %d picture in an encoder made for %d x %d" % (w, h, self.max_w, self.max_h))
        stream = stream or torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().cerb_jpeg_enc_coefs(picture.data_ptr(), picture.stride(0) if h > 1 else 3 * w, w, h, int(quality), int(subsampling),
                                                      self._coefs.data_ptr(), self._qt.data_ptr(), self._planes.data_ptr(), self._planes.numel(),
                                                      C.c_void_p(stream.cuda_stream)))
        n = workspace_bytes(w, h, subsampling)[1] // 2
        return self._coefs[:n], self._qt.view(2, 64)

    def encode(self, picture, quality=75, subsampling=2, stream=None):
        import torch

        stream = stream or torch.cuda.current_stream(self.device)
        h, w = int(picture.shape[0]), int(picture.shape[1])
        head = headers(w, h, quality, subsampling)  # (refuses a bad quality before anything is queued)
        self.coefficients(picture, quality, subsampling, stream)
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            _lib.check(_lib.lib().cerb_jpeg_enc_scan(self._coefs.data_ptr(), w, h, int(subsampling), self._scan_ws.data_ptr(), self._scan_ws.numel(),
                                                     self._scan.data_ptr(), self.scan_cap, self._len.data_ptr(), C.c_void_p(stream.cuda_stream)))
            self._len_host.copy_(self._len, non_blocking=True)
            first = min(self._pinned.numel(), workspace_bytes(w, h, subsampling)[3])
            self._pinned[:first].copy_(self._scan[:first], non_blocking=True)
            event = torch.cuda.Event()
            event.record(stream)
        picture.record_stream(stream)
        return Handle(self, head, event, first)


def encode_device(picture, quality=75, subsampling=2, stream=None):
    """one picture -> the bytes of its JPEG file (an Encoder made for this call alone)"""
    _check_picture(picture)
    return Encoder(picture.device, picture.shape[1], picture.shape[0]).encode(picture, quality, subsampling, stream).bytes()
