"""numpy statement of the JPEG ENCODER the device kernels implement (include/cerberus_hip.h, "JPEG encoding"; csrc/jpeg_encode.hip): colour conversion,
edge replication, 4:2:0 down-sampling, libjpeg's integer forward DCT ("islow"), quantisation, baseline Huffman coding with the Annex-K tables and one
restart interval per MCU row, and the file around the scan.  Sequential on purpose: one block, one symbol, one bit string after the other.  It must
equal PIL / libjpeg-turbo coefficient for coefficient (tests/test_jpeg_encode_host.py) and the kernels must equal it byte for byte."""
import io

import numpy as np

ZIGZAG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36,
          29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]  # natural index of the k-th zig-zag entry

# ---- Annex K -----------------------------------------------------------------------------------------------------------------------------------
Q_LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
          18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
Q_CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
_TAIL = [16 * r + s for r in range(16) for s in range(1, 11)]  # (only to CHECK the typed lists below: every run / size pair occurs once)
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xA1, 0x08,
            0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28,
            0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59,
            0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89,
            0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
            0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2,
            0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42, 0x91,
              0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26,
              0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58,
              0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87,
              0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
              0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA,
              0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA])
for _bits, _vals in (AC_LUMA, AC_CHROMA):
    assert sum(_bits) == len(_vals) == 162 and sorted(_vals) == sorted(_TAIL + [0x00, 0xF0])


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a DHT table (Annex C: codes of one length count up, a longer length doubles the next code)"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def qtable(base, quality):
    """natural-order uint16 [64]: the Annex-K table scaled as libjpeg's jpeg_set_quality does (force_baseline)"""
    q = int(quality)
    assert 1 <= q <= 100
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.array([min(255, max(1, (b * scale + 50) // 100)) for b in base], np.uint16)


def qtables(quality):
    return qtable(Q_LUMA, quality), qtable(Q_CHROMA, quality)


# ---- pixels -> quantised coefficients ------------------------------------------------------------------------------------------------------------
def geometry(h, w, subsampling):
    assert subsampling in (0, 2)
    s = 2 if subsampling == 2 else 1
    mcu = 8 * s
    return s, -(-h // mcu), -(-w // mcu)  # sampling factor of Y (both ways), MCU rows, MCU columns


def planes(img, subsampling):
    """uint8 [h, w, 3] RGB -> the padded Y plane and the padded (4:4:4) or down-sampled (4:2:0) Cb / Cr planes, int64.  libjpeg's order of edge work:
    columns are replicated at FULL resolution out to the MCU grid, rows only to a multiple of the vertical sampling (one row for an odd height); the
    component is down-sampled, and ITS last row is replicated down to the MCU grid."""
    h, w = img.shape[:2]
    s, mr, mc = geometry(h, w, subsampling)
    r, g, b = [img[..., k].astype(np.int64) for k in range(3)]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    out = [np.pad(y, ((0, mr * 8 * s - h), (0, mc * 8 * s - w)), mode="edge")]
    for p in (cb, cr):
        p = np.pad(p, ((0, -h % s), (0, mc * 8 * s - w)), mode="edge")
        if s == 2:
            bias = np.where(np.arange(p.shape[1] // 2) % 2 == 0, 1, 2)[None, :]
            p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
        out.append(np.pad(p, ((0, mr * 8 - p.shape[0]), (0, 0)), mode="edge"))
    return out


def fdct_1d(d):
    """one pass of jfdctint over the LAST axis (int64) -> (even outputs 0 and 4 UNSHIFTED sums, the six others unrounded at 13 bits)"""
    d0, d1, d2, d3, d4, d5, d6, d7 = [d[..., k] for k in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o4 = t10 + t11, t10 - t11
    z1 = (t12 + t13) * 4433
    o2, o6 = z1 + t13 * 6270, z1 - t12 * 15137
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    return o0, o4, {1: t7 + z1 + z4, 2: o2, 3: t6 + z2 + z3, 5: t5 + z2 + z4, 6: o6, 7: t4 + z1 + z3}


def fdct(block):
    """int64 [..., 8, 8] samples less 128 -> 8 x the DCT, int64 [..., 8, 8]"""
    o0, o4, odd = fdct_1d(block)  # pass 1 along the rows
    x = np.empty(block.shape, np.int64)
    x[..., 0], x[..., 4] = o0 << 2, o4 << 2
    for k, v in odd.items():
        x[..., k] = (v + (1 << 10)) >> 11
    o0, o4, odd = fdct_1d(np.swapaxes(x, -1, -2))  # pass 2 down the columns
    y = np.empty(block.shape, np.int64)
    y[..., 0], y[..., 4] = (o0 + 2) >> 2, (o4 + 2) >> 2
    for k, v in odd.items():
        y[..., k] = (v + (1 << 14)) >> 15
    return np.swapaxes(y, -1, -2)


def quantise(c, q):
    d = 8 * q.reshape(8, 8).astype(np.int64)
    return np.sign(c) * ((np.abs(c) + (d >> 1)) // d)


def coefficients(img, quality=75, subsampling=2):
    """-> (int16 coefficients in the decoder's layout: per component a raster of blocks of 64 in natural order, luma table, chroma table)"""
    h, w = img.shape[:2]
    s, mr, mc = geometry(h, w, subsampling)
    ql, qc = qtables(quality)
    out = []
    for k, p in enumerate(planes(img, subsampling)):
        br, bc = p.shape[0] // 8, p.shape[1] // 8
        blocks = p.reshape(br, 8, bc, 8).transpose(0, 2, 1, 3) - 128
        out.append(quantise(fdct(blocks), ql if k == 0 else qc).astype(np.int16).reshape(br, bc, 64))
    # 4:2:0: the Y blocks of an MCU that lie wholly beyond the component's own block grid (ceil(h / 8) x ceil(w / 8)) are libjpeg's "dummy blocks": no
    # AC, and the DC of the block before them in the MCU's order (top-left, top-right, bottom-left, bottom-right) -- for a dummy bottom row, of the
    # MCU's top-right block for both
    y, hb, wb = out[0], -(-h // 8), -(-w // 8)
    for row in range(mr):
        for m in range(mc):
            for dy in range(s):
                for dx in range(s):
                    br, bc = row * s + dy, m * s + dx
                    if br >= hb:
                        y[br, bc] = 0
                        y[br, bc, 0] = y[br - 1, m * s + 1, 0]
                    elif bc >= wb:
                        y[br, bc] = 0
                        y[br, bc, 0] = y[br, bc - 1, 0]
    return np.concatenate([o.reshape(-1) for o in out]), ql, qc


# ---- quantised coefficients -> entropy-coded scan ------------------------------------------------------------------------------------------------
class _Bits(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, length):
        self.acc = (self.acc << length) | (value & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def pad(self):
        while self.n:
            self.put(1, 1)


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v - 1) & ((1 << size) - 1)


def _block(bits, blk, pred, dc, ac):
    d = int(blk[0]) - pred
    size, mag = _magnitude(d)
    bits.put(*dc[size])
    bits.put(mag, size)
    run = 0
    for k in range(1, 64):
        v = int(blk[ZIGZAG[k]])
        if v == 0:
            run += 1
            continue
        while run >= 16:
            bits.put(*ac[0xF0])
            run -= 16
        size, mag = _magnitude(v)
        bits.put(*ac[(run << 4) | size])
        bits.put(mag, size)
        run = 0
    if run:
        bits.put(*ac[0x00])
    return int(blk[0])


def scan(coefs, h, w, subsampling):
    """the entropy-coded segment: one restart interval per MCU row, RSTm between the intervals"""
    s, mr, mc = geometry(h, w, subsampling)
    n0 = mr * s * mc * s * 64
    comp = [coefs[:n0].reshape(mr * s, mc * s, 64), coefs[n0:n0 + mr * mc * 64].reshape(mr, mc, 64), coefs[n0 + mr * mc * 64:].reshape(mr, mc, 64)]
    dcl, acl, dcc, acc = huff_codes(*DC_LUMA), huff_codes(*AC_LUMA), huff_codes(*DC_CHROMA), huff_codes(*AC_CHROMA)
    out = bytearray()
    for row in range(mr):
        bits, pred = _Bits(), [0, 0, 0]
        for m in range(mc):
            for dy in range(s):
                for dx in range(s):
                    pred[0] = _block(bits, comp[0][row * s + dy, m * s + dx], pred[0], dcl, acl)
            pred[1] = _block(bits, comp[1][row, m], pred[1], dcc, acc)
            pred[2] = _block(bits, comp[2][row, m], pred[2], dcc, acc)
        bits.pad()
        out += bits.out
        if row != mr - 1:
            out += bytes([0xFF, 0xD0 + row % 8])
    return bytes(out)


# ---- the file ------------------------------------------------------------------------------------------------------------------------------------
def _segment(marker, payload):
    return bytes([0xFF, marker, (len(payload) + 2) >> 8, (len(payload) + 2) & 255]) + bytes(payload)


def headers(h, w, quality, subsampling):
    s, _, mc = geometry(h, w, subsampling)
    ql, qc = qtables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i, q in enumerate((ql, qc)):
        out += _segment(0xDB, bytes([i]) + bytes(int(q[ZIGZAG[k]]) for k in range(64)))
    out += _segment(0xC0, bytes([8, h >> 8, h & 255, w >> 8, w & 255, 3, 1, (s << 4) | s, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, bytes([mc >> 8, mc & 255]))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


def encode(img, quality=75, subsampling=2):
    h, w = img.shape[:2]
    co, _, _ = coefficients(img, quality, subsampling)
    return headers(h, w, quality, subsampling) + scan(co, h, w, subsampling) + b"\xff\xd9"


# ---- PIL's side and the shared cases -------------------------------------------------------------------------------------------------------------
def pil_encode(img, quality=75, subsampling=2, restart_rows=0):
    from PIL import Image

    buf = io.BytesIO()
    kw = dict(restart_marker_rows=restart_rows) if restart_rows else {}
    Image.fromarray(img, "RGB").save(buf, format="JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()


def pil_decode(data):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def scan_of(data):
    """the entropy-coded bytes of a complete file (between the SOS segment and EOI)"""
    import jpeg_ref

    assert data[-2:] == b"\xff\xd9"
    return data[jpeg_ref.segments(data)[-1][2]:-2]


SIZES = [(16, 16), (17, 9), (37, 53), (64, 200), (240, 240), (8, 520)]  # (height, width)
QUALITIES = (30, 75, 95, 100)


def structured():
    """[(name, picture, quality)]: the pictures that drive one coding path each"""
    rng = np.random.RandomState(77)
    out = [("black", np.zeros((24, 40, 3), np.uint8), 75)]
    out.append(("noise_q100", rng.randint(0, 256, (48, 80, 3)).astype(np.uint8), 100))
    yy, xx = np.mgrid[0:32, 0:64]
    out.append(("checker8_q100", np.repeat((((yy // 8 + xx // 8) % 2) * 255).astype(np.uint8)[..., None], 3, axis=2), 100))
    # one high-frequency term per block: cos over the rows only, at the highest vertical frequency -> natural index 56, zig-zag position 35.  The
    # amplitude 61 is one of the two (47, 61) whose ROUNDED samples leave no other term at quality 100 (found by trying 1 .. 127)
    v = (128 + np.round(61 * np.cos((2 * (yy % 8) + 1) * 7 * np.pi / 16))).astype(np.uint8)
    out.append(("one_high_term_q100", np.repeat(v[..., None], 3, axis=2), 100))
    # bright noise on a near-white ground: long runs of 1-bits in the scan
    out.append(("ff_bytes", np.clip(rng.normal(235, 40, (40, 56, 3)), 0, 255).astype(np.uint8), 95))
    return out


def cases():
    """[(name, picture, quality, subsampling)]: SIZES x QUALITIES x 4:4:4 / 4:2:0 from jpeg_ref.image, then structured() at both samplings"""
    import jpeg_ref

    out = []
    for si, (h, w) in enumerate(SIZES):
        img = jpeg_ref.image(h, w, 40 + si)
        for ss in (0, 2):
            for q in QUALITIES:
                out.append(("%dx%d_ss%d_q%d" % (h, w, ss, q), img, q, ss))
    for name, img, q in structured():
        for ss in (0, 2):
            out.append(("%s_ss%d" % (name, ss), img, q, ss))
    return out
