"""numpy statement of the JPEG arithmetic the device kernels implement (include/cerberus_hip.h, "JPEG tiles"; csrc/jpeg_kernels.hip), and the seeded
streams the JPEG tests share.  Fed by the C entropy decoder's header + quantised coefficients, it must equal PIL byte for byte."""
import io

import numpy as np

A, B, C_, D, E, F, G, H_, I, J, K, L = 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172


def idct_1d(i):
    """one pass over the LAST axis (int64), unshifted"""
    i0, i1, i2, i3, i4, i5, i6, i7 = [i[..., k] for k in range(8)]
    z1 = (i2 + i6) * C_
    t2, t3 = z1 - i6 * H_, z1 + i2 * D
    t0, t1 = (i0 + i4) * 8192, (i0 - i4) * 8192
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    u0, u1, u2, u3 = i7, i5, i3, i1
    z1, z2, z3, z4 = u0 + u3, u1 + u2, u0 + u2, u1 + u3
    z5 = (z3 + z4) * F
    u0, u1, u2, u3 = u0 * A, u1 * J, u2 * L, u3 * G
    z1, z2 = z1 * -E, z2 * -K
    z3, z4 = z3 * -I + z5, z4 * -B + z5
    u0, u1, u2, u3 = u0 + z1 + z3, u1 + z2 + z4, u2 + z2 + z3, u3 + z1 + z4
    return np.stack([t10 + u3, t11 + u2, t12 + u1, t13 + u0, t13 - u0, t12 - u1, t11 - u2, t10 - u3], axis=-1)


def plane(coefs, q, brows, bcols):
    """int16 [brows * bcols * 64] quantised coefficients + uint16 [64] table -> uint8 [brows * 8, bcols * 8]"""
    x = coefs.reshape(brows, bcols, 8, 8).astype(np.int64) * q.reshape(8, 8).astype(np.int64)
    x = (np.swapaxes(idct_1d(np.swapaxes(x, -1, -2)), -1, -2) + 1024) >> 11  # pass 1 down the columns
    x = (idct_1d(x) + 131072) >> 18
    x = np.clip(x + 128, 0, 255).astype(np.uint8)
    return x.transpose(0, 2, 1, 3).reshape(brows * 8, bcols * 8)


def upsample_h2v1(p):
    p = p.astype(np.int32)
    h, w = p.shape
    left = np.concatenate([p[:, :1], p[:, :-1]], axis=1)
    right = np.concatenate([p[:, 1:], p[:, -1:]], axis=1)
    out = np.empty((h, 2 * w), np.int32)
    out[:, 0::2] = (3 * p + left + 1) >> 2
    out[:, 1::2] = (3 * p + right + 2) >> 2
    out[:, 0], out[:, -1] = p[:, 0], p[:, -1]
    return out


def upsample_h2v2(p):
    p = p.astype(np.int32)
    h, w = p.shape
    out = np.empty((2 * h, 2 * w), np.int32)
    for v in (0, 1):
        rr = np.clip(np.arange(h) + (1 if v else -1), 0, h - 1)
        s = 3 * p + p[rr]
        left = np.concatenate([s[:, :1], s[:, :-1]], axis=1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], axis=1)
        out[v::2, 0::2] = (3 * s + left + 8) >> 4
        out[v::2, 1::2] = (3 * s + right + 7) >> 4
    return out


def decode(hdr, coefs):
    """hdr: jpeg_device.JpegHdr of a decoded stream; coefs: its int16 coefficients -> uint8 [height, width, 3]"""
    W, Hh = hdr.width, hdr.height
    hs, vs = list(hdr.h), list(hdr.v)
    planes, off = [], 0
    for k in range(3):
        br, bc = hdr.mcu_rows * vs[k], hdr.mcu_cols * hs[k]
        q = np.array(hdr.q[k][:], np.uint16)
        p = plane(coefs[off:off + br * bc * 64], q, br, bc)
        off += br * bc * 64
        planes.append(p[: -(-Hh * vs[k] // vs[0]), : -(-W * hs[k] // hs[0])])  # the component's true size BEFORE up-sampling
    y = planes[0].astype(np.int32)
    if hs[0] == 1:
        cb, cr = planes[1].astype(np.int32), planes[2].astype(np.int32)
    elif vs[0] == 1:
        cb, cr = upsample_h2v1(planes[1]), upsample_h2v1(planes[2])
    else:
        cb, cr = upsample_h2v2(planes[1]), upsample_h2v2(planes[2])
    cb, cr = cb[:Hh, :W], cr[:Hh, :W]
    if hdr.transform:
        cb, cr = cb - 128, cr - 128
        r = y + ((91881 * cr + 32768) >> 16)
        g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
        b = y + ((116130 * cb + 32768) >> 16)
    else:
        r, g, b = y, cb, cr
    return np.clip(np.stack([r, g, b], axis=-1), 0, 255).astype(np.uint8)


# ---- seeded inputs ----------------------------------------------------------------------------------------------------------------------------
def image(h, w, seed):
    """smooth gradients + noise + a flat rectangle: large coefficients and all-zero blocks both occur"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.stack([40 + 170 * xx / max(1, w - 1), 220 - 180 * yy / max(1, h - 1), 128 + 100 * np.sin(xx / 7.0 + seed) * np.cos(yy / 5.0)], axis=-1)
    img += rng.normal(0, 18, img.shape)
    img[h // 4: h // 4 + max(1, h // 3), w // 3: w // 3 + max(1, w // 2)] = (200, 30, 90)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, quality=95, subsampling=0, restart=0, progressive=False, mode="RGB"):
    from PIL import Image

    buf = io.BytesIO()
    im = Image.fromarray(img if mode != "L" else img[..., 0], mode if mode == "L" else "RGB")
    kw = dict(restart_marker_blocks=restart) if restart else {}
    im.save(buf, format="JPEG", quality=quality, subsampling=subsampling, progressive=progressive, **kw)
    return buf.getvalue()


def segments(data):
    """[(marker, start, end)] of the marker segments in front of the scan; the last entry is the SOS segment"""
    out, i = [], 2
    while True:
        assert data[i] == 0xFF
        m = data[i + 1]
        n = (data[i + 2] << 8) | data[i + 3]
        out.append((m, i, i + 2 + n))
        i += 2 + n
        if m == 0xDA:
            return out


def split_tables(data):
    """a full stream -> (JPEGTables stream: SOI + DQT / DHT + EOI, abbreviated stream: everything else)"""
    tabs, rest, last = b"\xff\xd8", b"\xff\xd8", 0
    for m, a, b in segments(data):
        if m in (0xDB, 0xC4):
            tabs += data[a:b]
        else:
            rest += data[a:b]
        last = b
    return tabs + b"\xff\xd9", rest + data[last:]


def strip_app(data, markers=(0xE0, 0xEE)):
    out, last = b"\xff\xd8", 0
    for m, a, b in segments(data):
        if m not in markers:
            out += data[a:b]
        last = b
    return out + data[last:]


def rename_components(data, ids):
    """the component ids of SOF0 and SOS replaced (same length)"""
    d = bytearray(data)
    for m, a, b in segments(data):
        if m in (0xC0, 0xC1):
            for k in range(3):
                d[a + 4 + 6 + 3 * k] = ids[k]
        if m == 0xDA:
            for k in range(3):
                d[a + 4 + 1 + 2 * k] = ids[k]
    return bytes(d)


def pil_pixels(data, tables=None, photometric=6):
    """what the slide reader gets from PIL for this tile today (reader.TiffReader._decode)"""
    from PIL import Image

    from cerberus_amd.reader import _strip_jfif_app0

    if tables:
        data = tables[:-2] + data[2:]
    if photometric == 2:
        data = _strip_jfif_app0(data)
        data = data[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x00" + data[2:]
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


SIZES = [(16, 16), (24, 40), (37, 53), (17, 9), (64, 64), (240, 240)]  # (height, width)


def cases():
    """[(name, stream, tables or None, photometric)]: sizes x subsampling x quality, restart intervals, tables + abbreviated stream, photometric 2 with
    and without a JFIF header, component ids R G B, an Adobe transform-1 stream without JFIF"""
    out = []
    for si, (h, w) in enumerate(SIZES):
        img = image(h, w, 10 + si)
        for ss in (0, 1, 2):
            for q in (30, 95):
                out.append(("%dx%d_ss%d_q%d" % (h, w, ss, q), encode(img, q, ss), None, 6))
            out.append(("%dx%d_ss%d_rst3" % (h, w, ss), encode(img, 95, ss, restart=3), None, 6))
    img = image(40, 56, 3)
    for ss in (0, 1, 2):
        full = encode(img, 90, ss)
        tabs, rest = split_tables(full)
        out.append(("tables_ss%d" % ss, rest, tabs, 6))
        out.append(("photometric2_jfif_ss%d" % ss, full, None, 2))
        out.append(("photometric2_plain_ss%d" % ss, strip_app(full), None, 2))
        out.append(("ids_RGB_ss%d" % ss, rename_components(strip_app(full), b"RGB"), None, 6))
        out.append(("ids_123_plain_ss%d" % ss, strip_app(full), None, 6))
        adobe1 = strip_app(full)
        out.append(("adobe1_ss%d" % ss, adobe1[:2] + b"\xff\xee\x00\x0eAdobe\x00\x64\x00\x00\x00\x00\x01" + adobe1[2:], None, 6))
    return out


def write_jpeg_tiff(path, levels, tile=64, ss=2, progressive_at=None, mpp=None):
    """a tiled (pyramidal) TIFF with JPEG tiles as scanners write them: the stored components are the image's own planes (PhotometricInterpretation
    RGB, ids 1 2 3, a JFIF header the reader drops).  progressive_at: the index of the ONE tile written as a progressive stream."""
    from PIL import Image

    from cerberus_amd.reader import write_tiled_tiff

    calls = [0]

    def pil_jpeg(t):
        buf = io.BytesIO()
        prog = progressive_at is not None and calls[0] == progressive_at
        calls[0] += 1
        Image.merge("YCbCr", [Image.fromarray(np.ascontiguousarray(t[..., i])) for i in range(3)]).save(buf, format="JPEG", quality=90, subsampling=ss, progressive=prog)
        return buf.getvalue()

    write_tiled_tiff(path, levels, tile=tile, mpp=mpp, encode=(pil_jpeg, 7))
    return path
