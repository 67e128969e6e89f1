"""JPEG tiles (TIFF compression 7) of a slide level decoded for the device: the host does the Huffman pass in native code (one call per window, no
interpreter lock: cerb_jpeg_read_tiles), the GPU does dequantisation, inverse DCT, chroma up-sampling, colour conversion and placement
(cerb_jpeg_decode_window) -- the bytes PIL returns, bit for bit (include/cerberus_hip.h, "JPEG tiles").

    decode_window(reader, level, x0, y0, x1, y1, dst, stream, buffers)   # -> tiles that must go through reader._decode (place_fallback)
    counters()                                                           # {"native": tiles decoded here, "fallback": tiles handed back}

Opt-in: wsi.SlabUploader takes this path when CERB_JPEG_DECODE=device (run_infer_wsi.py --jpeg_decode=device) and uploader_source() finds a tiled
compression-7 level whose first tile is a stream this decoder takes.  Tiles it does not take (progressive, other sampling layouts, ...) fall back to PIL
one by one; a corrupt tile raises ValueError naming the file and the tile."""
import ctypes as C
import os
import threading

import numpy as np

from . import _lib

OK, UNSUPPORTED, CORRUPT, TOO_LARGE = 0, 1, -1, -2


class JpegHdr(C.Structure):
    """cerb_jpeg_hdr of csrc/jpeg_entropy.h"""
    _fields_ = [("status", C.c_int32), ("width", C.c_int32), ("height", C.c_int32), ("h", C.c_int32 * 3), ("v", C.c_int32 * 3), ("transform", C.c_int32),
                ("mcu_cols", C.c_int32), ("mcu_rows", C.c_int32), ("gx0", C.c_int32), ("gy0", C.c_int32), ("reserved", C.c_int32 * 4),
                ("coef_off", C.c_int64), ("q", (C.c_uint16 * 64) * 3)]


assert C.sizeof(JpegHdr) == 464

_COUNT = {"native": 0, "fallback": 0}
_COUNT_LOCK = threading.Lock()


def counters():
    with _COUNT_LOCK:
        return dict(_COUNT)


def reset_counters():
    with _COUNT_LOCK:
        _COUNT["native"] = _COUNT["fallback"] = 0


def _ptr(b):
    return C.cast(C.c_char_p(b), C.c_void_p) if b else None


def decode_stream(data, tables=None, photometric=6, coef_cap=None):
    """One stream through the host entropy decoder -> (status, JpegHdr, int16 coefficients).  No device involved."""
    data = bytes(data)
    if coef_cap is None:
        coef_cap = 3 * 16 * 16
        if len(data) >= 2:  # the frame header's size, 16-aligned, three full planes: what any accepted layout needs at most
            i = data.find(b"\xff\xc0")
            i = data.find(b"\xff\xc1") if i < 0 else i
            if 0 <= i and i + 9 <= len(data):
                hh, ww = (data[i + 5] << 8) | data[i + 6], (data[i + 7] << 8) | data[i + 8]
                coef_cap = 3 * (-(-ww // 16) * 16) * (-(-hh // 16) * 16)
    hdr = JpegHdr()
    coefs = np.zeros(max(1, int(coef_cap)), np.int16)
    used = C.c_longlong(0)
    rc = _lib.lib().cerb_jpeg_decode_stream(_ptr(tables), len(tables) if tables else 0, _ptr(data), len(data), 1 if photometric == 2 else 0,
                                            C.byref(hdr), coefs.ctypes.data, int(coef_cap), C.byref(used))
    return rc, hdr, coefs[: used.value]


def workspace_bytes(n_tiles, tw, th):
    """(stream buffer bytes -- pinned and device --, device scratch bytes) for n_tiles tiles of tw x th"""
    L = _lib.lib()
    return int(L.cerb_jpeg_workspace_bytes(n_tiles, tw, th, 0)), int(L.cerb_jpeg_workspace_bytes(n_tiles, tw, th, 1))


class Buffers(object):
    """One ring slot: the pinned stream buffer, its device copy and the device scratch, for up to n_tiles tiles of tw x th.  `scratch` may be shared
    between the slots of a ring whose work runs on ONE stream."""

    def __init__(self, n_tiles, tw, th, device, pinned=None, scratch=None):
        import torch

        self.n_tiles, self.tw, self.th = int(n_tiles), int(tw), int(th)
        self.stream_bytes, self.scratch_bytes = workspace_bytes(n_tiles, tw, th)
        self.pinned = pinned if pinned is not None else torch.empty((self.stream_bytes,), dtype=torch.uint8).pin_memory()
        assert self.pinned.numel() >= self.stream_bytes
        self.dev = torch.empty((self.stream_bytes,), dtype=torch.uint8, device=device)
        self.scratch = scratch if scratch is not None else torch.empty((self.scratch_bytes,), dtype=torch.uint8, device=device)
        assert self.scratch.numel() >= self.scratch_bytes

    def device_bytes(self):
        return self.stream_bytes + self.scratch_bytes


def window_tiles(p, x0, y0, x1, y1):
    return [(ty, tx) for ty in range(y0 // p.th, -(-y1 // p.th)) for tx in range(x0 // p.tw, -(-x1 // p.tw))]


def max_window_tiles(p, rows):
    """tiles a window of `rows` rows and the level's full width can touch, wherever it starts"""
    return (-(-p.w // p.tw)) * (min(-(-p.h // p.th), (max(1, int(rows)) + p.th - 2) // p.th + 1))


def read_tiles_host(reader, level, tiles, buf_ptr, buf_bytes):
    """The host half for tiles [(ty, tx)] of a level -> (bytes of the buffer in use, positions in `tiles` of the unsupported ones)."""
    p = reader.levels[level]
    across = -(-p.w // p.tw)
    n = len(tiles)
    idx = np.array([ty * across + tx for ty, tx in tiles], np.int64)
    offs = np.ascontiguousarray(np.asarray(p.offsets, np.int64)[idx])
    cnts = np.ascontiguousarray(np.asarray(p.counts, np.int64)[idx])
    gx0 = np.array([tx * p.tw for _, tx in tiles], np.int32)
    gy0 = np.array([ty * p.th for ty, _ in tiles], np.int32)
    tabs = bytes(p.jpeg_tables) if p.jpeg_tables else b""
    used, bad, n_uns = C.c_size_t(0), C.c_int32(-1), C.c_int32(0)
    uns = np.zeros(max(1, n), np.int32)
    from .reader import decode_threads

    rc = _lib.lib().cerb_jpeg_read_tiles(reader.fh.fileno(), n, offs.ctypes.data, cnts.ctypes.data, gx0.ctypes.data, gy0.ctypes.data, p.tw, p.th, _ptr(tabs),
                                         len(tabs), 1 if p.photometric == 2 else 0, buf_ptr, buf_bytes, decode_threads(), C.byref(used), C.byref(bad),
                                         C.byref(n_uns), uns.ctypes.data)
    if rc != 0:
        msg = _lib.lib().cerb_last_error().decode("utf-8", "replace")
        if bad.value >= 0:
            raise ValueError("%s: strip / tile %d of level %d: JPEG stream truncated or corrupt (%s)" % (reader.path, int(idx[bad.value]), level, msg))
        raise _lib.CerberusHipError(msg)
    return int(used.value), [int(v) for v in uns[: n_uns.value]]


def decode_window(reader, level, x0, y0, x1, y1, dst, stream=None, buffers=None):
    """Pixels [x0, x1) x [y0, y1) of a TiffReader level with JPEG tiles into dst (uint8 device tensor [y1 - y0, x1 - x0, 3], rows of any stride): the
    host half into pinned memory, ONE non_blocking copy of headers + coefficients, the device half, all on `stream` (default: the current one).
    Returns the tiles [(ty, tx)] this decoder does not take: the caller decodes exactly those the old way (place_fallback)."""
    import torch

    p = reader.levels[level]
    x0, y0, x1, y1 = max(0, int(x0)), max(0, int(y0)), min(p.w, int(x1)), min(p.h, int(y1))
    assert dst.dtype == torch.uint8 and dst.dim() == 3 and dst.shape[2] == 3 and dst.stride(2) == 1 and dst.stride(1) == 3
    assert dst.shape[0] >= y1 - y0 and dst.shape[1] >= x1 - x0
    tiles = window_tiles(p, x0, y0, x1, y1)
    if not tiles or x1 <= x0 or y1 <= y0:
        return []
    own = buffers is None
    if own:
        buffers = Buffers(len(tiles), p.tw, p.th, dst.device)
    assert len(tiles) <= buffers.n_tiles and (p.tw, p.th) == (buffers.tw, buffers.th), (len(tiles), buffers.n_tiles)
    used, uns = read_tiles_host(reader, level, tiles, buffers.pinned.data_ptr(), buffers.stream_bytes)
    stream = stream or torch.cuda.current_stream(dst.device)
    with torch.cuda.device(dst.device), torch.cuda.stream(stream):
        buffers.dev[:used].copy_(buffers.pinned[:used], non_blocking=True)
        _lib.check(_lib.lib().cerb_jpeg_decode_window(buffers.dev.data_ptr(), used, len(tiles), p.tw, p.th, buffers.scratch.data_ptr(), buffers.scratch.numel(),
                                                      dst.data_ptr(), dst.stride(0), x0, y0, x1, y1, C.c_void_p(stream.cuda_stream)))
    if own:  # buffers made for this call alone must outlive the work queued on them
        stream.synchronize()
    with _COUNT_LOCK:
        _COUNT["native"] += len(tiles) - len(uns)
        _COUNT["fallback"] += len(uns)
    return [tiles[i] for i in uns]


def place_fallback(reader, level, window, tiles, dst, stream=None):
    """The tiles decode_window handed back: each through reader._decode (PIL) and into its place in dst, on the same stream."""
    import torch

    p = reader.levels[level]
    x0, y0, x1, y1 = max(0, int(window[0])), max(0, int(window[1])), min(p.w, int(window[2])), min(p.h, int(window[3]))
    stream = stream or torch.cuda.current_stream(dst.device)
    for ty, tx in tiles:
        a0, a1 = max(y0, ty * p.th), min(y1, (ty + 1) * p.th)
        b0, b1 = max(x0, tx * p.tw), min(x1, (tx + 1) * p.tw)
        if a1 <= a0 or b1 <= b0:
            continue
        part = np.zeros((a1 - a0, b1 - b0, 3), np.uint8)
        reader._place_tile(p, (ty, tx), (b0, a0, b1, a1), part)
        with torch.cuda.stream(stream):
            dst[a0 - y0:a1 - y0, b0 - x0:b1 - x0].copy_(torch.from_numpy(part))


def level_supported(reader, level):
    """a tiled compression-7 level whose first tile is a stream of the tile's size that the entropy decoder takes"""
    p = reader.levels[level]
    if p.compression != 7 or not getattr(p, "tiled", False) or p.samples != 3 or not p.counts:
        return False
    data = os.pread(reader.fh.fileno(), p.counts[0], p.offsets[0])
    rc, hdr, _ = decode_stream(data, bytes(p.jpeg_tables) if p.jpeg_tables else None, p.photometric, coef_cap=workspace_bytes(1, p.tw, p.th)[1])
    return rc == OK and (hdr.width, hdr.height) == (p.tw, p.th)


def uploader_source(host, plan):
    """(reader, level) when wsi.SlabUploader's source is a TiffReader level this module decodes -- `plan`: the uploader's device-resample plan or
    None (then the rows must BE level 0) --, else None."""
    from .reader import TiffReader, _Rows

    if not isinstance(host, _Rows) or not isinstance(host.reader, TiffReader):
        return None
    r = host.reader
    if plan is not None:
        level = plan.lvl
    elif abs(r._scale(host.resolution, host.units) - 1.0) < 1e-9:
        level = 0
    else:
        return None
    return (r, level) if level_supported(r, level) else None


def ring_bytes_estimate(width, chunk_bytes=24 << 20, buffers=3, tile=256, resampled=False):
    """Device bytes of an uploader's coefficient ring (what stream_bands prices when the switch is on): per slot 2 bytes per sample of the largest
    chunk plus its tile row of slack, and one scratch of 1 byte per sample."""
    row = (-(-int(width) // tile) * tile) * 3
    rows = max(tile, (4 if resampled else 1) * int(chunk_bytes) // max(1, row)) + 2 * tile
    return (2 * int(buffers) + 1) * rows * row


def pack_stream_buffer(items):
    """[(JpegHdr, int16 coefficients, gx0, gy0)] of decode_stream -> the stream buffer cerb_jpeg_decode_window reads (uint8 array: headers, padded to
    256 bytes, then the coefficients back to back) -- per-stream decodes laid out as one window call lays them out."""
    n = len(items)
    base = -(-n * C.sizeof(JpegHdr) // 256) * 256
    total = sum(int(co.size) for _, co, _, _ in items)
    buf = np.zeros(base + 2 * total, np.uint8)
    off = 0
    for i, (hdr, co, gx0, gy0) in enumerate(items):
        h = JpegHdr.from_buffer_copy(bytes(hdr))
        h.gx0, h.gy0, h.coef_off = int(gx0), int(gy0), off
        buf[i * C.sizeof(JpegHdr):(i + 1) * C.sizeof(JpegHdr)] = np.frombuffer(bytes(h), np.uint8)
        buf[base + 2 * off: base + 2 * (off + co.size)] = np.ascontiguousarray(co, np.int16).view(np.uint8)
        off += int(co.size)
    return buf
