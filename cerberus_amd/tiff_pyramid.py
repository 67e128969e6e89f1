"""Pictures that live on the device written as the tiles of a pyramidal JPEG-in-TIFF file -- what QuPath, ASAP and OpenSlide open at full
resolution.  Not in the reference.  Two halves:

    enc = TileEncoder(device, max_w, max_h, tile)       # sibling of jpeg_encode.Encoder: owns workspace, tile bytes and a pinned buffer
    handle = enc.encode(picture_u8_cuda, quality=75, subsampling=2, stream=None)     # sides: multiples of `tile`
    data, offsets, counts = handle.tiles()              # ONE host wait; tile i (row-major) is data[offsets[i] : offsets[i] + counts[i]]

    w = PyramidWriter(path, width, height, tile, quality, subsampling, mpp=None)     # host only: imports no torch, takes tile bytes from ANY source
    w.add_tiles(level, tile_indices, data, offsets, counts)                          # in arrival order
    w.close()                                           # one IFD per level, the chain patched, the temporary file renamed to `path`

A tile is an ABBREVIATED stream, SOI SOF0 DRI SOS scan EOI (cerb_jpeg_enc_tiles, include/cerberus_hip.h "JPEG encoding"): the quantisation and Huffman
tables stand once per page in JPEGTables.  Every MCU row of a tile is a restart interval.  The file is always BigTIFF."""
import os
import struct

from .jpeg_encode import AC_CHROMA, AC_LUMA, DC_CHROMA, DC_LUMA, ZIGZAG, _segment, quant_tables


def check_tile(tile):
    if int(tile) != tile or not 16 <= tile <= 512 or tile % 16:
        raise ValueError("tiff_pyramid: tile must be a multiple of 16 in 16 .. 512, got %r" % (tile,))
    return int(tile)


def tile_prefix(tile, subsampling):
    """what stands in front of every tile's scan: SOI, SOF0 (tile x tile), DRI (one MCU row), SOS -- 41 bytes"""
    s = 2 if subsampling == 2 else 1
    mcu_cols = tile // (8 * s)
    return (b"\xff\xd8" + _segment(0xC0, bytes((8, tile >> 8, tile & 255, tile >> 8, tile & 255, 3, 1, (s << 4) | s, 0, 2, 0x11, 1, 3, 0x11, 1)))
            + _segment(0xDD, bytes((mcu_cols >> 8, mcu_cols & 255))) + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0))))


def jpeg_tables(quality):
    """the JPEGTables blob of a page: SOI, the two DQT of jpeg_encode.quant_tables, the four Annex-K DHT, EOI"""
    out = b"\xff\xd8"
    for i, q in enumerate(quant_tables(quality)):
        out += _segment(0xDB, bytes((i,)) + bytes(q[ZIGZAG[k]] for k in range(64)))
    for tc_th, (bits, vals) in ((0x00, DC_LUMA), (0x10, AC_LUMA), (0x01, DC_CHROMA), (0x11, AC_CHROMA)):
        out += _segment(0xC4, bytes((tc_th,)) + bytes(bits) + bytes(vals))
    return out + b"\xff\xd9"


def level_sizes(width, height, tile):
    """[(w, h)] of level 0, 1, ..: each the ceiling of half the one before, down to the first whose sides are both <= tile"""
    out = [(int(width), int(height))]
    while max(out[-1]) > tile:
        out.append((-(-out[-1][0] // 2), -(-out[-1][1] // 2)))
    return out


class PyramidWriter(object):
    """Tile bytes arrive in any order and go to the file at once; close() writes the directories.  Always BigTIFF (version 43, 8-byte offsets,
    TileOffsets / TileByteCounts as LONG8): a 98304-pixel-square slide passes 4 GB.  The file grows under `path` + ".part" and takes its name on
    close(); abort() removes it."""

    def __init__(self, path, width, height, tile, quality, subsampling, mpp=None):
        self.tile = check_tile(tile)
        if subsampling not in (0, 2):
            raise ValueError("tiff_pyramid: subsampling must be 0 (4:4:4) or 2 (4:2:0), got %r" % (subsampling,))
        if int(width) < 1 or int(height) < 1:
            raise ValueError("tiff_pyramid: the picture's sides must be >= 1, got %r x %r" % (width, height))
        self.tables = jpeg_tables(quality)  # (refuses a bad quality)
        self.path, self.subsampling, self.mpp = str(path), int(subsampling), None if mpp is None else float(mpp)
        self.sizes = level_sizes(width, height, self.tile)
        self.grids = [(-(-w // self.tile), -(-h // self.tile)) for w, h in self.sizes]  # tiles across, down
        self.where = [[None] * (a * d) for a, d in self.grids]  # per level and tile: (offset in the file, byte count)
        self._tmp = self.path + ".part"
        self._fh = open(self._tmp, "wb")
        self._fh.write(b"II" + struct.pack("<HHHQ", 43, 8, 0, 0))  # the first directory's offset is patched by close()
        self._pos = 16

    def add_tiles(self, level, tile_indices, data, offsets, counts):
        """tile tile_indices[i] of `level` (row-major over the level's tile grid) is data[offsets[i] : offsets[i] + counts[i]].  With one more offset
        than tiles (the total) and even offsets in ascending order -- what TileEncoder and cerb_jpeg_enc_tiles give -- the block goes out in one write."""
        where, n = self.where[level], len(tile_indices)
        mv = memoryview(data).cast("B") if not isinstance(data, (bytes, bytearray, memoryview)) else memoryview(data)
        offsets, counts = [int(v) for v in offsets], [int(v) for v in counts]
        if len(counts) != n or len(offsets) not in (n, n + 1):
            raise ValueError("tiff_pyramid: %d tiles with %d offsets and %d counts" % (n, len(offsets), len(counts)))
        for t in tile_indices:
            if not 0 <= int(t) < len(where):
                raise ValueError("tiff_pyramid: level %d has %d tiles, got tile index %d" % (level, len(where), int(t)))
        whole = len(offsets) == n + 1 and all(offsets[i] + counts[i] <= offsets[i + 1] for i in range(n)) and not any(o & 1 for o in offsets)
        if whole:
            self._fh.write(mv[offsets[0]:offsets[n]])
            for i, t in enumerate(tile_indices):
                where[int(t)] = (self._pos + offsets[i] - offsets[0], counts[i])
            self._pos += offsets[n] - offsets[0]
            return
        for i, t in enumerate(tile_indices):
            self._fh.write(mv[offsets[i]:offsets[i] + counts[i]])
            where[int(t)] = (self._pos, counts[i])
            self._pos += counts[i]
            if self._pos & 1:  # (TIFF: values start on a word boundary)
                self._fh.write(b"\0")
                self._pos += 1

    def abort(self):
        if self._fh is not None:
            self._fh.close()
            self._fh = None
            if os.path.exists(self._tmp):
                os.remove(self._tmp)

    def _put(self, data):
        at = self._pos
        self._fh.write(data)
        if len(data) & 1:
            self._fh.write(b"\0")
        self._pos += len(data) + (len(data) & 1)
        return at

    def close(self):
        for level, where in enumerate(self.where):
            missing = [i for i, v in enumerate(where) if v is None]
            if missing:
                self.abort()
                raise ValueError("tiff_pyramid: level %d lacks %d of its %d tiles (the first: %d)" % (level, len(missing), len(where), missing[0]))
        sizes = {1: 1, 3: 2, 4: 4, 5: 8, 7: 1, 16: 8}
        link = 8  # where the offset of the next directory goes: first the header's word
        for level, ((w, h), where) in enumerate(zip(self.sizes, self.where)):
            entries = []  # (tag, type, count, packed value)

            def put(tag, typ, vals):
                if typ == 7:
                    raw, cnt = bytes(vals), len(vals)
                elif typ == 5:
                    raw, cnt = b"".join(struct.pack("<II", a, b) for a, b in vals), len(vals)
                else:
                    raw, cnt = struct.pack("<%d%s" % (len(vals), {1: "B", 3: "H", 4: "I", 16: "Q"}[typ]), *vals), len(vals)
                assert len(raw) == cnt * sizes[typ]
                entries.append((tag, typ, cnt, raw if len(raw) <= 8 else struct.pack("<Q", self._put(raw))))

            ss = 2 if self.subsampling == 2 else 1
            put(254, 4, [1 if level else 0])
            put(256, 4, [w])
            put(257, 4, [h])
            put(258, 3, [8, 8, 8])
            put(259, 3, [7])
            put(262, 3, [6])
            put(277, 3, [3])
            if self.mpp is not None:  # pixels per centimetre of THIS level
                per_cm = (int(round(1e4 / (self.mpp * 2 ** level) * 1000)), 1000)
                put(282, 5, [per_cm])
                put(283, 5, [per_cm])
            put(284, 3, [1])
            if self.mpp is not None:
                put(296, 3, [3])
            put(322, 4, [self.tile])
            put(323, 4, [self.tile])
            put(324, 16, [v[0] for v in where])
            put(325, 16, [v[1] for v in where])
            put(347, 7, self.tables)
            put(530, 3, [ss, ss])
            ifd = self._put(struct.pack("<Q", len(entries)) + b"".join(struct.pack("<HHQ", t, ty, c) + v.ljust(8, b"\0") for t, ty, c, v in entries)
                            + struct.pack("<Q", 0))
            self._fh.seek(link)
            self._fh.write(struct.pack("<Q", ifd))
            self._fh.seek(self._pos)
            link = ifd + 8 + 20 * len(entries)
        self._fh.close()
        self._fh = None
        os.replace(self._tmp, self.path)


# ---- the device half -------------------------------------------------------------------------------------------------------------------------------
def tiles_workspace_bytes(w, h, tile, subsampling=2):
    """(workspace, the out_cap that never truncates) of cerb_jpeg_enc_tiles_workspace_bytes; (0, 0) for arguments the call refuses"""
    from . import _lib

    L = _lib.lib()
    return tuple(int(L.cerb_jpeg_enc_tiles_workspace_bytes(int(w), int(h), int(tile), int(subsampling), k)) for k in range(2))


class TileHandle(object):
    """One queued encode.  tiles() waits for it ONCE and returns (bytes, offsets [n + 1], counts [n]): numpy views of the encoder's pinned buffers,
    good until its next encode()."""

    def __init__(self, encoder, event, n_tiles, first):
        self._enc, self._event, self._n, self._first, self._out = encoder, event, n_tiles, first, None

    def tiles(self):
        if self._out is None:
            from . import _lib

            enc, n = self._enc, self._n
            self._event.synchronize()
            meta = enc._meta_host.numpy()
            offsets, counts = meta[:n + 1], meta[n + 1:2 * n + 1]
            total = int(offsets[n])
            if total > enc.out_cap:  # (cannot happen: out_cap is the bound of cerb_jpeg_enc_tiles_workspace_bytes(.., 1))
                raise _lib.CerberusHipError("tiff_pyramid: the tiles need %d bytes, the buffer holds %d" % (total, enc.out_cap))
            if total <= self._first:
                data = enc._pinned.numpy()[:total]
            else:  # a picture that compresses worse than the first copy allowed for: fetch everything (a second wait)
                data = enc._out[:total].cpu().numpy()
            self._out = (data, offsets, counts)
            self._enc = None
        return self._out


class TileEncoder(object):
    """Component planes, coefficients, the tiles' workspace and bytes on `device` for pictures up to max_w x max_h (multiples of `tile`) at either
    sampling, and the pinned buffers the tile bytes and their offsets / counts arrive in.  One encode is in flight at a time."""

    def __init__(self, device, max_w, max_h, tile):
        import torch

        self.device, self.tile = torch.device(device), check_tile(tile)
        self.max_w, self.max_h = int(max_w), int(max_h)
        planes, coefs, ws, self.out_cap = self._sizes(self.max_w, self.max_h, self.tile)
        n = (self.max_w // self.tile) * (self.max_h // self.tile)
        self._planes = torch.empty((planes,), dtype=torch.uint8, device=self.device)
        self._coefs = torch.empty((coefs // 2,), dtype=torch.int16, device=self.device)
        self._ws = torch.empty((ws,), dtype=torch.uint8, device=self.device)
        self._out = torch.empty((self.out_cap,), dtype=torch.uint8, device=self.device)
        self._meta = torch.zeros((2 * n + 1,), dtype=torch.int64, device=self.device)  # offsets [n + 1], counts [n] of the picture in flight
        self._meta_host = torch.zeros((2 * n + 1,), dtype=torch.int64).pin_memory()
        # the first copy brings 2 bits per sample and every tile's prefix: several times what quality 75 needs; more is fetched only when needed
        self._pinned = torch.empty((min(self.out_cap, max(1 << 16, self.max_w * self.max_h * 3 // 4 + 64 * n)),), dtype=torch.uint8).pin_memory()

    def device_bytes(self):
        return sum(t.numel() * t.element_size() for t in (self._planes, self._coefs, self._ws, self._out, self._meta))

    @staticmethod
    def _sizes(max_w, max_h, tile):
        """(planes, coefficients, tiles workspace, tile bytes) for either sampling"""
        from .jpeg_encode import workspace_bytes

        sizes = [workspace_bytes(max_w, max_h, ss)[:2] + tiles_workspace_bytes(max_w, max_h, tile, ss) for ss in (0, 2)]
        if not all(sizes[0]):
            raise ValueError("tiff_pyramid: the picture's sides must be multiples of tile %d in %d .. 32768, got %d x %d" % (tile, tile, max_w, max_h))
        return [max(a, b) for a, b in zip(*sizes)]

    @staticmethod
    def price(max_w, max_h, tile):
        """device bytes an encoder for max_w x max_h would hold, computed without touching a device"""
        return sum(TileEncoder._sizes(max_w, max_h, tile)) + 8 * (2 * (max_w // tile) * (max_h // tile) + 1)

    def encode(self, picture, quality=75, subsampling=2, stream=None):
        import ctypes as C

        import torch

        from . import _lib
        from .jpeg_encode import _check_picture

        _check_picture(picture)
        h, w, t = int(picture.shape[0]), int(picture.shape[1]), self.tile
        if w > self.max_w or h > self.max_h or w % t or h % t:
            raise ValueError("tiff_pyramid: a %d x %d picture in an encoder made for multiples of %d up to %d x %d" % (w, h, t, self.max_w, self.max_h))
        prefix = tile_prefix(t, subsampling)
        stream = stream or torch.cuda.current_stream(self.device)
        n = (w // t) * (h // t)
        L = _lib.lib()
        with torch.cuda.device(self.device), torch.cuda.stream(stream):
            st = C.c_void_p(stream.cuda_stream)
            _lib.check(L.cerb_jpeg_enc_coefs(picture.data_ptr(), picture.stride(0) if h > 1 else 3 * w, w, h, int(quality), int(subsampling),
                                             self._coefs.data_ptr(), None, self._planes.data_ptr(), self._planes.numel(), st))
            _lib.check(L.cerb_jpeg_enc_tiles(self._coefs.data_ptr(), w, h, t, int(subsampling), prefix, len(prefix), self._ws.data_ptr(), self._ws.numel(),
                                             self._out.data_ptr(), self.out_cap, self._meta.data_ptr(), self._meta.data_ptr() + 8 * (n + 1), st))
            self._meta_host[:2 * n + 1].copy_(self._meta[:2 * n + 1], non_blocking=True)
            first = min(self._pinned.numel(), tiles_workspace_bytes(w, h, t, subsampling)[1])
            self._pinned[:first].copy_(self._out[:first], non_blocking=True)
            event = torch.cuda.Event()
            event.record(stream)
        picture.record_stream(stream)
        return TileHandle(self, event, n, first)
