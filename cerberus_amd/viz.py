"""Overlay rendering of the tile CLI (reference misc/viz_utils.py:187-214 `visualize_instances_dict_orig`,
called at infer/tile.py:251-257).  The first half is pure host code: contours come from the GPU (cerb_inst_contour_*), drawing is PIL
(`cv2.drawContours` is not available in this image; line rasterisation may differ from OpenCV's by a pixel -- cosmetic).  The second half draws
the same pictures, and the slide overlay of misc/viz_utils.py:150-184, on the device (cerb_overlay_*)."""

import numpy as np

# colours / line widths of the reference's dataset.yml `viz_info` blocks (configuration data): RGB of the first three entries
DEFAULT_VIZ_INFO = {
    "gland": {"line_width": 12, "inst_colour": (255, 255, 0), "type_colour": {0: (0, 0, 0), 1: (255, 255, 0), 2: (177, 52, 235)}},
    "lumen": {"line_width": 12, "inst_colour": (255, 0, 255), "type_colour": {0: (0, 0, 0), 1: (131, 235, 52)}},
    "nuclei": {"line_width": 3, "inst_colour": (0, 255, 0),
               "type_colour": {0: (0, 0, 0), 1: (0, 0, 255), 2: (0, 255, 0), 3: (255, 0, 255), 4: (176, 244, 230), 5: (0, 191, 255), 6: (255, 165, 0)}},
}


def visualize_instances_dict_orig(input_image, inst_dict_, viz_info=None):
    """input_image: uint8 (H, W, 3) RGB; inst_dict_: {'Gland'|'Lumen'|'Nuclei': {id: {'contour': (K,2) int (x, y), 'type'?: int}}}.
    Draws in the reference's fixed order Gland, Lumen, Nuclei; colour = type colour when the instance has a type, else the
    tissue's instance colour.  Returns a new uint8 RGB array."""
    from PIL import Image, ImageDraw

    viz_info = DEFAULT_VIZ_INFO if viz_info is None else viz_info
    im = Image.fromarray(np.ascontiguousarray(np.asarray(input_image).astype(np.uint8)))
    draw = ImageDraw.Draw(im)
    for tissue in ("Gland", "Lumen", "Nuclei"):
        if tissue not in inst_dict_:
            continue
        vi = viz_info[tissue.lower()]
        width = int(vi["line_width"])
        for _, info in inst_dict_[tissue].items():
            contour = info.get("contour")
            if contour is None or len(contour) < 2:
                continue
            colour = vi["type_colour"].get(int(info["type"]), vi["inst_colour"]) if "type" in info else vi["inst_colour"]
            pts = [(int(x), int(y)) for x, y in np.asarray(contour).reshape(-1, 2)]
            draw.line(pts + [pts[0]], fill=tuple(int(c) for c in colour[:3]), width=width, joint="curve")
    return np.array(im)


def up2_nearest(img):
    """cv2.resize(img, (0, 0), fx=2, fy=2, interpolation=INTER_NEAREST) (infer/tile.py:254)."""
    a = np.asarray(img)
    return np.repeat(np.repeat(a, 2, axis=0), 2, axis=1)


# ---- the same pictures drawn on the device (cerb_overlay_*: include/cerberus_hip.h "instance overlays") -------------------------
# The stroke is the project's own integer definition (round caps and joints, exact), not PIL's and not OpenCV's: the two differ from it in a share of
# the painted pixels that is cosmetic and unpinned.  Nothing below draws on the host, and nothing falls back to the functions above.
DRAW_ORDER = ("Gland", "Lumen", "Nuclei")
OVERLAY_MAX_SIDE = 32768


def colour_word(rgb):
    """(R, G, B) -> the uint32 word R | G << 8 | B << 16 of cerb_overlay_resolve."""
    r, g, b = (int(c) & 255 for c in tuple(rgb)[:3])
    return r | (g << 8) | (b << 16)


def contour_colours(tissue, tab, has_type, viz_info=None):
    """uint32 colour word per row of a cerb_inst_table array: the type colour where the instance has a type (inst_info.majority_type; a type the
    tissue has no colour for falls back as in visualize_instances_dict_orig), else the tissue's instance colour."""
    from .inst_info import majority_type

    vi = (DEFAULT_VIZ_INFO if viz_info is None else viz_info)[tissue.lower()]
    n = int(np.asarray(tab).shape[0])
    if not has_type:
        return np.full(n, colour_word(vi["inst_colour"]), np.uint32)
    lut = np.array([colour_word(vi["type_colour"].get(t, vi["inst_colour"])) for t in range(8)], np.uint32)
    return lut[majority_type(tab)]


def _pack_dict(tissue, insts, vi, width=None):
    """One tissue of an instance dictionary {id: {'contour': (K, 2) (x, y), 'type'?}} as a group of draw_contours_device (host arrays)."""
    pts, cnts, cols = [], [], []
    for info in insts.values():
        contour = info.get("contour")
        if contour is None or len(contour) < 2:
            continue
        c = np.asarray(contour).reshape(-1, 2)
        pts.append(c.astype(np.int64))
        cnts.append(c.shape[0])
        cols.append(colour_word(vi["type_colour"].get(int(info["type"]), vi["inst_colour"]) if "type" in info else vi["inst_colour"]))
    counts = np.asarray(cnts, np.int32)
    return {"points": np.concatenate(pts) if pts else np.zeros((0, 2), np.int64), "offsets": np.cumsum(counts, dtype=np.int64) - counts, "counts": counts,
            "colours": np.asarray(cols, np.uint32), "width": int(vi["line_width"] if width is None else width), "mul": 1, "div": 1, "origin": (0, 0)}


def _group_to_device(g, dev, who="draw_contours_device"):
    """-> (points int32 [P, 2], offsets int64 [n], counts int32 [n], colours uint32-as-int32 [n]) on dev.  A run that leaves the point list draws nothing:
    host arrays are checked (ValueError), device arrays get their count cleared on the device -- no host wait."""
    import torch

    def put(a, dt, shape):
        if isinstance(a, torch.Tensor):
            t = a.to(device=dev, dtype=dt)
        else:
            a = np.asarray(a)
            if dt == torch.int32 and a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError("%s: a value does not fit int32" % who)
            t = torch.from_numpy(np.ascontiguousarray(a.astype({torch.int32: np.int32, torch.int64: np.int64}[dt]))).to(dev)
        return t.reshape(shape).contiguous()

    pts, offs, cnts = put(g["points"], torch.int32, (-1, 2)), put(g["offsets"], torch.int64, (-1,)), put(g["counts"], torch.int32, (-1,))
    col = g["colours"]
    if isinstance(col, torch.Tensor):
        col = col.to(device=dev).contiguous().view(torch.int32).reshape(-1)
    else:
        col = torch.from_numpy(np.ascontiguousarray(np.asarray(col, dtype=np.uint32)).view(np.int32)).to(dev).reshape(-1)
    n = int(cnts.shape[0])
    if int(offs.shape[0]) != n or int(col.shape[0]) != n:
        raise ValueError("%s: offsets, counts and colours must have one entry per contour" % who)
    if not any(isinstance(g[k], torch.Tensor) for k in ("points", "offsets", "counts")):
        o, c = np.asarray(g["offsets"], dtype=np.int64).reshape(-1), np.maximum(np.asarray(g["counts"], dtype=np.int64).reshape(-1), 0)
        if n and not bool(((o >= 0) & (o + c <= int(pts.shape[0]))).all()):
            raise ValueError("%s: a contour's run of points leaves the point list" % who)
    else:
        inside = (offs >= 0) & (offs + cnts.clamp(min=0) <= int(pts.shape[0]))
        cnts = torch.where(inside, cnts, torch.zeros_like(cnts))
    if pts.shape[0] == 0:
        pts = torch.zeros((1, 2), dtype=torch.int32, device=dev)
    return pts, offs, cnts, col


def draw_contours_device(image, groups, up=1):
    """image: uint8 [H, W, 3] RGB, numpy or CUDA; groups: a list of {'points' [P, 2] (x, y), 'offsets' [n], 'counts' [n], 'colours' uint32 [n]
    (R | G << 8 | B << 16), 'width' 1..255, 'mul' 1..16, 'div' 1..4096, 'origin' (x, y)}, arrays numpy or CUDA.  Contour i of a group is the closed
    polygon through points[offsets[i] : offsets[i] + counts[i]], each point taken through (p mul - origin) / div (toward zero).  Groups are drawn in
    list order and contours in array order, later over earlier.  -> CUDA uint8 [H up, W up, 3]: the image up-scaled (nearest) with the strokes on it.
    One clear, one stamp per group and one resolve on the current stream, with no host wait in between."""
    import ctypes as C

    import torch

    from . import _lib

    L = _lib.lib()
    if isinstance(image, torch.Tensor):
        if not image.is_cuda:
            image = image.cuda()
        src = image
    else:
        src = torch.from_numpy(np.ascontiguousarray(np.asarray(image))).cuda()
    if src.dtype != torch.uint8 or src.dim() != 3 or src.shape[2] != 3:
        raise ValueError("draw_contours_device: the image must be uint8 [H, W, 3], got %s %s" % (src.dtype, tuple(src.shape)))
    if src.stride(2) != 1 or src.stride(1) != 3:
        src = src.contiguous()
    dev = src.device
    h, w, up = int(src.shape[0]), int(src.shape[1]), int(up)
    oh, ow = h * up, w * up
    if not (1 <= up <= 8) or min(h, w) < 1 or max(oh, ow) > OVERLAY_MAX_SIDE:
        raise ValueError("draw_contours_device: up must be 1..8 and the picture's sides 1..%d, got a %d x %d image with up=%r" % (OVERLAY_MAX_SIDE, h, w, up))
    packed = [_group_to_device(g, dev) for g in groups]
    total = sum(int(p[2].shape[0]) for p in packed)
    colours = torch.cat([p[3] for p in packed]) if total else torch.zeros(1, dtype=torch.int32, device=dev)
    ws_bytes = int(L.cerb_overlay_workspace_bytes(oh, ow))
    ws = torch.empty(ws_bytes // 4, dtype=torch.int32, device=dev)
    dst = torch.empty((oh, ow, 3), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        _lib.check(L.cerb_overlay_clear(ws.data_ptr(), ws_bytes, oh, ow, stream))
        first = 0
        for g, (pts, offs, cnts, _) in zip(groups, packed):
            n = int(cnts.shape[0])
            if n:
                ox, oy = (int(v) for v in g.get("origin", (0, 0)))
                _lib.check(L.cerb_overlay_stamp(pts.data_ptr(), offs.data_ptr(), cnts.data_ptr(), n, int(g.get("mul", 1)), int(g.get("div", 1)), ox, oy,
                                                int(g["width"]), first, ws.data_ptr(), ws_bytes, oh, ow, stream))
            first += n
        _lib.check(L.cerb_overlay_resolve(src.data_ptr(), int(src.stride(0)), h, w, up, colours.data_ptr(), total, ws.data_ptr(), ws_bytes,
                                          dst.data_ptr(), int(dst.stride(0)), oh, ow, stream))
    return dst


def pack_parts(parts, extra=None, viz_info=None, ds=1, origin=(0, 0), line_width=None):
    """The groups draw_contours_device takes (host arrays) for the instance arrays of a slide or tile.  parts: [(tissue, tab, cnts, pts, offs,
    has_type, ds_factor[, per-instance origin])] as collect_wsi_inst_arrays / build_from_parts have them; extra: {tissue: {key: ready dictionary}}
    (the per-region dictionaries of masked slides, already in the dictionary's coordinates).  Draw order Gland, Lumen, Nuclei whatever order the
    parts come in; instances info_from_table drops (area == 0, fewer than 3 points) get a count of 0; a part whose ds_factor is 0.5 is drawn with
    mul = 2, and per-instance tile origins are added here, on the host, as info_from_table adds them (np.round(p / ds_factor) + origin)."""
    from .inst_info import _shift_points

    viz_info = DEFAULT_VIZ_INFO if viz_info is None else viz_info
    ox, oy = (int(v) for v in origin)
    groups = []
    for tissue in DRAW_ORDER:
        vi = viz_info[tissue.lower()]
        width = int(vi["line_width"] if line_width is None else line_width)
        for part in parts or ():
            if part[0] != tissue:
                continue
            _, tab, cnts, pts, offs, has_type, ds_factor = part[:7]
            inst_origin = part[7] if len(part) > 7 else None
            tab, cnts, offs = np.asarray(tab), np.asarray(cnts), np.asarray(offs, dtype=np.int64)
            n = int(tab.shape[0])
            if n == 0:
                continue
            counts = np.where((tab[:, 0] > 0) & (cnts >= 3), cnts, 0).astype(np.int32)
            pts = np.asarray(pts).reshape(-1, 2)
            mul = 1
            if float(ds_factor) == 0.5 and inst_origin is None:
                mul = 2  # np.round(p / 0.5) of an integer is 2 p: multiplied on the device
            elif float(ds_factor) != 1.0:
                pts = np.round(pts / float(ds_factor)).astype("int")
            if inst_origin is not None:
                org, c64 = np.asarray(inst_origin, dtype=np.int64).reshape(n, 2), cnts.astype(np.int64)
                if len(pts) == int(c64.sum()) and np.array_equal(offs, np.cumsum(c64) - c64):  # the runs are the list, in order: one repeat
                    pts = pts.astype(np.int64) + np.repeat(org, c64, axis=0)
                else:
                    pts = _shift_points(pts.astype(np.int64), cnts, offs, org)
            groups.append({"points": pts, "offsets": offs, "counts": counts, "colours": contour_colours(tissue, tab, bool(has_type), viz_info),
                           "width": width, "mul": mul, "div": int(ds), "origin": (ox, oy)})
        if extra and extra.get(tissue):
            g = _pack_dict(tissue, extra[tissue], vi, width)
            g["counts"] = np.where(g["counts"] >= 3, g["counts"], 0).astype(np.int32)
            g["div"], g["origin"] = int(ds), (ox, oy)
            groups.append(g)
    return groups


def overlay_from_parts(image, parts, extra=None, viz_info=None, up=1, ds=1, origin=(0, 0), line_width=None):
    """The overlay of a tile or slide from its instance ARRAYS, without a dictionary: image (uint8 [H, W, 3], numpy or CUDA) up-scaled by `up` with
    every instance of `parts` and `extra` (see pack_parts) drawn on it at (p - origin) / ds, p in the instance dictionary's coordinates.
    line_width=None: the tissue's viz_info width.  -> CUDA uint8 [H up, W up, 3]."""
    return draw_contours_device(image, pack_parts(parts, extra, viz_info, ds, origin, line_width), up)


def half_width_viz_info(viz_info=None):
    """viz_info with every line width halved, at least 1 (gland 6, lumen 6, nuclei 1): the tile overlay draws the full widths on a picture at x2
    magnification, so this is the same look on one at x1."""
    viz_info = DEFAULT_VIZ_INFO if viz_info is None else viz_info
    return {k: dict(v, line_width=max(1, int(v["line_width"]) // 2)) for k, v in viz_info.items()}


def _pad_edge_(pic, hv, wv):
    """edge replication, in place, of the valid hv x wv pixels of a device picture out to its full size (np.pad(valid, mode="edge"))"""
    if wv < pic.shape[1]:
        pic[:hv, wv:] = pic[:hv, wv - 1:wv]
    if hv < pic.shape[0]:
        pic[hv:] = pic[hv - 1:hv]


def pyramid_windows(width, height, tile, rows):
    """[(x0, y0, x1, y1)] of level 0: row strips `rows` high, cut into column windows where the slide is wider than 32768; sides are multiples of
    2 tile (so every window starts at an even pixel and on the tile grid) except where the slide ends"""
    cols = OVERLAY_MAX_SIDE // (2 * tile) * (2 * tile)
    return [(x0, y0, min(x0 + cols, width), min(y0 + rows, height)) for y0 in range(0, height, rows) for x0 in range(0, width, cols)]


def pyramid_device_bytes(width, height, tile, rows):
    """what slide_overlay_pyramid holds on the device for a window height of `rows`: (resident levels 1 .., one window: pixels read + picture drawn +
    padded picture, the overlay plane, the tile encoder)"""
    from .tiff_pyramid import TileEncoder, level_sizes

    def up(v):
        return -(-v // tile) * tile

    sizes = level_sizes(width, height, tile)
    cw, ch = min(up(width), OVERLAY_MAX_SIDE // (2 * tile) * (2 * tile)), min(up(height), rows)
    resident = sum(3 * up(w) * up(h) for w, h in sizes[1:])
    return resident, 9 * cw * ch, 4 * cw * ch, TileEncoder.price(cw, ch, tile)


def slide_overlay_pyramid(reader, proc_res, parts, extra, path, tile=256, quality=75, viz_info=None, window_rows=None, timings=None):
    """The slide at the processing resolution (proc_res microns per pixel, as tissue.thumbnail reads it at ds = 1) with every instance of `parts` and
    `extra` (see pack_parts) drawn on it at HALF the tissue's line width, written to `path` as a pyramidal JPEG-tiled BigTIFF
    (cerberus_amd/tiff_pyramid.py; 4:2:0).  Level 0 is walked in windows (pyramid_windows): pixels from reader.read_bounds, strokes from
    draw_contours_device through a translated origin, each window reduced x2 (cerb_resample_box: exact means, half to even, clamped at the slide's
    edge) into a RESIDENT level 1 and encoded tile by tile on the device; levels 1, 2, .. are then encoded in windows and reduced in turn.  Padding
    out to the tile grid replicates the edge of the level's own pixels.  Memory is priced before anything is allocated: window_rows=None takes the
    tallest window that fits (a multiple of 2 tile), and a slide that does not fit with the smallest raises ValueError naming the bytes.
    timings: a dictionary that receives seconds per stage (read, draw, reduce, encode, download, write; the device is then waited for between the
    stages), the file's size and the peak device bytes.  -> [(w, h)] of the levels."""
    import ctypes as C
    import os
    import time

    import torch

    from . import _lib
    from .tiff_pyramid import PyramidWriter, TileEncoder, check_tile, level_sizes

    tile = check_tile(tile)
    s = reader._scale(proc_res, "mpp")
    W, H = (max(1, int(v)) for v in reader.slide_dimensions(s, "baseline"))
    dev = torch.device("cuda", torch.cuda.current_device())
    step = 2 * tile

    def up(v, m=tile):
        return -(-v // m) * m

    free = int(torch.cuda.mem_get_info(dev)[0])
    if window_rows is None:
        # at most 2^26 pixels a window (more brings no more parallelism), halved until the device has room
        rows = max(step, min(up(H, step), OVERLAY_MAX_SIDE // step * step, (1 << 26) // min(up(W), OVERLAY_MAX_SIDE) // step * step))
        while rows > step and sum(pyramid_device_bytes(W, H, tile, rows)) > 0.9 * free:
            rows = max(step, rows // 2 // step * step)
    else:
        rows = int(window_rows)
        if rows < step or rows % step or rows > OVERLAY_MAX_SIDE:
            raise ValueError("slide_overlay_pyramid: window_rows must be a multiple of 2 tile = %d up to %d, got %r" % (step, OVERLAY_MAX_SIDE, window_rows))
    need = pyramid_device_bytes(W, H, tile, rows)
    if sum(need) > 0.9 * free:
        raise ValueError("slide_overlay_pyramid: a %d x %d slide at tile %d needs %d bytes on the device with the smallest window (%d rows): %d for the resident "
                         "levels, %d for a window, %d for the overlay plane, %d for the tile encoder; %d are free"
                         % ((W, H, tile, sum(need), rows) + need + (free,)))
    L = _lib.lib()
    sizes = level_sizes(W, H, tile)
    proc_mpp = float(np.atleast_1d(proc_res)[0]) if reader.info.mpp is not None else None
    writer = PyramidWriter(path, W, H, tile, quality, 2, mpp=proc_mpp)
    took = dict.fromkeys(("read", "draw", "reduce", "encode", "download", "write"), 0.0)
    clock = [time.perf_counter()]

    def lap(stage):
        if timings is not None:
            torch.cuda.synchronize(dev)
            now = time.perf_counter()
            took[stage] += now - clock[0]
            clock[0] = now

    def emit(enc, level, pic, x0, y0):
        """the tiles of `pic`, whose top left tile is the level's tile (y0 / tile, x0 / tile), encoded and appended to the file"""
        handle = enc.encode(pic, quality, 2)
        lap("encode")
        data, offsets, counts = handle.tiles()
        lap("download")
        across = writer.grids[level][0]
        ty, tx = np.mgrid[0:pic.shape[0] // tile, 0:pic.shape[1] // tile]
        writer.add_tiles(level, ((ty + y0 // tile) * across + tx + x0 // tile).reshape(-1), data, offsets, counts)
        lap("write")

    def reduce(src, hv, wv, dst):
        """dst (a view whose first pixel is the one src's first 2 x 2 box becomes) <- the x2 reduction of src's valid hv x wv pixels"""
        _lib.check(L.cerb_resample_box(src.data_ptr(), int(src.stride(0)), hv, wv, 2, dst.data_ptr(), int(dst.stride(0)), -(-hv // 2), -(-wv // 2),
                                       C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))

    try:
        if timings is not None:
            torch.cuda.reset_peak_memory_stats(dev)
        with torch.cuda.device(dev):
            levels = [None] + [torch.empty((up(h), up(w), 3), dtype=torch.uint8, device=dev) for w, h in sizes[1:]]
            cw = min(up(W), OVERLAY_MAX_SIDE // step * step)
            enc = TileEncoder(dev, cw, min(up(H), rows), tile)
            pic = torch.empty((min(up(H), rows), cw, 3), dtype=torch.uint8, device=dev)
            groups = pack_parts(parts, extra, half_width_viz_info(viz_info), ds=1, origin=(0, 0))
            for g in groups:  # uploaded once; a window only moves the origin
                g["points"], g["offsets"], g["counts"], g["colours"] = _group_to_device(g, dev)
            clock[0] = time.perf_counter()
            for x0, y0, x1, y1 in pyramid_windows(W, H, tile, rows):
                hv, wv = y1 - y0, x1 - x0
                pixels = torch.from_numpy(np.ascontiguousarray(reader.read_bounds((x0, y0, x1, y1), resolution=s, units="baseline")[..., :3])).to(dev)
                lap("read")
                drawn = draw_contours_device(pixels, [dict(g, origin=(x0, y0)) for g in groups])
                lap("draw")
                if len(sizes) > 1:
                    reduce(drawn, hv, wv, levels[1][y0 // 2:, x0 // 2:])
                    lap("reduce")
                view = pic[:up(hv), :up(wv)]
                view[:hv, :wv] = drawn
                _pad_edge_(view, hv, wv)
                emit(enc, 0, view, x0, y0)
                pixels = drawn = None
            for k in range(1, len(sizes)):
                w, h = sizes[k]
                if k + 1 < len(sizes):
                    reduce(levels[k], h, w, levels[k + 1])
                _pad_edge_(levels[k], h, w)
                lap("reduce")
                for x0, y0, x1, y1 in pyramid_windows(up(w), up(h), tile, min(up(H), rows)):
                    emit(enc, k, levels[k][y0:y1, x0:x1], x0, y0)
                levels[k] = None
        writer.close()
    except BaseException:
        writer.abort()
        raise
    if timings is not None:
        timings.update(took, file_bytes=os.path.getsize(path), peak_device_bytes=int(torch.cuda.max_memory_allocated(dev)), window_rows=rows)
    return sizes


def visualize_instances_dict_device(input_image, inst_dict_, viz_info=None):
    """visualize_instances_dict_orig for callers who hold a dictionary, drawn on the device: same arguments, same kind of result (a new uint8 RGB
    numpy array), same tissue order, colours and widths; the stroke is the integer definition of include/cerberus_hip.h instead of PIL's."""
    viz_info = DEFAULT_VIZ_INFO if viz_info is None else viz_info
    groups = [_pack_dict(t, inst_dict_[t], viz_info[t.lower()]) for t in DRAW_ORDER if t in inst_dict_]
    return draw_contours_device(np.ascontiguousarray(np.asarray(input_image).astype(np.uint8)), groups, 1).cpu().numpy()
