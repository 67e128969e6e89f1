"""Label maps from instance contours, on the device: the step back from an instance dictionary (dat/<slide>.dat, the reference's save_json files, QuPath /
GeoJSON polygons) to the int32 label maps that compute_stats.py, compute_features.py and targets.gen_targets take.

The definition is include/cerberus_hip.h's ("label maps from contours"): the even-odd interior on pixel centres (cerb_overlay_fill) plus the width-1
outline of the same contour (cerb_overlay_stamp), painted into the overlay's priority plane, and one pass that turns the plane into labels
(cerb_overlay_labels).  It is the project's own, in integers; cv2.drawContours(thickness=FILLED) is not pinned.  Interior rings
(holes) are not supported: the loaders drop them and say how many.  Nothing here fills on the host."""
import json
import os
from collections import OrderedDict

import numpy as np

from .viz import DRAW_ORDER, OVERLAY_MAX_SIDE

PLANE_BYTES = 1 << 30  # a map with a side above OVERLAY_MAX_SIDE is filled in windows whose plane stays under this


def fill_windows(h, w, window=None):
    """[(x0, y0, x1, y1)]: the whole map when both sides fit the plane (and no window is asked for), otherwise windows whose plane stays under 1 GiB."""
    if window is None:
        if max(h, w) <= OVERLAY_MAX_SIDE:
            return [(0, 0, w, h)]
        ww = min(w, 16384)
        wh = min(h, OVERLAY_MAX_SIDE, (PLANE_BYTES // 4 - 1) // ww)
    else:
        wh, ww = (int(v) for v in window)
        if not (1 <= wh <= OVERLAY_MAX_SIDE and 1 <= ww <= OVERLAY_MAX_SIDE):
            raise ValueError("fill_contours_device: a window's sides must be 1..%d, got %r" % (OVERLAY_MAX_SIDE, window))
    return [(x0, y0, min(x0 + ww, w), min(y0 + wh, h)) for y0 in range(0, h, wh) for x0 in range(0, w, ww)]


def _int32_table(values, n, dev, name):
    import torch

    if isinstance(values, torch.Tensor):
        t = values.to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
    else:
        a = np.asarray(values)
        if a.size and (a.dtype.kind not in "iub" or a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError("fill_contours_device: %r must be integers that fit int32" % name)
        t = torch.from_numpy(np.ascontiguousarray(a.astype(np.int32)).reshape(-1)).to(dev)
    if int(t.shape[0]) != n:
        raise ValueError("fill_contours_device: %r must have one entry per contour (%d), got %d" % (name, n, int(t.shape[0])))
    return t


def fill_contours_device(shape, groups, background=0, window=None):
    """shape: (H, W); groups: a list of {'points' [P, 2] (x, y), 'offsets' [n], 'counts' [n], 'ids' int32 [n] (optional), 'types' [n] (optional),
    'mul' 1..16, 'div' 1..4096, 'origin' (x, y)}, arrays numpy or CUDA -- the groups of viz.draw_contours_device with 'ids' in place of 'colours'.
    Contour i of a group is the closed polygon through points[offsets[i] : offsets[i] + counts[i]], each point taken through (p mul - origin) / div
    (toward zero); its FILLED SET -- the even-odd interior plus its width-1 outline -- takes the value ids[i].  Groups without 'ids' number their
    contours on: 1, 2, .. over the groups.  Later contours lie over earlier ones; several contours may share an id.
    -> CUDA int32 [H, W] (`background` where nothing was filled); when a group carries 'types', a pair (label map, uint8 class map: types[i] over the
    same pixels, 0 elsewhere and for groups without types).
    One clear, then fill + stamp(width 1) per group, then one labels pass per map, on the current stream with no host wait.  A map with a side above
    32768 is filled in windows through `origin` (window=(h, w): windows of that size for any map); that needs div == 1 in every group, because the
    division truncates toward zero and so does not commute with a translation."""
    import ctypes as C

    import torch

    from . import _lib
    from .viz import _group_to_device

    h, w = (int(v) for v in shape)
    if h < 1 or w < 1:
        raise ValueError("fill_contours_device: shape must be (H, W) with both sides at least 1, got %r" % (tuple(shape),))
    background = int(background)
    if not -2 ** 31 <= background < 2 ** 31:
        raise ValueError("fill_contours_device: background must fit int32")
    windows = fill_windows(h, w, window)
    if len(windows) > 1 and any(int(g.get("div", 1)) != 1 for g in groups):
        raise ValueError("fill_contours_device: a %d x %d map is filled in windows, which needs div == 1 in every group" % (h, w))
    dev = torch.device("cuda", torch.cuda.current_device())
    L = _lib.lib()
    packed, ids, types, first = [], [], [], 0
    with_types = any(g.get("types") is not None for g in groups)
    for g in groups:
        n = int(g["counts"].shape[0]) if hasattr(g["counts"], "shape") else len(g["counts"])
        pts, offs, cnts, _ = _group_to_device(dict(g, colours=np.zeros(n, np.uint32)), dev, "fill_contours_device")
        packed.append((pts, offs, cnts))
        ids.append(torch.arange(first + 1, first + n + 1, dtype=torch.int32, device=dev) if g.get("ids") is None else _int32_table(g["ids"], n, dev, "ids"))
        if with_types:
            types.append(torch.zeros(n, dtype=torch.int32, device=dev) if g.get("types") is None else _int32_table(g["types"], n, dev, "types"))
        first += n
    total = first
    one = torch.zeros(1, dtype=torch.int32, device=dev)
    id_table = torch.cat(ids) if total else one
    type_table = (torch.cat(types) if total else one) if with_types else None
    out = torch.empty((h, w), dtype=torch.int32, device=dev)
    cls = torch.empty((h, w), dtype=torch.int32, device=dev) if with_types else None
    ph, pw = max(y1 - y0 for _, y0, _, y1 in windows), max(x1 - x0 for x0, _, x1, _ in windows)
    ws = torch.empty(ph * pw, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    with torch.cuda.device(dev):
        for x0, y0, x1, y1 in windows:
            wh, ww = y1 - y0, x1 - x0
            nb = int(L.cerb_overlay_workspace_bytes(wh, ww))
            _lib.check(L.cerb_overlay_clear(ws.data_ptr(), nb, wh, ww, stream))
            first = 0
            for g, (pts, offs, cnts) in zip(groups, packed):
                n = int(cnts.shape[0])
                if n:
                    mul, div = int(g.get("mul", 1)), int(g.get("div", 1))
                    ox, oy = (int(v) for v in g.get("origin", (0, 0)))
                    ox, oy = ox + x0, oy + y0  # (div == 1 whenever a window does not start at the map's corner)
                    _lib.check(L.cerb_overlay_fill(pts.data_ptr(), offs.data_ptr(), cnts.data_ptr(), n, mul, div, ox, oy, first, ws.data_ptr(), nb, wh, ww, stream))
                    _lib.check(L.cerb_overlay_stamp(pts.data_ptr(), offs.data_ptr(), cnts.data_ptr(), n, mul, div, ox, oy, 1, first, ws.data_ptr(), nb, wh, ww, stream))
                first += n
            for table, dst, bg in ((id_table, out, background), (type_table, cls, 0)):
                if dst is not None:
                    view = dst[y0:y1, x0:x1]
                    _lib.check(L.cerb_overlay_labels(table.data_ptr(), total, bg, ws.data_ptr(), nb, view.data_ptr(), int(dst.stride(0)) * 4, wh, ww, stream))
    return (out, cls.to(torch.uint8)) if with_types else out


def label_maps_from_parts(parts, extra, shape, ds=1, origin=(0, 0)):
    """Label maps of a slide or tile from its instance ARRAYS.  parts / extra: as viz.pack_parts takes them, with its conventions (mul = 2 for a part
    whose ds_factor is 0.5, per-instance origins added on the host, instances info_from_table drops -- area 0, fewer than 3 points -- get a count of
    0 and so fill nothing).  The id of an instance is its table row + 1 (the key info_from_table gives it); the entries of extra[tissue] number on
    after the tissue's parts.  shape: (H, W) of the maps, which show the dictionary's coordinates p at (p - origin) / ds.
    -> {tissue: (CUDA int32 label map, CUDA uint8 class map or None)}: majority types (inst_info.majority_type) where the part has types."""
    from .inst_info import majority_type
    from .viz import pack_parts

    out = OrderedDict()
    for tissue in DRAW_ORDER:
        groups, first, typed = [], 0, False
        for part in parts or ():
            if part[0] != tissue:
                continue
            tab = np.asarray(part[1])
            n = int(tab.shape[0])
            for g in pack_parts([part], None, None, ds, origin):
                g["ids"] = np.arange(first + 1, first + n + 1, dtype=np.int32)
                if part[5]:
                    g["types"], typed = majority_type(tab).astype(np.int32), True
                groups.append(g)
            first += n
        if extra and extra.get(tissue):
            for g in pack_parts(None, {tissue: extra[tissue]}, None, ds, origin):
                n = len(g["counts"])
                g["ids"] = np.arange(first + 1, first + n + 1, dtype=np.int32)
                kept = [info for info in extra[tissue].values() if info.get("contour") is not None and len(info["contour"]) >= 2]
                if any("type" in info for info in kept):
                    g["types"], typed = np.asarray([int(info.get("type", 0)) for info in kept], np.int32), True
                groups.append(g)
                first += n
        if not groups and not any(p[0] == tissue for p in parts or ()) and not (extra and tissue in extra):
            continue
        for g in groups:
            g.pop("colours", None), g.pop("width", None)
        res = fill_contours_device(shape, groups)
        out[tissue] = res if typed else (res, None)
    return out


def dict_tissues(inst_dict):
    """The keys of an instance dictionary that hold instances ({key: {'contour': ..}}), in the dictionary's order -- not its resolution entries."""
    return [k for k, v in inst_dict.items() if isinstance(v, dict) and all(isinstance(e, dict) for e in v.values())]


def dict_group(insts, mul=1, div=1, origin=(0, 0)):
    """One tissue of an instance dictionary as a group of fill_contours_device: ids 1 .. n in dictionary order (an entry without a contour keeps its id and
    fills nothing), 'more_contours' (the further rings of a MultiPolygon, load_annotations) under the same id.  -> (group, class vector by id or None)"""
    pts, cnts, ids, types = [], [], [], np.zeros(len(insts) + 1, np.int32)
    typed = False
    for i, info in enumerate(insts.values(), 1):
        if "type" in info and info["type"] is not None:
            types[i], typed = int(info["type"]), True
        rings = ([] if info.get("contour") is None else [info["contour"]]) + list(info.get("more_contours", ()))
        for ring in rings:
            c = np.asarray(ring).reshape(-1, 2)
            pts.append(c.astype(np.int64))
            cnts.append(c.shape[0])
            ids.append(i)
    counts = np.asarray(cnts, np.int32)
    group = {"points": np.concatenate(pts) if pts else np.zeros((0, 2), np.int64), "offsets": np.cumsum(counts, dtype=np.int64) - counts, "counts": counts,
             "ids": np.asarray(ids, np.int32), "mul": int(mul), "div": int(div), "origin": tuple(int(v) for v in origin)}
    return group, (types if typed else None)


def label_maps_from_dict(inst_dict, shape=None, tissues=None, div=1):
    """Label maps of an instance dictionary {tissue: {key: {'contour': (K, 2) (x, y), 'type'?}}, ..} (dat/<slide>.dat, load_annotations).  shape: (H, W);
    None takes the dictionary's 'proc_dimensions' (YX).  tissues: which to fill (default: all it holds).  div: an integer, or {tissue: integer}, to fill
    a tissue at 1 / div of the dictionary's resolution (its map is then ceil(shape / div)).  Instance ids are 1 .. n in dictionary order.
    -> {tissue: (CUDA int32 map, int32 class vector indexed by id -- numpy, entry 0 is 0 -- or None when no instance has a type)}"""
    if shape is None:
        if "proc_dimensions" not in inst_dict:
            raise ValueError("label_maps_from_dict: the dictionary has no 'proc_dimensions': give the shape")
        shape = tuple(int(v) for v in np.asarray(inst_dict["proc_dimensions"]).reshape(-1)[:2])
    h, w = (int(v) for v in shape)
    out = OrderedDict()
    for tissue in (dict_tissues(inst_dict) if tissues is None else tissues):
        if tissue not in inst_dict:
            raise ValueError("label_maps_from_dict: the dictionary holds no %r" % (tissue,))
        d = int(div.get(tissue, 1) if isinstance(div, dict) else div)
        group, types = dict_group(inst_dict[tissue], div=d)
        out[tissue] = (fill_contours_device((-(-h // d), -(-w // d)), [group]), types)
    return out


# ---- annotations that come as polygons ------------------------------------------------------------------------------------------------------------------
def _ring(coords, what):
    a = np.asarray(coords, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] < 2:
        raise ValueError("%s: a ring must be a list of [x, y] positions" % what)
    a = np.round(a[:, :2]).astype(np.int64)  # (QuPath writes fractions of a pixel)
    if len(a) > 1 and (a[0] == a[-1]).all():
        a = a[:-1]  # GeoJSON closes a ring by repeating its first position; contours here are closed by definition
    return a


def _load_geojson(doc, path, tissue):
    if not isinstance(doc, dict) or doc.get("type") != "FeatureCollection":
        raise ValueError("%s: a GeoJSON annotation file must be a FeatureCollection, got %r" % (path, doc.get("type") if isinstance(doc, dict) else type(doc).__name__))
    out, holes = OrderedDict(), 0
    for k, feat in enumerate(doc.get("features", ())):
        geom = (feat or {}).get("geometry") or {}
        kind = geom.get("type")
        if kind == "Polygon":
            polys = [geom["coordinates"]]
        elif kind == "MultiPolygon":
            polys = list(geom["coordinates"])
        else:
            raise ValueError("%s: feature %d has geometry %r; only Polygon and MultiPolygon are filled" % (path, k, kind))
        name = (((feat.get("properties") or {}).get("classification") or {}).get("name")) or tissue
        if not name:
            raise ValueError("%s: feature %d has no properties.classification.name: name the tissue" % (path, k))
        rings = []
        for poly in polys:
            if not poly:
                continue
            rings.append(_ring(poly[0], path))
            holes += len(poly) - 1  # interior rings: dropped and counted
        if not rings:
            continue
        entry = {"contour": rings[0]}
        if len(rings) > 1:
            entry["more_contours"] = rings[1:]
        dst = out.setdefault(str(name), OrderedDict())
        key = feat.get("id")
        dst[len(dst) + 1 if key is None or key in dst else key] = entry
    return out, holes


def load_annotations(path, tissue=None):
    """Polygon annotations as an instance dictionary {tissue: {key: {'contour': int64 (K, 2) (x, y), 'more_contours'?: [..], 'type'?: int}}, ..} for
    label_maps_from_dict.  By extension:
      .dat      an instance dictionary as run_infer_wsi.py writes it (a plain pickle; its resolution entries are kept)
      .json     the reference's save_json file, {"mag": .., "instances": {tissue: {id: {.., "contour", "type"}}}} ("mag" is kept under that key)
      .geojson  a FeatureCollection (QuPath's export): of a Polygon the exterior ring, of a MultiPolygon every exterior ring under ONE key; a ring's
                closing duplicate is dropped, positions are rounded to whole pixels; properties.classification.name names the tissue, otherwise
                `tissue` does.  Interior rings (holes) are dropped.
    -> (dictionary, number of interior rings dropped).  Any other extension, top-level object or geometry is refused by name (ValueError)."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".dat":
        import pickle

        with open(path, "rb") as fh:
            doc = pickle.load(fh)
        if not isinstance(doc, dict):
            raise ValueError("%s: a .dat annotation file must hold a dictionary, got %s" % (path, type(doc).__name__))
        return doc, 0
    if ext == ".json":
        with open(path) as fh:
            doc = json.load(fh)
        if not isinstance(doc, dict) or not isinstance(doc.get("instances"), dict):
            raise ValueError("%s: not a {\"mag\", \"instances\": {tissue: {id: {..}}}} file" % path)
        out = OrderedDict()
        for name, insts in doc["instances"].items():
            dst = out[name] = OrderedDict()
            for key, info in insts.items():
                entry = {"contour": None if info.get("contour") is None else np.asarray(info["contour"], np.int64).reshape(-1, 2)}
                if info.get("type") is not None:
                    entry["type"] = int(info["type"])
                dst[key] = entry
        out["mag"] = doc.get("mag")
        return out, 0
    if ext == ".geojson":
        with open(path) as fh:
            doc = json.load(fh)
        return _load_geojson(doc, path, tissue)
    raise ValueError("%s: annotations are read from .dat, .json and .geojson files, not %r" % (path, ext))
