"""Independent restatement of the overlay definition of include/cerberus_hip.h ("instance overlays"): a SEQUENTIAL painter -- one contour after the
other, one segment after the other, later over earlier -- in numpy int64 with math.isqrt, plus the same predicate in plain Python integers.  Shares
no code with cerberus_amd; the tests demand equality with it, bit for bit."""
import math

import numpy as np

COORD_MAX = 1 << 20


def covered_int(px, py, ax, ay, bx, by, w):
    """Is the centre of pixel (px, py) within w / 2 of the segment a -> b?  Python integers: cannot overflow."""
    vx, vy, ux, uy = bx - ax, by - ay, px - ax, py - ay
    vv, t = vx * vx + vy * vy, ux * vx + uy * vy
    if vv == 0 or t <= 0:
        return 4 * (ux * ux + uy * uy) <= w * w
    if t >= vv:
        return 4 * ((px - bx) ** 2 + (py - by) ** 2) <= w * w
    return abs(ux * vy - uy * vx) <= math.isqrt((w * w * vv) // 4)


def covered_np(xs, ys, ax, ay, bx, by, w):
    """The same for int64 arrays of pixel coordinates (broadcast against each other) -> bool array."""
    xs, ys = np.asarray(xs, np.int64), np.asarray(ys, np.int64)
    ax, ay, bx, by, w = int(ax), int(ay), int(bx), int(by), int(w)
    vx, vy = np.int64(bx - ax), np.int64(by - ay)
    ux, uy = xs - np.int64(ax), ys - np.int64(ay)
    vv = int(vx) * int(vx) + int(vy) * int(vy)
    t = ux * vx + uy * vy
    at_a = 4 * (ux * ux + uy * uy) <= w * w
    if vv == 0:
        return at_a & np.ones(np.broadcast(xs, ys).shape, bool)
    dx, dy = xs - np.int64(bx), ys - np.int64(by)
    at_b = 4 * (dx * dx + dy * dy) <= w * w
    band = np.abs(ux * vy - uy * vx) <= np.int64(math.isqrt((w * w * vv) // 4))
    return np.where(t <= 0, at_a, np.where(t >= vv, at_b, band))


def transform(points, mul=1, div=1, origin=(0, 0)):
    """(p mul - origin) / div toward zero, int64 [K, 2]."""
    q = np.asarray(points, np.int64).reshape(-1, 2) * np.int64(mul) - np.asarray(origin, np.int64).reshape(1, 2)
    return np.sign(q) * (np.abs(q) // np.int64(div))


def paint_contour(prio, pts, width, ordinal, full=False):
    """Closed contour through pts (already transformed, int64 [K, 2]) into the priority plane, sequentially: every covered pixel takes `ordinal`
    (the caller paints in ascending ordinals, so plain assignment is the painter's order).  full: test every pixel of the image; otherwise only a
    generous box of `width + 2` round the segment -- test_overlay_host.py holds the two equal."""
    h, w = prio.shape
    k = len(pts)
    if k == 0 or (np.abs(pts) > COORD_MAX).any():
        return
    for s in range(1 if k <= 2 else k):
        ax, ay = (int(v) for v in pts[s])
        bx, by = (int(v) for v in pts[(s + 1) % k])
        if full:
            x0, x1, y0, y1 = 0, w - 1, 0, h - 1
        else:
            m = width + 2
            x0, x1, y0, y1 = max(0, min(ax, bx) - m), min(w - 1, max(ax, bx) + m), max(0, min(ay, by) - m), min(h - 1, max(ay, by) + m)
            if x0 > x1 or y0 > y1:
                continue
        ys, xs = np.arange(y0, y1 + 1, dtype=np.int64)[:, None], np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
        hit = covered_np(xs, ys, ax, ay, bx, by, width)
        view = prio[y0:y1 + 1, x0:x1 + 1]
        view[hit] = ordinal


def paint_group(prio, points, offsets, counts, width, first_ordinal=0, mul=1, div=1, origin=(0, 0), full=False):
    """One stamp call: contour i gets ordinal first_ordinal + i + 1.  -> first_ordinal for the next group."""
    points = np.asarray(points, np.int64).reshape(-1, 2)
    for i, (o, c) in enumerate(zip(np.asarray(offsets).tolist(), np.asarray(counts).tolist())):
        if c > 0:
            paint_contour(prio, transform(points[o:o + c], mul, div, origin), int(width), first_ordinal + i + 1, full)
    return first_ordinal + len(counts)


def resolve(src, prio, colours, up=1):
    """-> uint8 [h up, w up, 3]: colours[prio - 1] (uint32 words R | G << 8 | B << 16) where prio != 0, src[y // up][x // up] elsewhere."""
    out = np.repeat(np.repeat(np.asarray(src, np.uint8), up, axis=0), up, axis=1).copy()
    assert out.shape[:2] == prio.shape
    colours = np.asarray(colours, np.uint32)
    ys, xs = np.nonzero(prio)
    c = colours[prio[ys, xs].astype(np.int64) - 1]
    out[ys, xs, 0], out[ys, xs, 1], out[ys, xs, 2] = c & 255, (c >> 8) & 255, (c >> 16) & 255
    return out


def draw(image, groups, up=1, full=False):
    """cerberus_amd.viz.draw_contours_device restated: groups of {'points', 'offsets', 'counts', 'colours', 'width', 'mul', 'div', 'origin'}."""
    image = np.asarray(image, np.uint8)
    prio = np.zeros((image.shape[0] * up, image.shape[1] * up), np.uint32)
    first, colours = 0, []
    for g in groups:
        first = paint_group(prio, g["points"], g["offsets"], g["counts"], g["width"], first, g.get("mul", 1), g.get("div", 1), g.get("origin", (0, 0)), full)
        colours.append(np.asarray(g["colours"], np.uint32))
    return resolve(image, prio, np.concatenate(colours) if colours else np.zeros(0, np.uint32), up)


def colour_word(rgb):
    return int(rgb[0]) | (int(rgb[1]) << 8) | (int(rgb[2]) << 16)


def dict_groups(inst_dict, viz_info, order=("Gland", "Lumen", "Nuclei"), width=None, div=1, min_points=2):
    """The groups of an instance dictionary {tissue: {id: {'contour', 'type'?}}}: tissue order, type colour else instance colour."""
    groups = []
    for tissue in order:
        if tissue not in inst_dict:
            continue
        vi = viz_info[tissue.lower()]
        pts, cnts, cols = [], [], []
        for info in inst_dict[tissue].values():
            c = info.get("contour")
            if c is None or len(c) < min_points:
                continue
            pts.append(np.asarray(c, np.int64).reshape(-1, 2))
            cnts.append(len(c))
            rgb = vi["type_colour"].get(int(info["type"]), vi["inst_colour"]) if "type" in info else vi["inst_colour"]
            cols.append(colour_word(rgb))
        cnts = np.asarray(cnts, np.int64)
        groups.append({"points": np.concatenate(pts) if pts else np.zeros((0, 2), np.int64), "offsets": np.cumsum(cnts) - cnts, "counts": cnts,
                       "colours": np.asarray(cols, np.uint32), "width": int(vi["line_width"] if width is None else width), "mul": 1, "div": div, "origin": (0, 0)})
    return groups
