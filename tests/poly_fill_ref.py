"""Independent restatement of the polygon fill of include/cerberus_hip.h ("label maps from contours"): a SEQUENTIAL painter -- one contour after the
other, later over earlier -- in numpy int64, plus the crossing count of one pixel in plain Python integers and fractions.  The outline half reuses
tests/overlay_ref.py (transform, covered_np); nothing here shares code with cerberus_amd.  The tests demand equality with it, bit for bit."""
from fractions import Fraction

import numpy as np

import overlay_ref

COORD_MAX = overlay_ref.COORD_MAX


def crossings_int(px, py, pts):
    """How many edges of the closed polygon pts cross the ray from the centre of pixel (px, py) to the left -- in exact rationals: the edge a -> b
    counts iff min(ay, by) <= py < max(ay, by) and its x at that row, ax + (py - ay) (bx - ax) / (by - ay), is <= px (ceil(X) <= px iff X <= px)."""
    k, n = len(pts), 0
    for s in range(k):
        ax, ay = (int(v) for v in pts[s])
        bx, by = (int(v) for v in pts[(s + 1) % k])
        if min(ay, by) <= py < max(ay, by) and ax + Fraction((py - ay) * (bx - ax), by - ay) <= px:
            n += 1
    return n


def interior_int(h, w, pts):
    """bool [h, w]: the interior by counting every pixel's crossings on its own (slow: for small pictures)."""
    out = np.zeros((h, w), bool)
    if len(pts) >= 3:
        for y in range(h):
            for x in range(w):
                out[y, x] = crossings_int(x, y, pts) & 1
    return out


def interior_np(h, w, pts):
    """bool [h, w]: the same, edge by edge: every edge toggles, in each row it crosses, the pixels from xc = ax + ceil((y - ay) (bx - ax) / (by - ay))
    on.  The toggles are counted at their first column and summed along the row."""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    k = len(pts)
    if k < 3:
        return np.zeros((h, w), bool)
    first = np.zeros((h, w + 1), np.int64)
    for s in range(k):
        (ax, ay), (bx, by) = (int(v) for v in pts[s]), (int(v) for v in pts[(s + 1) % k])
        lo, hi = max(min(ay, by), 0), min(max(ay, by), h)  # rows lo .. hi - 1
        if lo >= hi:
            continue
        ys = np.arange(lo, hi, dtype=np.int64)
        num, den = (ys - ay) * np.int64(bx - ax), np.int64(by - ay)
        xc = ax - ((-num) // den)  # numpy's // floors, for either sign of den: -floor(-q) = ceil(q)
        np.add.at(first, (ys, np.clip(xc, 0, w)), 1)
    return (np.cumsum(first[:, :w], axis=1) & 1).astype(bool)


def outline_np(h, w, pts):
    """bool [h, w]: the width-1 stroke of the closed contour (overlay_ref's predicate; a count of 2 is one capsule, 1 a disk)."""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    k = len(pts)
    out = np.zeros((h, w), bool)
    for s in range(1 if k <= 2 else k):
        (ax, ay), (bx, by) = (int(v) for v in pts[s]), (int(v) for v in pts[(s + 1) % k])
        # a width-1 stroke reaches half a pixel: a box of 2 round the segment holds it (tests/test_overlay_host.py holds box and full picture equal)
        x0, x1, y0, y1 = max(0, min(ax, bx) - 2), min(w - 1, max(ax, bx) + 2), max(0, min(ay, by) - 2), min(h - 1, max(ay, by) + 2)
        if x0 > x1 or y0 > y1:
            continue
        ys, xs = np.arange(y0, y1 + 1, dtype=np.int64)[:, None], np.arange(x0, x1 + 1, dtype=np.int64)[None, :]
        out[y0:y1 + 1, x0:x1 + 1] |= overlay_ref.covered_np(xs, ys, ax, ay, bx, by, 1)
    return out


def fill_contour(prio, pts, ordinal, interior_only=False):
    """The filled set of one contour (pts already transformed, int64 [K, 2]) takes `ordinal` (the caller paints in ascending ordinals).  A contour with a
    coordinate beyond the range is skipped whole, interior and outline.  interior_only: what cerb_overlay_fill alone paints."""
    pts = np.asarray(pts, np.int64).reshape(-1, 2)
    if len(pts) == 0 or (np.abs(pts) > COORD_MAX).any():
        return
    h, w = prio.shape
    hit = interior_np(h, w, pts)
    if not interior_only:
        hit |= outline_np(h, w, pts)
    prio[hit] = ordinal


def fill_group(prio, points, offsets, counts, first_ordinal=0, mul=1, div=1, origin=(0, 0), interior_only=False):
    """One fill (+ stamp of width 1) call: contour i gets ordinal first_ordinal + i + 1.  -> first_ordinal for the next group."""
    points = np.asarray(points, np.int64).reshape(-1, 2)
    for i, (o, c) in enumerate(zip(np.asarray(offsets).tolist(), np.asarray(counts).tolist())):
        if c > 0:
            fill_contour(prio, overlay_ref.transform(points[o:o + c], mul, div, origin), first_ordinal + i + 1, interior_only)
    return first_ordinal + len(counts)


def labels(prio, table, background=0):
    """-> int32 [h, w]: table[prio - 1] where prio is in 1 .. len(table), background elsewhere."""
    table = np.asarray(table, np.int32).reshape(-1)
    out = np.full(prio.shape, background, np.int32)
    named = (prio > 0) & (prio <= len(table))
    out[named] = table[prio[named].astype(np.int64) - 1]
    return out


def fill(shape, groups, background=0):
    """cerberus_amd.rasterize.fill_contours_device restated: groups of {'points', 'offsets', 'counts', 'ids'?, 'types'?, 'mul', 'div', 'origin'}.
    -> (label map, class map or None)"""
    prio = np.zeros(tuple(shape), np.uint32)
    first, ids, types = 0, [], []
    for g in groups:
        n = len(g["counts"])
        ids.append(np.asarray(g["ids"], np.int32) if g.get("ids") is not None else np.arange(first + 1, first + n + 1, dtype=np.int32))
        types.append(np.asarray(g["types"], np.int32) if g.get("types") is not None else np.zeros(n, np.int32))
        first = fill_group(prio, g["points"], g["offsets"], g["counts"], first, g.get("mul", 1), g.get("div", 1), g.get("origin", (0, 0)))
    cat = (lambda v: np.concatenate(v) if v else np.zeros(0, np.int32))
    with_types = any(g.get("types") is not None for g in groups)
    return labels(prio, cat(ids), background), (labels(prio, cat(types), 0) if with_types else None)
