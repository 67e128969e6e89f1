"""Plain-Python restatement of cerberus_amd/inst_features.py's integers (include/cerberus_hip.h: cerb_inst_shape, cerb_inst_hull_rows,
cerb_inst_relate, cerb_points_knn): loops over pixels with Python integers, the hull by a textbook monotone chain over ALL pixel centres of the
instance (not the per-row shortcut of the device code), the relation by integer division, the neighbours by a full sort on (d2, index).  No checker
of its own lives here; tests/test_inst_features_host.py holds it against closed forms and scipy."""
from fractions import Fraction

import numpy as np


def valid(v, n_inst):
    v = int(v)
    return v if 1 <= v <= n_inst else 0


def inst_table(lab, n_inst, type_map=None):
    """cerb_inst_table's rows as Python integers: [n_inst][16]."""
    H, W = lab.shape
    t = [[0, 0, 0, H, 0, W, 0, H * W] + [0] * 8 for _ in range(n_inst)]
    for y in range(H):
        for x in range(W):
            l = valid(lab[y, x], n_inst)
            if not l:
                continue
            r = t[l - 1]
            r[0] += 1
            r[1] += x
            r[2] += y
            r[3], r[4], r[5], r[6] = min(r[3], y), max(r[4], y + 1), min(r[5], x), max(r[6], x + 1)
            r[7] = min(r[7], y * W + x)
            if type_map is not None:
                r[8 + (int(type_map[y, x]) & 7)] += 1
    return t


def _cross(o, a, b):
    return (a[0] - o[0]) * (b[1] - o[1]) - (a[1] - o[1]) * (b[0] - o[0])


def convex_hull(points):
    """Andrew's monotone chain over all points (x, y), strict vertices only.  -> vertices in the order of increasing angle in a y-UP frame."""
    pts = sorted(set(points))
    if len(pts) <= 1:
        return pts
    lower, upper = [], []
    for p in pts:
        while len(lower) >= 2 and _cross(lower[-2], lower[-1], p) <= 0:
            lower.pop()
        lower.append(p)
    for p in reversed(pts):
        while len(upper) >= 2 and _cross(upper[-2], upper[-1], p) <= 0:
            upper.pop()
        upper.append(p)
    return lower[:-1] + upper[:-1]


def hull_of(points):
    """(hull_area2, vertices counter-clockwise ON THE SCREEN (y down) from the top-left vertex: the leftmost point of the top row)."""
    hull = convex_hull(points)
    if len(hull) == 0:
        return 0, []
    # the chain above turns counter-clockwise in a y-up frame = clockwise on the screen: reverse it
    hull = hull[::-1]
    start = min(range(len(hull)), key=lambda i: (hull[i][1], hull[i][0]))
    hull = hull[start:] + hull[:start]
    a2 = 0
    for i in range(len(hull)):
        (xa, ya), (xb, yb) = hull[i], hull[(i + 1) % len(hull)]
        a2 += xa * yb - xb * ya
    return abs(a2), hull


def shape_rows(lab, n_inst, with_hull=True):
    """([n_inst][8] Python integers = {m20, m02, m11, crack, border_px, hull_area2, hull_pts, rows}, [vertex list per instance])"""
    H, W = lab.shape
    tab = inst_table(lab, n_inst)
    rows = [[0] * 8 for _ in range(n_inst)]
    pix = [[] for _ in range(n_inst)]
    for y in range(H):
        for x in range(W):
            l = valid(lab[y, x], n_inst)
            if not l:
                continue
            r, t = rows[l - 1], tab[l - 1]
            dx, dy = x - t[5], y - t[3]
            r[0] += dx * dx
            r[1] += dy * dy
            r[2] += dx * dy
            sides = 0
            for yy, xx in ((y - 1, x), (y + 1, x), (y, x - 1), (y, x + 1)):
                if yy < 0 or yy >= H or xx < 0 or xx >= W or valid(lab[yy, xx], n_inst) != l:
                    sides += 1
            r[3] += sides
            r[4] += 1 if sides else 0
            pix[l - 1].append((x, y))
    hulls = []
    for i in range(n_inst):
        if with_hull and pix[i]:
            a2, hull = hull_of(pix[i])
            rows[i][5], rows[i][6], rows[i][7] = a2, len(hull), len(set(p[1] for p in pix[i]))
            hulls.append(hull)
        else:
            hulls.append([])
    return rows, hulls


def relate(child_tab, child_type, parent_lab, shift, n_parent):
    """(parent_of [n_child], parent_rows [n_parent][10]) with integer division."""
    PH, PW = parent_lab.shape
    parent_of = []
    rows = [[0] * 10 for _ in range(n_parent)]
    for i, t in enumerate(child_tab):
        p = 0
        if t[0] > 0:
            cx, cy = (t[1] // t[0]) >> shift, (t[2] // t[0]) >> shift
            if 0 <= cx < PW and 0 <= cy < PH:
                p = valid(parent_lab[cy, cx], n_parent)
        parent_of.append(p)
        if p:
            rows[p - 1][0] += 1
            rows[p - 1][1] += t[0]
            if child_type is not None:
                rows[p - 1][2 + (int(child_type[i]) & 7)] += 1
    return parent_of, rows


def knn(xy, k):
    """(idx [n][k], d2 [n][k]): full sort on (d2, index) over the other points, -1 where there are fewer than k."""
    pts = [(int(p[0]), int(p[1])) for p in xy]
    idx, d2 = [], []
    for i, (xi, yi) in enumerate(pts):
        cand = sorted(((xj - xi) ** 2 + (yj - yi) ** 2, j) for j, (xj, yj) in enumerate(pts) if j != i)[:k]
        idx.append([c[1] for c in cand] + [-1] * (k - len(cand)))
        d2.append([c[0] for c in cand] + [-1] * (k - len(cand)))
    return idx, d2


def centroids_q4(tab):
    return [((16 * t[1]) // t[0], (16 * t[2]) // t[0]) if t[0] > 0 else (0, 0) for t in tab]


def _isqrt_frac(q, digits=40):
    """sqrt of a non-negative Fraction to `digits` decimal digits, as a Fraction (integer square root of the scaled value)."""
    import math

    s = 10 ** digits
    return Fraction(math.isqrt(q.numerator * s * s // q.denominator), s)


def derived_exact(t, s):
    """The derived columns of one instance (table row t, shape row s, Python integers) in fractions.Fraction; square roots to 40 digits; the one
    transcendental (atan2) is taken in float64 of the exactly computed, once-rounded arguments.  -> {name: float}; A = 0 is not accepted."""
    import math

    A = Fraction(t[0])
    bw, bh = t[6] - t[5], t[4] - t[3]
    sx, sy = t[1] - t[0] * t[5], t[2] - t[0] * t[3]
    mu20, mu02, mu11 = s[0] - Fraction(sx * sx) / A, s[1] - Fraction(sy * sy) / A, s[2] - Fraction(sx * sy) / A
    a, b, c = mu20 / A + Fraction(1, 12), mu02 / A + Fraction(1, 12), mu11 / A
    d = _isqrt_frac((a - b) ** 2 + 4 * c * c)
    l1, l2 = (a + b + d) / 2, max((a + b - d) / 2, Fraction(0))
    hull_area = Fraction(s[5], 2) + (bw - 1) + (bh - 1) + 1
    pi = Fraction("3.14159265358979323846264338327950288419716939937510")
    return {"mu20": float(mu20), "mu02": float(mu02), "mu11": float(mu11), "major_axis": float(4 * _isqrt_frac(l1)), "minor_axis": float(4 * _isqrt_frac(l2)),
            "eccentricity": float(_isqrt_frac(max(1 - l2 / l1, Fraction(0)))), "orientation": math.atan2(float(2 * c), float(a - b)) / 2,
            "perimeter_crack": float(s[3]), "circularity": float(4 * pi * A / (s[3] * s[3])), "hull_area": float(hull_area),
            "solidity": float(A / hull_area), "extent": float(A / (bw * bh)),
            "_gap": float((l1 - l2) / l1)}  # (relative gap of the two eigenvalues: eccentricity and orientation are ill-conditioned where it vanishes)


def tables(lab, n_inst):
    """(cerb_inst_table rows, shape rows) as int64 numpy arrays."""
    tab = inst_table(lab, n_inst)
    rows, _ = shape_rows(lab, n_inst)
    return np.array(tab, np.int64).reshape(n_inst, 16), np.array(rows, np.int64).reshape(n_inst, 8)
