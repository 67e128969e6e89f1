"""Instance morphometry and gland-level relations on the device: what lies between "label maps in HBM" and the numbers a pathologist or a graph model
uses -- the shape of every gland, lumen and nucleus, which nuclei of which class lie in which gland, how much of a gland is lumen, which glands are
neighbours.

    shape = shape_table(labels, table=None)         # int64 [n][8] = {m20, m02, m11, crack, border_px, hull_area2, hull_pts, rows}
    counts, offsets, points = hull_points(labels, table)
    cols = derived(table, shape)                    # {name: float64 [n]}: axes, eccentricity, orientation, circularity, solidity, extent, ...
    parent_of, parent_rows = relate(child_table, parent_labels, n_parent, child_type=None, shift=0)
    idx, d2 = knn(centroids_q4(table), k)
    tables = tissue_features(nuclei, gland, lumen, nuclei_type=None, shift=0, k=4)     # {tissue: {column: [n]}}

The integer definitions are written out in include/cerberus_hip.h (cerb_inst_shape, cerb_inst_hull_rows, cerb_inst_relate, cerb_points_knn) and
computed by csrc/inst_features.hip; `table` is cerb_inst_table's output (cerberus_amd.postproc.inst_table_device).  Every integer is exact.  The
derived columns are float64 torch arithmetic on those integers (formulas in `derived_formulas`); parity with skimage.measure.regionprops is NOT
claimed.  There is no CPU path: tensors stay on the device and a call without a GPU raises CerberusHipError.

Synchronisation: shape_table and hull_points wait once for the sum of the box heights (the size of the extents workspace), hull_points once more for
the number of vertices; both once more for the largest id when no table is given.  relate and knn wait for nothing."""
import math
from collections import OrderedDict

import torch

from . import _lib
from .inst_metrics import _label_map, _need_gpu, _stream

SHAPE = ("m20", "m02", "m11", "crack", "border_px", "hull_area2", "hull_pts", "rows")
PARENT = ("children", "child_area") + tuple("class%d" % c for c in range(8))
DERIVED = ("mu20", "mu02", "mu11", "major_axis", "minor_axis", "eccentricity", "orientation", "perimeter_crack", "circularity", "hull_area", "solidity",
           "extent")
TISSUES = ("nuclei", "gland", "lumen")
KNN_MAX_POINTS = 2 ** 17
KNN_MAX_K = 8


def _table_for(labels, table):
    from .postproc import inst_table_device

    if table is None:
        n = int(labels.max().clamp(min=0).item()) if labels.numel() else 0
        return inst_table_device(labels, None, n)
    if not (torch.is_tensor(table) and table.is_cuda and table.dtype == torch.int64 and table.dim() == 2 and table.shape[1] == 16 and table.is_contiguous()):
        raise ValueError("table: cerb_inst_table's output, a contiguous CUDA int64 [n, 16] tensor")
    return table


def _box_rows(table):
    """(box heights int64 [n] -- 0 for an absent id --, their exclusive scan)"""
    bh = torch.where(table[:, 0] > 0, (table[:, 4] - table[:, 3]).clamp(min=0), torch.zeros_like(table[:, 0]))
    incl = torch.cumsum(bh, 0)
    return bh, (incl - bh).contiguous(), incl


def _shape_and_hull(labels, table, want_points):
    _need_gpu()
    lab = _label_map(labels, "labels")
    table = _table_for(lab, table)
    dev = lab.device
    n = int(table.shape[0])
    h, w = int(lab.shape[0]), int(lab.shape[1])
    shape = torch.zeros((n, 8), dtype=torch.int64, device=dev)
    if n == 0 or h == 0 or w == 0:
        return lab, table, shape, None, None
    L = _lib.lib()
    with torch.cuda.device(dev):
        st = _stream(dev)
        _lib.check(L.cerb_inst_shape(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), shape.data_ptr(), st))
        _, row_offsets, incl = _box_rows(table)
        total = int(incl[-1].item())  # THE wait: the workspace is sized by it
        extents = torch.empty((max(total, 1), 2), dtype=torch.int32, device=dev)
        pts = torch.empty((2 * max(total, 1), 2), dtype=torch.int32, device=dev) if want_points else None
        _lib.check(L.cerb_inst_hull_rows(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), row_offsets.data_ptr(), extents.data_ptr(),
                                         pts.data_ptr() if pts is not None else None, shape.data_ptr(), st))
    return lab, table, shape, row_offsets, pts


def shape_table(labels, table=None):
    """int64 CUDA [n][8], row id-1 = {m20, m02, m11, crack, border_px, hull_area2, hull_pts, rows} (include/cerberus_hip.h).  labels: [H, W] integer map
    (a CUDA int32 tensor is read in place, row-strided views too); table: cerb_inst_table's rows of that map, computed here when not given (n = the
    map's largest id)."""
    return _shape_and_hull(labels, table, False)[2]


def hull_points(labels, table):
    """The strict vertices of every instance's convex hull (of its pixel centres), counter-clockwise on the screen from the top-left vertex.
    -> (counts int32 [n], offsets int64 [n] = exclusive scan of counts, points int32 [sum counts, 2] as (x, y)), all on the device."""
    lab, table, shape, row_offsets, pts = _shape_and_hull(labels, table, True)
    n = int(table.shape[0])
    dev = lab.device
    counts = shape[:, 6].clamp(min=0)
    offsets = torch.cumsum(counts, 0) - counts
    total = int(counts.sum().item()) if n else 0
    if total == 0:
        return counts.to(torch.int32), offsets, torch.zeros((0, 2), dtype=torch.int32, device=dev)
    inst = torch.repeat_interleave(torch.arange(n, device=dev), counts, output_size=total)
    k = torch.arange(total, device=dev) - offsets[inst]
    return counts.to(torch.int32), offsets, pts[2 * row_offsets[inst] + k].contiguous()


def derived_formulas(xp, table, shape):
    """The derived columns, written once for numpy and torch (xp = the module; float64 arrays in, float64 arrays out), in evaluation order:

        A = area (nan where it is 0),  bw = x2 - x1,  bh = y2 - y1
        sx = sum_x - A x1,  sy = sum_y - A y1                         (first moments about the box corner; exact integers below 2^53)
        mu20 = m20 - sx sx / A,  mu02 = m02 - sy sy / A,  mu11 = m11 - sx sy / A      (central second moments)
        a = mu20 / A + 1/12,  b = mu02 / A + 1/12,  c = mu11 / A      (1/12: the second moment of the pixel's own unit square)
        d = sqrt((a - b)(a - b) + 4 c c)
        l1 = (a + b + d) / 2,  l2 = max((a + b - d) / 2, 0)
        major_axis = 4 sqrt(l1),  minor_axis = 4 sqrt(l2)             (the axes of the ellipse with the same second moments)
        eccentricity = sqrt(max(1 - l2 / l1, 0))
        orientation = atan2(2 c, a - b) / 2                           (angle of the major axis from +x towards +y, y down; in (-pi/2, pi/2])
        perimeter_crack = crack
        circularity = 4 pi A / (crack crack)
        hull_area = hull_area2 / 2 + (bw - 1) + (bh - 1) + 1          (the hull of the pixel SQUARES: centre hull (+) unit square, exactly)
        solidity = A / hull_area                                       (exactly 1 for every axis-aligned rectangle)
        extent = A / (bw bh)

    An absent id (A = 0) gives nan."""
    A, sum_x, sum_y = table[:, 0], table[:, 1], table[:, 2]
    y1, y2, x1, x2 = table[:, 3], table[:, 4], table[:, 5], table[:, 6]
    m20, m02, m11, crack, hull_area2 = shape[:, 0], shape[:, 1], shape[:, 2], shape[:, 3], shape[:, 5]
    A = xp.where(A > 0, A, A * float("nan"))
    zero = A * 0.0  # (nan for an absent id: carried into the columns that do not divide by A)
    bw, bh = x2 - x1, y2 - y1
    sx, sy = sum_x - A * x1, sum_y - A * y1
    mu20, mu02, mu11 = m20 - sx * sx / A, m02 - sy * sy / A, m11 - sx * sy / A
    a, b, c = mu20 / A + 1.0 / 12.0, mu02 / A + 1.0 / 12.0, mu11 / A
    d = xp.sqrt((a - b) * (a - b) + 4.0 * c * c)
    l1, l2 = (a + b + d) / 2.0, xp.maximum((a + b - d) / 2.0, zero)
    hull_area = hull_area2 / 2.0 + (bw - 1.0) + (bh - 1.0) + 1.0 + zero
    atan2 = xp.arctan2 if hasattr(xp, "arctan2") else xp.atan2
    return OrderedDict((("mu20", mu20), ("mu02", mu02), ("mu11", mu11), ("major_axis", 4.0 * xp.sqrt(l1)), ("minor_axis", 4.0 * xp.sqrt(l2)),
                        ("eccentricity", xp.sqrt(xp.maximum(1.0 - l2 / l1, zero))), ("orientation", atan2(2.0 * c, a - b) / 2.0),
                        ("perimeter_crack", crack + zero), ("circularity", 4.0 * math.pi * A / (crack * crack)), ("hull_area", hull_area),
                        ("solidity", A / hull_area), ("extent", A / (bw * bh))))


def derived(table, shape):
    """{name: float64 CUDA [n]} for the names in DERIVED, from cerb_inst_table's rows and shape_table's rows of the same map: the formulas of
    derived_formulas in float64 torch arithmetic.  The centroid stays where cerberus_amd.inst_info.info_from_table computes it."""
    _need_gpu()
    return derived_formulas(torch, table.to(torch.float64), shape.to(torch.float64))


def relate(child_table, parent_labels, n_parent, child_type=None, shift=0):
    """Every child instance's parent: the parent map's id under the child's integer centroid (cerb_inst_relate).  child_table: cerb_inst_table's rows of
    the child map; parent_labels: [PH, PW] integer map; shift: 0 when both maps share a grid, 1 for a full-resolution child map over a x0.5 parent map;
    child_type: optional integer classes [n_child] BY ROW (row i = id i + 1).
    -> (parent_of int32 [n_child], parent_rows int64 [n_parent][10] = {children, child area in child-map pixels, children of class 0..7})."""
    _need_gpu()
    if int(shift) < 0 or int(shift) > 30:
        raise ValueError("relate: shift must lie in [0, 30]")
    plab = _label_map(parent_labels, "parent_labels")
    dev = plab.device
    child_table = _table_for(None, child_table.to(dev))
    n_child, n_parent = int(child_table.shape[0]), int(n_parent)
    parent_of = torch.zeros(n_child, dtype=torch.int32, device=dev)
    rows = torch.zeros((max(n_parent, 0), 10), dtype=torch.int64, device=dev)
    ctype = None
    if child_type is not None:
        ctype = torch.as_tensor(child_type).to(dev).to(torch.int32).contiguous()
        if ctype.dim() != 1 or int(ctype.numel()) != n_child:
            raise ValueError("relate: child_type has %s entries for %d children" % (tuple(ctype.shape), n_child))
    ph, pw = int(plab.shape[0]), int(plab.shape[1])
    if n_child == 0 or ph == 0 or pw == 0 or n_parent < 0:
        return parent_of, rows
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().cerb_inst_relate(child_table.data_ptr(), n_child, ctype.data_ptr() if ctype is not None else None, plab.data_ptr(),
                                               plab.stride(0), ph, pw, int(shift), n_parent, parent_of.data_ptr(),
                                               rows.data_ptr() if n_parent else None, _stream(dev)))
    return parent_of, rows


def centroids_q4(table):
    """int64 [n][2]: (floor(16 sum_x / area), floor(16 sum_y / area)), the centroid in sixteenths of a pixel; (0, 0) for an absent id."""
    a = table[:, 0].clamp(min=1)
    return torch.stack([torch.div(16 * table[:, 1], a, rounding_mode="floor"), torch.div(16 * table[:, 2], a, rounding_mode="floor")], 1)


def knn(points_q4, k):
    """The k nearest OTHER points of every point (cerb_points_knn: brute force, exact int64 squared distances, ties to the smaller index).
    points_q4: integer [n][2], |coordinate| < 2^26.  -> (idx int32 [n][k], d2 int64 [n][k]); -1 fills both where n - 1 < k."""
    k = int(k)
    if k < 1 or k > KNN_MAX_K:
        raise ValueError("knn: k must lie in [1, %d], got %d" % (KNN_MAX_K, k))
    n = int(points_q4.shape[0])
    if n > KNN_MAX_POINTS:
        raise ValueError("knn: %d points; the search is brute force and stops at 2^17 = %d points -- a grid-binned search for more is not built"
                         % (n, KNN_MAX_POINTS))
    _need_gpu()
    pts = torch.as_tensor(points_q4)
    if pts.dim() != 2 or pts.shape[1] != 2 or pts.is_floating_point():
        raise ValueError("knn: points are integers [n, 2]")
    if not pts.is_cuda:
        pts = pts.cuda()
    dev = pts.device
    pts = pts.to(torch.int32).contiguous()
    idx = torch.full((n, k), -1, dtype=torch.int32, device=dev)
    d2 = torch.full((n, k), -1, dtype=torch.int64, device=dev)
    if n:
        with torch.cuda.device(dev):
            _lib.check(_lib.lib().cerb_points_knn(pts.data_ptr(), n, k, idx.data_ptr(), d2.data_ptr(), _stream(dev)))
    return idx, d2


def _one_tissue(labels):
    lab, table, shape, _, _ = _shape_and_hull(labels, None, False)
    n = int(table.shape[0])
    cols = OrderedDict()
    cols["id"] = torch.arange(1, n + 1, dtype=torch.int64, device=lab.device)
    cols["area"] = table[:, 0]
    for name, c in (("y1", 3), ("x1", 5), ("y2", 4), ("x2", 6)):
        cols[name] = table[:, c]
    for c, name in enumerate(SHAPE):
        cols[name] = shape[:, c]
    cols.update(derived(table, shape))
    return lab, table, cols


def _types_by_row(nuclei_type, lab, n):
    """nuclei_type -> int32 [n] by row: a [H, W] class map (majority class per instance, the rule of get_inst_info_dict) or a vector indexed by id."""
    if nuclei_type is None:
        return None
    t = torch.as_tensor(nuclei_type) if not torch.is_tensor(nuclei_type) else nuclei_type
    if t.dim() == 2:
        from .inst_metrics import majority_types

        return majority_types(lab.contiguous(), t, max_id=n)[1:].contiguous()
    if t.dim() != 1 or t.is_floating_point() or int(t.numel()) < n + 1:
        raise ValueError("nuclei_type: a [H, W] class map or an integer vector indexed by instance id (at least %d entries)" % (n + 1))
    return t.to(lab.device)[1:n + 1].to(torch.int32).contiguous()


def tissue_features(nuclei, gland, lumen, nuclei_type=None, shift=0, k=4):
    """{'nuclei' | 'gland' | 'lumen': {column: CUDA tensor [n]}}, one row per id 1 .. n of that map (n = its largest id; a tissue given as None is left
    out).  Every tissue: id, area, y1, x1, y2, x2, the eight shape words (SHAPE) and the derived columns (DERIVED).  Nuclei and lumina: gland_id, the
    gland under the instance's integer centroid (0 = none; no gland map: the column is missing).  Glands: n_nuclei, nuclei_area (in nuclei-map
    pixels), n_nuclei_class0..7, n_lumina, lumen_area, lumen_fraction = lumen_area / area, knn_id1..k (ids of the k nearest other glands by
    centroid, -1 = none) and knn_dist1..k (pixels: sqrt(d2 / 256) of the centroids in sixteenths; nan = none).
    nuclei_type: a [H, W] class map of the nuclei map or a class vector indexed by nucleus id; shift: 0 when nuclei and gland maps share a grid, 1
    for full-resolution nuclei over x0.5 gland and lumen maps (lumina and glands always share a grid)."""
    _need_gpu()
    out, tabs, labs = OrderedDict(), {}, {}
    for name, m in zip(TISSUES, (nuclei, gland, lumen)):
        if m is not None:
            labs[name], tabs[name], out[name] = _one_tissue(m)
    if "gland" not in out:
        return out
    g, gt = out["gland"], tabs["gland"]
    n_g = int(gt.shape[0])
    dev = gt.device
    if "nuclei" in out:
        ntab = tabs["nuclei"].to(dev)
        types = _types_by_row(nuclei_type, labs["nuclei"], int(ntab.shape[0]))
        parent_of, rows = relate(ntab, labs["gland"], n_g, types.to(dev) if types is not None else None, shift)
        out["nuclei"]["gland_id"] = parent_of.to(out["nuclei"]["id"].device)
        g["n_nuclei"], g["nuclei_area"] = rows[:, 0], rows[:, 1]
        for c in range(8):
            g["n_nuclei_class%d" % c] = rows[:, 2 + c]
    if "lumen" in out:
        parent_of, rows = relate(tabs["lumen"].to(dev), labs["gland"], n_g, None, 0)
        out["lumen"]["gland_id"] = parent_of.to(out["lumen"]["id"].device)
        g["n_lumina"], g["lumen_area"] = rows[:, 0], rows[:, 1]
        g["lumen_fraction"] = rows[:, 1].to(torch.float64) / gt[:, 0].to(torch.float64)
    k = int(k)
    if k > 0:
        present = torch.nonzero(gt[:, 0] > 0)[:, 0]  # absent ids have no centroid: the search runs over the glands that occur
        idx, d2 = knn(centroids_q4(gt)[present], k)
        ids = torch.full((n_g, k), -1, dtype=torch.int64, device=dev)
        dist = torch.full((n_g, k), float("nan"), dtype=torch.float64, device=dev)
        if int(present.numel()):
            found = idx >= 0
            ids[present] = torch.where(found, present[idx.clamp(min=0).to(torch.int64)] + 1, torch.full_like(idx, -1, dtype=torch.int64))
            dist[present] = torch.where(found, torch.sqrt(d2.to(torch.float64) / 256.0), torch.full_like(d2, float("nan"), dtype=torch.float64))
        for j in range(k):
            g["knn_id%d" % (j + 1)] = ids[:, j]
        for j in range(k):
            g["knn_dist%d" % (j + 1)] = dist[:, j]
    return out


def write_csv(path, cols):
    """One tissue's table as CSV: integers as integers, float64 by repr (round-trips)."""
    import csv

    names = list(cols)
    host = [cols[c].cpu().numpy() for c in names]
    with open(path, "w", newline="") as fh:
        wr = csv.writer(fh)
        wr.writerow(names)
        for i in range(len(host[0]) if host else 0):
            wr.writerow([repr(float(v[i])) if v.dtype.kind == "f" else int(v[i]) for v in host])


def shift_for(child_shape, parent_shape):
    """0 when the two maps share a grid, 1 when the parent map is the x0.5 grid of the child map (ceil or floor of each side); anything else is refused."""
    ch, cw = int(child_shape[0]), int(child_shape[1])
    ph, pw = int(parent_shape[0]), int(parent_shape[1])
    if (ch, cw) == (ph, pw):
        return 0
    if ph in (ch // 2, (ch + 1) // 2) and pw in (cw // 2, (cw + 1) // 2):
        return 1
    raise ValueError("nuclei map %d x %d over gland map %d x %d: the ratio of the two grids must be 1 or 2" % (ch, cw, ph, pw))
