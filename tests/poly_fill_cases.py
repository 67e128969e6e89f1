"""Engineered inputs shared by the polygon-fill tests: label maps whose instances are each ONE 8-connected piece without holes (so the filled set of an
instance's outer contour is the instance: include/cerberus_hip.h, "label maps from contours"), some of them touching."""
import numpy as np


def ellipse_map(h, w, cell, rmin, rmax, seed, jitter=2):
    """int32 [h, w]: one ellipse per cell of a grid, radii rmin .. rmax (more than cell / 2: neighbours touch, the later one on top), ids 1 .. n in
    raster order of the cells.  -> (map, n)"""
    rs = np.random.RandomState(seed)
    lab = np.zeros((h, w), np.int32)
    ys, xs = np.mgrid[0:h, 0:w]
    n = 0
    for cy in range(cell // 2, h - cell // 2 + 1, cell):
        for cx in range(cell // 2, w - cell // 2 + 1, cell):
            ry, rx = (int(v) for v in rs.randint(rmin, rmax + 1, 2))
            oy, ox = (int(v) for v in rs.randint(-jitter, jitter + 1, 2))
            n += 1
            lab[((ys - cy - oy) * rx) ** 2 + ((xs - cx - ox) * ry) ** 2 <= (rx * ry) ** 2] = n
    return lab, n


def is_round_trip_map(lab, n):
    """every id 1 .. n occurs, as one 8-connected piece that binary_fill_holes leaves unchanged"""
    from scipy import ndimage

    for i in range(1, n + 1):
        m = lab == i
        if not m.any() or ndimage.label(m, structure=np.ones((3, 3), int))[1] != 1 or not np.array_equal(ndimage.binary_fill_holes(m), m):
            return False
    return True


def touching_pairs(lab):
    """how many 4-neighbour pixel pairs carry two different non-zero ids"""
    a, b = lab[:, :-1], lab[:, 1:]
    c, d = lab[:-1], lab[1:]
    return int(((a != b) & (a > 0) & (b > 0)).sum() + ((c != d) & (c > 0) & (d > 0)).sum())


def nuclei_map():
    """150 x 170, 42 instances in cells of 24"""
    return ellipse_map(150, 170, 24, 6, 13, seed=4)


def slide_triple():
    """(nuclei 150 x 170, gland 75 x 85, lumen 75 x 85, nuclei class map uint8): a slide's maps, gland and lumen at half the resolution, lumina inside glands"""
    nuclei, _ = nuclei_map()
    gland, _ = ellipse_map(75, 85, 36, 11, 17, seed=8)
    lumen, _ = ellipse_map(75, 85, 36, 3, 6, seed=9, jitter=4)
    rs = np.random.RandomState(10)
    types = np.kron(rs.randint(0, 7, (10, 11)), np.ones((16, 16), np.int64)).astype(np.uint8)[:150, :170]
    return nuclei, gland, lumen, np.ascontiguousarray(types)
