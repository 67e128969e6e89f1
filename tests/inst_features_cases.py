"""The label maps, relation cases and point sets of the instance-feature tests (tests/test_inst_features_host.py, tests/test_inst_features_gpu.py):
each the smallest shape at which one of the kernels of cerberus_amd/csrc/inst_features.hip can go wrong.  numpy only; no checker lives here."""
import numpy as np

# The derived float64 columns (cerberus_amd.inst_features.derived_formulas): the largest relative deviation of the formulas run in numpy float64 on
# the restatement's integers from their evaluation in fractions.Fraction, over every instance of shape_cases(), measured by
# tests/test_inst_features_host.py (which asserts it): 1.14e-13, in minor_axis of the one-pixel-wide lines (a + b - d cancels there), rounded up --
# and the bar of the device-side torch arithmetic, 16 x that, for differences in operation order.
DERIVED_MEASURED = 1.2e-13
DERIVED_BAR = 16 * DERIVED_MEASURED


def blob_labels(H, W, seed, n_blobs, rmin, rmax, first_id=1):
    """Seeded elliptical blobs painted in id order (a later blob overwrites an earlier one: touching instances, instances cut in pieces, absent ids)."""
    rs = np.random.RandomState(seed)
    lab = np.zeros((H, W), np.int32)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for i in range(n_blobs):
        r = rs.uniform(rmin, rmax)
        cy, cx = rs.uniform(0, H), rs.uniform(0, W)
        ax, th = rs.uniform(0.6, 1.4), rs.uniform(0, np.pi)
        dy, dx = yy - cy, xx - cx
        u = (np.cos(th) * dx + np.sin(th) * dy) * ax
        v = (-np.sin(th) * dx + np.cos(th) * dy) / ax
        lab[u * u + v * v <= r * r] = first_id + i
    return lab


def _disc(radius):
    yy, xx = np.mgrid[-radius:radius + 1, -radius:radius + 1]
    return (yy * yy + xx * xx <= radius * radius)


def shape_cases():
    """[(name, int32 map, n_inst)]"""
    cases = []
    # width not a multiple of 64: waves straddle rows; absent ids (overwritten blobs and n_inst above the largest id), an id above n_inst, a negative id
    m = blob_labels(70, 97, 11, 14, 3.0, 14.0)
    m[3, 5] = 40      # above n_inst: background
    m[4, 5] = -7      # negative: background
    m[69, 96] = 15
    cases.append(("blobs70x97", m, 17))
    cases.append(("one_pixel_map", np.array([[1]], np.int32), 1))
    cases.append(("empty_one_pixel_map", np.array([[0]], np.int32), 2))
    m = np.zeros((1, 130), np.int32)
    m[0, :70] = 1
    m[0, 70:75] = 2
    m[0, 129] = 3
    cases.append(("row1x130", m, 3))
    # one instance filling several whole waves next to single-pixel instances: the whole-wave and the short-run path in one launch
    m = np.zeros((9, 128), np.int32)
    m[1:7, :] = 1
    m[7, ::2] = np.arange(2, 66)
    m[8, 5] = 66
    m[0, 127] = 67
    cases.append(("waves_and_singles", m, 67))
    # two instances sharing an edge; an instance touching all four map borders
    m = np.zeros((12, 20), np.int32)
    m[2:9, 3:10] = 1
    m[2:9, 10:15] = 2
    cases.append(("shared_edge", m, 2))
    m = np.ones((11, 13), np.int32)
    m[4:7, 5:9] = 2
    cases.append(("four_borders", m, 2))
    # hull shapes, one map each so that a mistake names its shape
    m = np.zeros((5, 7), np.int32)
    m[2, 3] = 1
    cases.append(("single_pixel", m, 1))
    m = np.zeros((5, 80), np.int32)
    m[2, 3:75] = 1
    cases.append(("horizontal_line", m, 1))
    m = np.zeros((30, 5), np.int32)
    m[2:27, 3] = 1
    cases.append(("vertical_line", m, 1))
    m = np.zeros((20, 20), np.int32)
    for i in range(15):
        m[2 + i, 3 + i] = 1
        m[2 + i, 18 - i] = 2
    m[0, 0], m[1, 2], m[2, 4] = 3, 3, 3   # a line of slope 1/2: collinear, not 45 degrees
    cases.append(("diagonal_lines", m, 3))
    m = np.zeros((12, 15), np.int32)
    m[3:8, 2:13] = 1
    m[9:12, 0:3] = 2    # a square
    cases.append(("rectangle", m, 2))
    m = np.zeros((14, 12), np.int32)
    m[1:12, 2:5] = 1
    m[9:12, 2:11] = 1
    cases.append(("L", m, 1))
    m = np.zeros((12, 14), np.int32)
    m[1:10, 1:12] = 1
    m[3:8, 4:10] = 0    # a 9 x 11 ring, its hole off centre
    cases.append(("ring", m, 1))
    m = np.zeros((16, 16), np.int32)
    m[1:4, 2:6] = 1
    m[9:13, 8:15] = 1   # two pieces, rows 4..8 empty
    m[6, 0:3] = 2
    cases.append(("two_pieces", m, 2))
    m = np.zeros((23, 25), np.int32)
    m[2:21, 3:22][_disc(9)] = 1
    cases.append(("disc9", m, 1))
    return cases


def fuzz_maps(count=40, seed=2024):
    """[(name, map, n_inst)]: seeded blob maps of 17 .. 96 pixels a side, nuclei-like and gland-like."""
    rs = np.random.RandomState(seed)
    out = []
    for i in range(count):
        H, W = int(rs.randint(17, 97)), int(rs.randint(17, 97))
        if i % 2:
            m = blob_labels(H, W, 1000 + i, int(rs.randint(1, 5)), 10.0, 40.0)
        else:
            m = blob_labels(H, W, 1000 + i, int(rs.randint(3, 30)), 1.5, 7.0)
        out.append(("fuzz%02d_%dx%d" % (i, H, W), m, int(m.max()) + int(rs.randint(0, 3))))
    return out


def relation_cases():
    """[(name, child map, n_child, child_type (by row) or None, parent map, n_parent, shift)]"""
    cases = []
    child = blob_labels(41, 37, 5, 25, 1.5, 4.0)
    n_child = int(child.max()) + 1
    types = (np.arange(n_child) * 5 + 3) % 11          # classes above 7 are folded by & 7
    parent = blob_labels(41, 37, 6, 4, 8.0, 14.0)
    cases.append(("shift0", child, n_child, types, parent, int(parent.max()), 0))
    cases.append(("shift0_no_types", child, n_child, None, parent, int(parent.max()), 0))
    # parent ids out of range: above n_parent and negative
    p2 = parent.copy()
    p2[p2 == 2] = -2
    cases.append(("parent_ids_out_of_range", child, n_child, types, p2, int(parent.max()) - 1, 0))
    # shift 1: odd-sized child map over the ceil(h / 2) parent map
    half = blob_labels(21, 19, 7, 3, 5.0, 8.0)
    child1 = child.copy()
    child1[40, 36] = n_child                            # the last pixel of the odd-sized map: (20, 18) in the parent grid
    cases.append(("shift1_ceil", child1, n_child, types, half, int(half.max()), 1))
    # the floor(h / 2) map: that centroid's shifted pixel lies outside the parent map
    cases.append(("shift1_outside", child1, n_child, types, np.ones((20, 18), np.int32), 1, 1))
    # a C-shaped child: its centroid lies in its own hollow, on the parent map's background
    c = np.zeros((15, 15), np.int32)
    c[2:13, 2:13] = 1
    c[5:10, 5:13] = 0
    p = np.ones((15, 15), np.int32)
    p[5:10, 5:13] = 0
    cases.append(("c_shape", c, 1, np.array([4]), p, 1, 0))
    return cases


def point_cases():
    """[(name, int64 [n][2])]; every case is run for every k in 1 .. 8 (so n = k + 1 and n - 1 < k occur for n = 1 .. 9)."""
    rs = np.random.RandomState(77)
    cases = [("n%d" % n, rs.randint(-500, 500, (n, 2))) for n in (1, 2, 3, 4, 5, 6, 7, 8, 9)]
    cases.append(("n257", rs.randint(-3000, 3000, (257, 2))))       # one point past the staging tile
    cases.append(("n600", rs.randint(-40, 40, (600, 2))))           # crosses it twice; a small range: many equal distances
    dup = rs.randint(-10, 10, (40, 2))
    cases.append(("duplicates", np.concatenate([dup, dup[:25], dup[:10]])))
    gy, gx = np.mgrid[0:12, 0:11]
    cases.append(("lattice", np.stack([gx.ravel() * 16, gy.ravel() * 16], 1)))
    big = 2 ** 26 - 1
    cases.append(("extreme", np.array([[big, big], [-big, -big], [big, -big], [-big, big], [0, 0], [big, big - 1], [-big, 1 - big]])))
    return [(name, np.asarray(p, np.int64)) for name, p in cases]


def tissue_triple(H=128, W=128, seed=3):
    """(nuclei, gland, lumen, nuclei class map, the classes by nucleus id) on one grid: glands with lumina inside them, nuclei everywhere."""
    gland = blob_labels(H, W, seed, 5, 14.0, 30.0)
    lumen = blob_labels(H, W, seed + 1, 9, 3.0, 7.0)
    lumen[gland == 0] = 0
    nuclei = blob_labels(H, W, seed + 2, 60, 2.0, 4.5)
    rs = np.random.RandomState(seed + 3)
    per_id = rs.randint(0, 6, int(nuclei.max()) + 1)
    per_id[0] = 0
    return nuclei, gland, lumen, per_id[nuclei].astype(np.uint8), per_id
