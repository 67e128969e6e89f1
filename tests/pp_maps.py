"""Engineered inputs for the nuclei / gland / lumen post-processing, and a CPU prediction of the flood tier every mask component takes.

Host only: numpy and the C oracle's stage entries (oracle/postproc_ref.py).  Nothing is imported from cerberus_amd: the tier rule below is a second
statement of the table in DESIGN.md ("post-processing: engineered maps"), not a copy of the library's.

Builder
    place(m, y0, x0, shape, cores, values) writes one cluster into an (H, W, 2) float32 map.  `shape` is the boolean mask wanted AFTER the
    reference's cross erosion: it is grown by the cross, channel 1 is 0.6 there (so inner + contour > 0.5), channel 0 is below 0.5 on the grown
    shape and above 0.5 on the `cores` (the markers).  Dilation followed by erosion is a closing: it fills the inner corners of L / C / comb
    shapes, so areas are read from predict_tiers, never worked out by hand.
Values
    Values("distinct", seed): a seeded permutation of an arithmetic sequence of multiples of 2^-16 -- every float32 inside one cluster differs from
    every other by construction.  Values("tied", seed): the same numbers rounded to 1/16.
Predictor
    predict_tiers(m) -> (components, counts): per kept mask component (tier, need, win, area, n_labels), and components per tier.
"""
import numpy as np

from oracle import postproc_ref as pr

# ---- values ---------------------------------------------------------------------------------------------------------------------------------------------
_Q = 65536.0           # every value is k / 65536 with k < 2^16: exact in float32
_LOW_SPAN = 29000      # k of a non-marker pixel: 1 .. 29000 -> below 0.4425 (rounds to at most 7/16)
_CORE_BASE = 36864     # 0.5625: a marker pixel stays above 0.5 when rounded to 1/16
_CORE_SPAN = 22000     # k of a marker pixel: 36864 .. 58864 -> below 0.8982


class Values(object):
    def __init__(self, kind, seed):
        assert kind in ("distinct", "tied")
        self.kind = kind
        self.rs = np.random.RandomState(seed)

    def draw(self, n, core):
        """n pairwise distinct float32 (rounded to 1/16 for 'tied'): a permutation of base + stride * (0 .. n-1)."""
        span, base = (_CORE_SPAN, _CORE_BASE) if core else (_LOW_SPAN, 1)
        assert 0 < n <= span, n
        k = base + self.rs.permutation(n).astype(np.int64) * (span // n)
        v = (k / _Q).astype(np.float32)
        assert len(np.unique(v)) == n and np.array_equal(v.astype(np.float64) * _Q, k)
        if self.kind == "tied":
            v = (np.round(v * np.float32(16.0)) / np.float32(16.0)).astype(np.float32)
        assert (v > 0.5).all() if core else (v < 0.5).all()
        return v


# ---- shapes (boolean masks) -----------------------------------------------------------------------------------------------------------------------------
def rect(h, w):
    return np.ones((h, w), bool)


def rect_trunc(h, w, j):
    """h x w rectangle whose last row lacks its last j pixels."""
    assert 0 <= j < w
    s = np.ones((h, w), bool)
    if j:
        s[h - 1, w - j:] = False
    return s


def rect_area(w, area):
    """Rows of w pixels, the last one partial: exactly `area` pixels."""
    h = -(-area // w)
    return rect_trunc(h, w, h * w - area)


def ell(h, w, t, j=0):
    """L: a bar of t columns on the left, a bar of t rows at the bottom; the bottom row lacks its last j pixels."""
    s = np.zeros((h, w), bool)
    s[:, :t] = True
    s[h - t:, :] = True
    if j:
        s[h - 1, w - j:] = False
    return s


def cee(h, w, t):
    """C open to the right: left bar, top bar, bottom bar, each t thick."""
    s = np.zeros((h, w), bool)
    s[:, :t] = True
    s[:t, :] = True
    s[h - t:, :] = True
    return s


def serpentine(h, w, t, pitch):
    """Horizontal runs t thick every `pitch` rows, joined at alternating ends."""
    s = np.zeros((h, w), bool)
    rows = list(range(0, h - t + 1, pitch))
    for i, r in enumerate(rows):
        s[r:r + t, :] = True
        if i + 1 < len(rows):
            c = slice(w - t, w) if i % 2 == 0 else slice(0, t)
            s[r:rows[i + 1] + t, c] = True
    return s[:rows[-1] + t]


def comb(h, w, t, pitch):
    """A spine t thick across the middle row with teeth t thick every `pitch` columns, up and down alternately from column 0, both at every other."""
    s = np.zeros((h, w), bool)
    mid = h // 2
    s[mid:mid + t, :] = True
    for i, c in enumerate(range(0, w - t + 1, pitch)):
        if i % 3 != 1:
            s[:mid, c:c + t] = True
        if i % 3 != 0:
            s[mid:, c:c + t] = True
    return s


def ring(h, w, t):
    s = np.ones((h, w), bool)
    s[t:h - t, t:w - t] = False
    return s


def nested_rings(h, w, t, gap):
    """A ring and, `gap` pixels inside it, a second one."""
    s = ring(h, w, t)
    o = t + gap
    s[o:h - o, o:w - o] |= ring(h - 2 * o, w - 2 * o, t)
    return s


def _grow_cross(s):
    g = np.zeros((s.shape[0] + 2, s.shape[1] + 2), bool)
    g[1:-1, 1:-1] = s
    c = g.copy()
    c[1:] |= g[:-1]
    c[:-1] |= g[1:]
    c[:, 1:] |= g[:, :-1]
    c[:, :-1] |= g[:, 1:]
    return c


def place(m, y0, x0, shape, cores, values, clip=False):
    """Write one cluster with its shape's top-left pixel at (y0, x0).  cores: (dy, dx, h, w) rectangles, or (dy, dx, boolean mask), relative to the
    shape, each wholly inside it.  The shape must lie inside the map and so must its grown version, unless `clip` (the erosion never lets the border
    win, so a shape on the map's edge survives it); the grown shape may not come within one pixel (8-neighbourhood) of an earlier cluster.
    Returns the number of cores."""
    shape = np.asarray(shape, bool)
    g = _grow_cross(shape)
    H, W = m.shape[:2]
    assert y0 >= 0 and x0 >= 0 and y0 + shape.shape[0] <= H and x0 + shape.shape[1] <= W, "the shape leaves the map"
    big = np.zeros((H + 2, W + 2), bool)
    big[y0:y0 + g.shape[0], x0:x0 + g.shape[1]] = g
    assert clip or not (big[0].any() or big[-1].any() or big[:, 0].any() or big[:, -1].any()), "the grown shape leaves the map"
    full = big[1:-1, 1:-1]
    v = big.copy()
    v[1:] |= big[:-1]
    v[:-1] |= big[1:]
    near = v.copy()
    near[:, 1:] |= v[:, :-1]
    near[:, :-1] |= v[:, 1:]
    assert not (near[1:-1, 1:-1] & (m[..., 1] != 0)).any(), "clusters touch"
    m[..., 1][full] = np.float32(0.6)
    m[..., 0][full] = values.draw(int(full.sum()), core=False)
    cm = np.zeros(m.shape[:2], bool)
    for c in cores:
        k = np.ones((c[2], c[3]), bool) if len(c) == 4 else np.asarray(c[2], bool)
        assert shape[c[0]:c[0] + k.shape[0], c[1]:c[1] + k.shape[1]][k].all() and c[0] >= 0 and c[1] >= 0, "a core leaves the shape"
        cm[y0 + c[0]:y0 + c[0] + k.shape[0], x0 + c[1]:x0 + c[1] + k.shape[1]] |= k
    if cm.any():
        m[..., 0][cm] = values.draw(int(cm.sum()), core=True)
    return len(cores)


# ---- predictor ------------------------------------------------------------------------------------------------------------------------------------------
TIERS = ("tiny", "small", "big", "lds", "global")


def tier_rule(need, win, area):
    """The flood tier of a component with markers of several labels; first match wins ("post-processing: engineered maps")."""
    if need <= 512 and win <= 1024:
        return "tiny"
    if need <= 1024 and win <= 2304:
        return "small"
    if need <= 2048 and win <= 16384:
        return "big"
    if area <= 1024:
        return "lds"
    return "global"


def front(m):
    """(mask component ids, start map, seeds, floodable) of the nuclei front, restated from the oracle's stage entries."""
    m = np.asarray(m, np.float32)
    raw = (m[..., 0] + m[..., 1]) > np.float32(0.5)
    lab, n = pr.label4(pr.erode_cross3(raw))
    area = np.bincount(lab.ravel(), minlength=n + 1)
    comp = np.where(area[lab] >= 8, lab, 0)
    ml, n = pr.label4(m[..., 0] > np.float32(0.5))
    marea = np.bincount(ml.ravel(), minlength=n + 1)
    markers, _ = pr.label4(pr.fill_holes((ml > 0) & (marea[ml] >= 4)))
    start = np.where(comp > 0, markers, 0)
    fl = (comp > 0) & (start == 0)
    nb = np.zeros_like(fl)
    nb[1:] |= fl[:-1]
    nb[:-1] |= fl[1:]
    nb[:, 1:] |= fl[:, :-1]
    nb[:, :-1] |= fl[:, 1:]
    return comp, start, (start > 0) & nb, fl, int(markers.max())


def predict_tiers(m):
    """-> (comps, counts).  comps: {first pixel (y, x): (tier, need, win, area, n_labels)} for every kept mask component, tier one of TIERS, 'single' (its
    markers carry one label: filled, not flooded) or 'none' (no marker inside, or nothing left to flood).  counts: components per tier."""
    comp, start, seeds, fl, _ = front(m)
    comps = {}
    counts = dict.fromkeys(TIERS + ("single", "none"), 0)
    for c in np.unique(comp)[1:]:
        ys, xs = np.nonzero(comp == c)
        area = len(ys)
        win = int(ys.max() - ys.min() + 3) * int(xs.max() - xs.min() + 3)
        n_labels = len(np.unique(start[ys, xs])) - int((start[ys, xs] == 0).any())
        need = int(seeds[ys, xs].sum()) + int(fl[ys, xs].sum())
        if n_labels == 0 or (n_labels > 1 and not seeds[ys, xs].any()):
            tier = "none"
        elif n_labels == 1:
            tier = "single"
        else:
            tier = tier_rule(need, win, area)
        counts[tier] += 1
        comps[(int(ys[0]), int(xs[0]))] = (tier, need, win, area, n_labels)
    return comps, counts


def distinct_within_components(m):
    """True when no two pixels of one kept mask component hold the same inner value."""
    comp = front(m)[0]
    for c in np.unique(comp)[1:]:
        v = m[..., 0][comp == c]
        if len(np.unique(v)) != len(v):
            return False
    return True


def tied_seed_pairs(m):
    """Number of kept mask components with two seeds of equal inner value."""
    comp, _, seeds, _, _ = front(m)
    n = 0
    for c in np.unique(comp)[1:]:
        v = m[..., 0][(comp == c) & seeds]
        n += int(len(np.unique(v)) != len(v))
    return n




# ---- the fixed nuclei maps --------------------------------------------------------------------------------------------------------------------------------
class _Sheet(object):
    """A map being filled: remembers every cluster's first pixel (raster order) by name, which is also the first pixel of its mask component (a
    closing adds no pixel to a shape's first row)."""

    def __init__(self, h, w, values):
        self.m = np.zeros((h, w, 2), np.float32)
        self.v = values
        self.at = {}

    def put(self, name, y, x, shape, cores, clip=False):
        r = int(np.argmax(shape.any(1)))
        self.at[name] = (y + r, x + int(np.argmax(shape[r])))
        place(self.m, y, x, shape, cores, self.v, clip)


def _two_cores(shape):
    """Two 3 x 3 markers one pixel inside a rectangle whose last row may be partial: 9 labelled pixels each, 8 of them seeds (need = area - 2)."""
    h, w = shape.shape
    return [(1, 1, 3, 3), (h - 5, w - 4, 3, 3)]


def tier_map(kind):
    """One component per flood tier, one single-label component and one without a marker.  -> (map, markers placed, {name: first pixel}); the name of a
    flooded component is the tier it is meant for."""
    s = _Sheet(140, 248, Values(kind, 11))
    s.put("lds", 2, 2, ell(135, 135, 3), [(0, 0, 3, 3), (132, 132, 3, 3)])
    s.put("global", 4, 12, rect(80, 80), [(10, 10, 4, 4), (40, 60, 4, 4), (70, 20, 4, 4)])
    s.put("small", 4, 98, rect(25, 35), [(2, 2, 5, 5), (18, 28, 5, 5)])
    s.put("tiny", 36, 98, rect(16, 24), [(2, 2, 4, 4), (10, 18, 4, 4)])
    s.put("single", 60, 98, rect(12, 12), [(4, 4, 4, 4)])
    s.put("none", 80, 98, rect(10, 10), [])
    s.put("big", 4, 144, rect(60, 100), [(2, 2, 56, 40), (2, 58, 56, 40)])
    return s.m, 2 + 3 + 2 + 2 + 1 + 0 + 2, s.at


# (name, tier at the cap, tier one past it, which figure, value at the cap, value one past it -- for a window the next value the shapes can reach)
CAPS = (
    ("need512", "tiny", "small", "need", 512, 513),
    ("win1024", "tiny", "small", "win", 1024, 1056),
    ("need1024", "small", "big", "need", 1024, 1025),
    ("win2304", "small", "big", "win", 2304, 2352),
    ("need2048", "big", "global", "need", 2048, 2049),
    ("win16384", "big", "global", "win", 16384, 16512),
    ("area1024", "lds", "global", "area", 1024, 1025),
)


def cap_map(kind):
    """For each of the seven caps of the tier rule one component exactly at it (name + '@') and one exactly one past it (name + '+').
    -> (map, markers placed, {name: first pixel})."""
    s = _Sheet(196, 300, Values(kind, 12))
    # area 1024 / 1025 with a window past every cap: two thin Ls, one in the other's corner
    s.put("area1024@", 12, 2, ell(172, 172, 3), [(0, 0, 3, 3), (169, 169, 3, 3)])
    s.put("area1024+", 2, 12, ell(173, 172, 3, 2), [(0, 0, 3, 3), (170, 160, 3, 3)])
    # window 16384 / 16512: two thin Cs, the second mirrored and hooked into the first
    s.put("win16384@", 4, 24, cee(126, 126, 3), [(0, 123, 3, 3), (123, 123, 3, 3)])
    s.put("win16384+", 12, 32, cee(126, 127, 3)[:, ::-1], [(0, 0, 3, 3), (123, 0, 3, 3)])
    x = 194
    s.put("win2304@", 2, x, rect(46, 46), [(1, 1, 44, 20), (1, 25, 44, 20)])
    s.put("win2304+", 52, x, rect(46, 47), [(1, 1, 44, 20), (1, 26, 44, 20)])
    for name, y, area in (("need2048@", 102, 2050), ("need2048+", 149, 2051)):
        sh = rect_area(50, area)
        s.put(name, y, x, sh, _two_cores(sh))
    x = 250
    s.put("win1024@", 2, x, rect(30, 30), [(1, 1, 28, 13), (1, 16, 28, 13)])
    s.put("win1024+", 36, x, rect(30, 31), [(1, 1, 28, 13), (1, 17, 28, 13)])
    for name, y, w, area in (("need1024@", 70, 36, 1026), ("need1024+", 103, 36, 1027), ("need512@", 136, 26, 514), ("need512+", 160, 26, 515)):
        sh = rect_area(w, area)
        s.put(name, y, x, sh, _two_cores(sh))
    return s.m, 28, s.at


def seam_map():
    """A nuclei map of 4 x 4 labelling tiles (64 wide, 32 high; seams at x = 64, 128, 192 and y = 32, 64, 96) whose shapes cross the seams.
    -> (map, markers that survive the marker front, {name: first pixel}, {name: eroded mask wanted, at map size})."""
    s = _Sheet(100, 200, Values("distinct", 13))
    masks = {}

    def put(name, y, x, shape, cores, clip=False):
        s.put(name, y, x, shape, cores, clip)
        masks[name] = np.zeros((100, 200), bool)
        masks[name][y:y + shape.shape[0], x:x + shape.shape[1]] = shape

    # 1-px corridors: ten runs over columns 2 .. 197 (every vertical seam ten times, y = 32 twice), and, transposed, seven runs down rows 42 .. 98
    # (y = 64 and y = 96 seven times); a 1 x 4 marker at either end, so that a corridor cut at a seam changes the flood
    sh = serpentine(37, 196, 1, 4)
    put("serpentine", 2, 2, sh, [(0, 0, 1, 4), (36, 0, 1, 4)])
    sh = serpentine(25, 57, 1, 4).T
    put("serpentine_t", 42, 2, sh, [(0, 0, 4, 1), (0, 24, 4, 1)])
    # comb: spine on rows 64 .. 65, teeth above and below the seam y = 64, across x = 64
    put("comb", 54, 36, comb(21, 80, 2, 6), [(10, 0, 2, 4), (10, 76, 2, 4)])
    # marker rings in one rectangle (rows 44 .. 93, columns 122 .. 193).  A 2 x 2 marker sits in each hole: a hole that is filled swallows it, one
    # that is not leaves an instance too many.
    r1 = ring(9, 12, 2)            # hole: columns 126 .. 133 of the map, over x = 128
    r1[4:6, 5:7] = True
    r2 = ring(12, 9, 2)            # hole: rows 60 .. 67 of the map, over y = 64
    r2[5:7, 4:6] = True
    r3 = nested_rings(15, 15, 2, 2)  # a ring in a ring
    r4 = ring(9, 9, 2)
    r4[4, 3:6] = True              # 3-px speck: removed before the fill
    r5 = ring(9, 10, 2)
    r5[4, 3:7] = True              # 4-px speck: kept, then swallowed by the fill
    put("rings", 44, 122, rect(50, 72), [(2, 2, r1), (14, 20, r2), (30, 2, r3), (2, 30, r4), (2, 50, r5)])
    # a marker U whose inside opens onto the map's last row: not a hole, so the 2 x 2 marker inside stays an instance
    u = ring(8, 9, 2)
    u[6:8, 2:7] = False
    u[4:6, 3:5] = True
    put("border_ring", 88, 40, rect(12, 14), [(4, 2, u)], clip=True)
    return s.m, 2 + 2 + 2 + 5 + 2, s.at, masks


def nuclei_threshold_map():
    """Mask components of 7 and 8 pixels and markers of 3 and 4 pixels, each alone and three pixels from a kept neighbour (the closest two
    clusters can lie without merging).  -> (map, markers that survive the marker front)."""
    s = _Sheet(64, 64, Values("distinct", 14))
    s.put("mask7", 2, 2, rect_area(4, 7), [(0, 0, 2, 2)])            # component dropped: its marker keeps its id, no pixel carries it
    s.put("mask8", 2, 12, rect_area(4, 8), [(0, 0, 2, 2)])
    s.put("kept_a", 10, 2, rect(6, 6), [(1, 1, 2, 2)])
    s.put("mask7_near", 10, 11, rect_area(4, 7), [(0, 0, 2, 2)])
    s.put("kept_b", 10, 24, rect(6, 6), [(1, 1, 2, 2)])
    s.put("mask8_near", 10, 33, rect_area(4, 8), [(0, 0, 2, 2)])
    s.put("marker3", 22, 2, rect(6, 8), [(2, 2, 1, 3)])               # marker dropped: nothing to flood from
    s.put("marker4", 22, 16, rect(6, 8), [(2, 2, 1, 4)])
    s.put("marker3_near", 34, 2, rect(8, 12), [(1, 1, 2, 2), (5, 7, 1, 3)])
    s.put("marker4_near", 46, 2, rect(8, 12), [(1, 1, 2, 2), (5, 7, 1, 4)])  # the last marker in raster order survives: ids run up to the count
    return s.m, 6 + 0 + 1 + 1 + 2


# ---- gland / lumen maps -----------------------------------------------------------------------------------------------------------------------------------
def gl_params(tissue, ds):
    """(threshold, min_size, ksize, pad) as loader/postproc.py works them out."""
    if tissue == "Gland":
        return 0.55, int(1000 * ds ** 2), int(10 * ds), 2 * int(10 * ds)
    return 0.5, int(150 * ds ** 2), int(2 * ds), 2 * int(2 * ds)


_SLIT_RING = {("Gland", 1.0): (50, 7, 7, 13), ("Gland", 0.5): (30, 4, 2, 8), ("Lumen", 1.0): (20, 3, 1, 5), ("Lumen", 0.5): (12, 2, 1, 4)}


def slit_ring(size, t, slit):
    """A square ring with `slit` rows cut out of the middle of its right side."""
    s = ring(size, size, t)
    a = (size - slit) // 2
    s[a:a + slit, size - t:] = False
    return s


def _gl_sheet(items, gap):
    """Rows of shapes, `gap` pixels between them and from the border; shapes given as lists per row.  -> (map with channel 0 = 1 on the shapes,
    {(row, column): (y0, x0)})."""
    hs = [max(sh.shape[0] for sh in row) for row in items]
    ws = [sum(sh.shape[1] for sh in row) + gap * (len(row) + 1) for row in items]
    m = np.zeros((sum(hs) + gap * (len(items) + 1), max(ws), 2), np.float32)
    at = {}
    y = gap
    for i, row in enumerate(items):
        x = gap
        for j, sh in enumerate(row):
            m[y:y + sh.shape[0], x:x + sh.shape[1], 0][sh] = 1.0
            at[(i, j)] = (y, x)
            x += sh.shape[1] + gap
        y += hs[i] + gap
    return m, at


def gl_area_map(tissue, ds):
    """Components of min_size - 1 and min_size pixels, two kept ones two pixels apart (their dilations overlap: the later id wins), and two rings
    with a slit -- one the dilation closes, so that the inside becomes a hole and is filled, one it leaves open.
    -> (map, instances expected, {'closed' / 'open': a pixel in the middle of that ring})."""
    thr, min_size, ksize, pad = gl_params(tissue, ds)
    size, t, s_close, s_open = _SLIT_RING[(tissue, ds)]
    w = max(6, int(np.sqrt(min_size)) + 3)
    a, b = rect_area(w, min_size - 1), rect_area(w, min_size)
    pair = np.zeros((b.shape[0], 2 * w + 2), bool)
    pair[:, :w] = b
    pair[:, w + 2:] = b[::-1, ::-1]
    m, at = _gl_sheet([[a, b], [pair], [slit_ring(size, t, s_close), slit_ring(size, t, s_open)]], 2 * pad + ksize + 3)
    mid = {"closed": (at[(2, 0)][0] + size // 2, at[(2, 0)][1] + size // 2), "open": (at[(2, 1)][0] + size // 2, at[(2, 1)][1] + size // 2)}
    return m, 1 + 2 + 2, mid


def gl_border_map(tissue, ds, d):
    """One slit ring (the closing kind) whose box lies d pixels from all four borders."""
    size, t, s_close, _ = _SLIT_RING[(tissue, ds)]
    m = np.zeros((size + 2 * d, size + 2 * d, 2), np.float32)
    m[d:d + size, d:d + size, 0][slit_ring(size, t, s_close)] = 1.0
    return m


# ---- tiny maps ----------------------------------------------------------------------------------------------------------------------------------------------
TINY_SIZES = [(h, w) for h in range(1, 10) for w in range(1, 10)] + [(1, 64), (64, 1), (2, 128), (3, 4)]


def tiny_map(h, w):
    """Two-channel noise quantised to 1/4 (ties everywhere, holes, specks next to markers), one fixed seed per size."""
    rs = np.random.RandomState(1000 * h + w)
    return (np.round(rs.rand(h, w, 2).astype(np.float32) * np.array([1.2, 0.4], np.float32) * 4) / 4).astype(np.float32)
