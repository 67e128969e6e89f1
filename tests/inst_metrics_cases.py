"""The hand-computed 8 x 8 cases of the instance metrics, shared by tests/test_inst_metrics_host.py (the restatement) and
tests/test_inst_metrics_gpu.py (the kernels).  cases() -> [(name, true, pred, expected integer counters, expected sum_iou as a (num, den) list)].

With a, b the areas, c the overlap, u = a + b - c:
  perfect   two instances under other ids.  a = b = c = 8 and 9: tp 2, every sum 17, dice totals 34.
  split     true 24 px; pred 16 + 8.  (1,1): c 16, u 24 -> match, 2/3.  (1,2): c 8, u 24.  AJI takes pred 1 (16/24), pred 2 is unused: 16 / (24 + 8).
  merged    true 16 + 8; pred 24.  (1,4) matches, 2/3; true 2 has only pred 4 too: I = 16 + 8, U = 24 + 24.
  half      true 4 px, pred its first 2: c 2, u 4 -> IoU exactly 0.5, 2c > u is false: NO match.  AJI 2 / 4.
  tie       true 6 px (row 0, columns 0-5).  pred 9 = columns 0-1 of it (b 2, c 2, u 6); pred 5 = columns 2-4 of rows 0 and 1 (b 6, c 3, u 9):
            2/6 == 3/9.  The tie goes to the SMALLER id, 5, although 9 comes first in raster order: I 3, U 9 + 2 (pred 9 unused) = 11.
  no_true / no_pred / nothing: the zero cases."""
import numpy as np

KEYS = ("tp", "fp", "fn", "aji_inter", "aji_union", "dice2_inter", "dice2_total", "dice1_inter", "dice1_total", "n_true", "n_pred")


def _z():
    return np.zeros((8, 8), np.int32)


def cases():
    out = []
    t, p = _z(), _z()
    t[0:2, 0:4], t[4:7, 4:7] = 3, 7
    p[0:2, 0:4], p[4:7, 4:7] = 5, 2
    out.append(("perfect", t, p, (2, 0, 0, 17, 17, 17, 34, 17, 34, 2, 2), [(8, 8), (9, 9)]))
    t, p = _z(), _z()
    t[0:4, 0:6] = 1
    p[0:4, 0:4], p[0:4, 4:6] = 1, 2
    out.append(("split", t, p, (1, 1, 0, 16, 32, 24, 72, 24, 48, 1, 2), [(16, 24)]))
    t, p = _z(), _z()
    t[0:4, 0:4], t[0:4, 4:6] = 1, 2
    p[0:4, 0:6] = 4
    out.append(("merged", t, p, (1, 0, 1, 24, 48, 24, 72, 24, 48, 2, 1), [(16, 24)]))
    t, p = _z(), _z()
    t[0, 0:4] = 1
    p[0, 0:2] = 1
    out.append(("half", t, p, (0, 1, 1, 2, 4, 2, 6, 2, 6, 1, 1), []))
    t, p = _z(), _z()
    t[0, 0:6] = 1
    p[0, 0:2], p[0:2, 2:5] = 9, 5
    out.append(("tie", t, p, (0, 2, 1, 3, 11, 5, 20, 5, 14, 1, 2), []))
    t, p = _z(), _z()
    p[2:4, 2:4] = 2
    out.append(("no_true", t, p, (0, 1, 0, 0, 4, 0, 0, 0, 4, 0, 1), []))
    out.append(("no_pred", p.copy(), t.copy(), (0, 0, 1, 0, 4, 0, 0, 0, 4, 1, 0), []))
    out.append(("nothing", _z(), _z(), (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0), []))
    return out


def expected_ratios(counters, ious):
    """dq, sq, pq, aji, dice2, dice1 by hand from the expected counters (nan where a denominator is 0; dq, sq: 0)."""
    c = dict(zip(KEYS, counters))
    s = sum(n / d for n, d in ious)
    den = c["tp"] + c["fp"] / 2 + c["fn"] / 2
    dq = c["tp"] / den if den else 0.0
    sq = s / c["tp"] if c["tp"] else 0.0
    nan = float("nan")
    return {"dq": dq, "sq": sq, "pq": dq * sq, "aji": c["aji_inter"] / c["aji_union"] if c["aji_union"] else nan,
            "dice2": 2 * c["dice2_inter"] / c["dice2_total"] if c["dice2_total"] else nan,
            "dice1": 2 * c["dice1_inter"] / c["dice1_total"] if c["dice1_total"] else nan}


def blob_labels(h, w, n, seed, max_id, rmin=3.0, rmax=9.0):
    """Random discs with ids drawn from 1 .. max_id (gaps), later discs overwrite earlier ones."""
    rs = np.random.RandomState(seed)
    lab = np.zeros((h, w), np.int32)
    yy, xx = np.mgrid[0:h, 0:w]
    ids = np.sort(rs.choice(np.arange(1, max_id + 1), size=n, replace=False))
    for i in ids:
        r, cy, cx = rs.uniform(rmin, rmax), rs.uniform(0, h), rs.uniform(0, w)
        lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = i
    return lab
