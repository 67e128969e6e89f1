"""Independent restatement of the instance metrics (PQ, AJI, Dice2, Dice1, remap_label) in numpy and Python integers, written from the
definitions: a dict of combined keys and plain loops.  The checker of tests/test_inst_metrics_*.py; nothing of the package is imported here.

    stats(true, pred, type_true=None, type_pred=None, cls=None) -> dict of Python ints + 'sum_iou' (math.fsum) + the ratios
    pairs(true, pred) -> (area_true {id: a}, area_pred {id: b}, {(t, p): c})
    remap_label(lab, by_size=False)

type_true / type_pred: anything indexable by instance id.  Ratios with a zero denominator are nan, except dq and sq (0)."""
import math

import numpy as np


def pairs(true, pred):
    t = np.asarray(true).astype(np.int64).ravel()
    p = np.asarray(pred).astype(np.int64).ravel()
    assert t.shape == p.shape
    a, b, c = {}, {}, {}
    for ids, out in ((t, a), (p, b)):
        u, n = np.unique(ids[ids > 0], return_counts=True)
        for i, k in zip(u.tolist(), n.tolist()):
            out[i] = k
    both = (t > 0) & (p > 0)
    key = (t[both] << 32) | p[both]
    u, n = np.unique(key, return_counts=True)
    for k, m in zip(u.tolist(), n.tolist()):
        c[(k >> 32, k & 0xFFFFFFFF)] = m
    return a, b, c


def _ratio(num, den):
    return float("nan") if den == 0 else num / den


def stats(true, pred, type_true=None, type_pred=None, cls=None):
    a, b, c = pairs(true, pred)
    if cls is not None:
        a = {t: v for t, v in a.items() if int(type_true[t]) == cls}
        b = {p: v for p, v in b.items() if int(type_pred[p]) == cls}
        c = {(t, p): v for (t, p), v in c.items() if t in a and p in b}
    tp, ious = 0, []
    by_t = {}
    for (t, p), n in sorted(c.items()):
        u = a[t] + b[p] - n
        if 2 * n > u:
            tp += 1
            ious.append(n / u)  # int / int: the correctly rounded quotient
        by_t.setdefault(t, []).append((p, n, u))
    inter = union = 0
    used = set()
    for t in sorted(a):
        if t not in by_t:
            union += a[t]
            continue
        bp, bn, bu = by_t[t][0]
        for p, n, u in by_t[t][1:]:  # ascending p: strictly larger only, so a tie keeps the smaller id
            if n * bu > bn * u:
                bp, bn, bu = p, n, u
        inter += bn
        union += bu
        used.add(bp)
    for p in b:
        if p not in used:
            union += b[p]
    out = {
        "tp": tp, "fp": len(b) - tp, "fn": len(a) - tp, "aji_inter": inter, "aji_union": union,
        "dice2_inter": sum(c.values()), "dice2_total": sum(a[t] + b[p] for t, p in c),
        "dice1_inter": sum(c.values()), "dice1_total": sum(a.values()) + sum(b.values()),
        "n_true": len(a), "n_pred": len(b), "sum_iou": math.fsum(ious),
    }
    out.update(ratios(out))
    return out


def ratios(s):
    den = s["tp"] + s["fp"] / 2 + s["fn"] / 2
    dq = s["tp"] / den if den else 0.0
    sq = s["sum_iou"] / s["tp"] if s["tp"] else 0.0
    return {"dq": dq, "sq": sq, "pq": dq * sq, "aji": _ratio(s["aji_inter"], s["aji_union"]),
            "dice2": _ratio(2 * s["dice2_inter"], s["dice2_total"]), "dice1": _ratio(2 * s["dice1_inter"], s["dice1_total"])}


def remap_label(lab, by_size=False):
    lab = np.asarray(lab)
    ids = [int(i) for i in np.unique(lab) if i != 0]
    out = np.zeros(lab.shape, np.int32)
    if by_size:
        area = {i: int((lab == i).sum()) for i in ids}
        ids = sorted(ids, key=lambda i: -area[i])  # stable: equal areas keep ascending id
    for new, old in enumerate(ids):
        out[lab == old] = new + 1
    return out
