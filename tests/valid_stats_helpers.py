"""Shared by tests/test_valid_stats_host.py, tests/test_valid_stats_gpu.py and scripts/time_valid_stats.py: the fixture's steps and a numpy
restatement of the reference's accumulator (models/run_desc.py:606-688) on natural [N, H, W] maps with integer counters."""
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CHANNEL_INFO = OrderedDict([("Lumen", {"INST": 3}), ("Gland", {"INST": 3}), ("Nuclei", {"INST": 3}), ("Nuclei#TYPE", {"TYPE": 7}), ("Gland#TYPE", {"TYPE": 3}),
                            ("Patch-Class", {"OUT": 9})])
HEADS = OrderedDict([("Lumen-INST", 3), ("Gland-INST", 3), ("Nuclei-INST", 3), ("Nuclei-TYPE", 7), ("Gland-TYPE", 3), ("Patch-Class", 9)])
MAXC = 16


def restate(acc, pred, true, dummy, hw, heads=HEADS):
    """acc int64 [heads][16][4] += the step's over_inter, over_total, over_correct, nr_pixels.  pred / true: natural shapes (any array with
    N * H * W [* (C-1)] elements; Patch-Class may hold one value per sample); labels compared as float32."""
    dummy = np.asarray(dummy)
    n, (h, w) = dummy.shape[0], hw
    with np.errstate(invalid="ignore"):
        for i, (key, c) in enumerate(heads.items()):
            flag = np.any(dummy == key, axis=-1)
            spread = lambda a: np.broadcast_to(np.asarray(a).reshape(n, 1, 1), (n, h, w)) if np.asarray(a).size == n and h * w != 1 else np.asarray(a).reshape(n, h, w)
            t = spread(true[key]).astype(np.float32)
            inst, masked = key.endswith("INST"), key.endswith("TYPE")
            p = np.asarray(pred[key], np.float32).reshape(n, h, w, c - 1) if inst else spread(pred[key]).astype(np.float32)
            m = (t > 0) if masked else np.ones(t.shape, bool)
            for k in range(1 if (inst or masked) else 0, c):
                pk = (p[..., k - 1] > 0.5) if inst else (p == k)
                pr = pk * np.float32(k) if inst else p
                tk = t == k
                per_sample = [(m & pk & tk).sum((1, 2)), (m & pk).sum((1, 2)) + (m & tk).sum((1, 2)), (t == pr).sum((1, 2)), np.full(n, h * w)]
                acc[i, k] += [int(v[flag].sum()) for v in per_sample]
    return acc


def dummy_array(has, heads=HEADS):
    d = np.full(np.asarray(has).shape, None, dtype=object)
    for j, key in enumerate(heads):
        d[np.asarray(has)[:, j], j] = key
    return d


def golden_steps():
    """[(name, pred, true, dummy, (h, w), counters after the step)] of tests/golden/valid_stats.npz; step a reads valid_step.npz's nopc arrays."""
    g = np.load(os.path.join(GOLDEN, "valid_stats.npz"))
    gs = np.load(os.path.join(GOLDEN, "valid_step.npz"))
    assert [str(h) for h in g["heads"]] == list(HEADS) and [int(c) for c in g["classes"]] == list(HEADS.values())
    steps = []
    for name in [str(s) for s in g["steps"]]:
        if name == "a":
            pred = OrderedDict((k, gs["nopc/pred/" + k]) for k in HEADS)
            true = OrderedDict((k, gs["nopc/true/" + k]) for k in HEADS)
            hw = tuple(int(v) for v in gs["nopc/img"].shape[1:3])
        else:
            pred = OrderedDict((k, g["%s/pred/%s" % (name, k)]) for k in HEADS)
            true = OrderedDict((k, g["%s/true/%s" % (name, k)]) for k in HEADS)
            hw = tuple(int(v) for v in g[name + "/hw"])
        steps.append((name, pred, true, dummy_array(g[name + "/has_target"]), hw, g[name + "/counters"]))
    return g, steps


def nested(acc, heads=HEADS):
    """int64 [heads][16][4] -> the reference's nested dict of float64."""
    out = OrderedDict()
    for i, (key, c) in enumerate(heads.items()):
        out[key] = OrderedDict((k, OrderedDict(zip(("over_inter", "over_total", "over_correct", "nr_pixels"), (np.float64(v) for v in acc[i, k]))))
                               for k in range(0 if key == "Patch-Class" else 1, c))
    return out


def edge_step(n=1, h=12, w=20, seed=3):
    """One step of N = 1 that holds every edge at once: probabilities exactly 0.5, its two float32 neighbours and NaN, labels above the class range and
    NaN labels, an all-dummy head (Gland-INST)."""
    rs = np.random.RandomState(seed)
    f32 = np.float32
    special = np.array([0.5, np.nextafter(f32(0.5), f32(0)), np.nextafter(f32(0.5), f32(1)), np.nan, 0.0, 1.0, 0.25, 0.75], f32)
    pred, true = OrderedDict(), OrderedDict()
    for key, c in HEADS.items():
        if key.endswith("INST"):
            pred[key] = special[rs.randint(0, 8, (n, h, w, c - 1))]
            t = rs.randint(0, c + 2, (n, h, w)).astype(f32)
        elif key.endswith("TYPE"):
            pred[key] = rs.randint(0, c, (n, h, w)).astype(np.int64)
            t = rs.randint(0, c + 2, (n, h, w)).astype(f32)
        else:
            pred[key] = rs.randint(0, c, (n, h, w)).astype(f32)  # a map that varies inside the tile: the general form
            t = rs.randint(0, c + 2, (n, h, w)).astype(f32)
        t[rs.rand(n, h, w) < 0.03] = np.nan
        true[key] = t
    has = np.ones((n, len(HEADS)), bool)
    has[:, list(HEADS).index("Gland-INST")] = False
    return pred, true, dummy_array(has), (h, w)
