"""cerberus_amd.valid_stats without a GPU: the numpy restatement of the reference's accumulator (tests/valid_stats_helpers.py) against what the
REFERENCE's own ProcStepRawOutput accumulated (tests/golden/valid_stats.npz, written by tests/tools/gen_golden_valid_stats.py), and the package's
scalar formulas against the reference's proc_cum_epoch_step_output."""
from collections import OrderedDict

import numpy as np

from valid_stats_helpers import CHANNEL_INFO, HEADS, MAXC, golden_steps, nested, restate


def test_restatement_reproduces_every_golden_counter_of_every_step():
    g, steps = golden_steps()
    assert len(steps) >= 3 and len(set(s[3].shape[0] for s in steps)) == len(steps)  # different batch sizes
    acc = np.zeros((len(HEADS), MAXC, 4), np.int64)
    for name, pred, true, dummy, hw, exp in steps:
        restate(acc, pred, true, dummy, hw)
        assert exp.dtype == np.float64 and np.array_equal(acc.astype(np.float64), exp), (name, np.argwhere(acc != exp)[:5])
    # the figures of the reference's run on valid_step.npz's nopc arrays
    a = steps[0][5]
    assert a[0, 1].tolist() == [4764.0, 29632.0, 6815.0, 27648.0] and a[1, 1, 3] == 18432.0 and not a[5].any()
    # the synthetic steps do flag every head somewhere, Patch-Class included, and count something for every class the callback keeps
    final = steps[-1][5]
    for i, (key, c) in enumerate(HEADS.items()):
        for k in range(0 if key == "Patch-Class" else 1, c):
            assert final[i, k, 3] > 0 and (final[i, k, 1] > 0 or key == "Patch-Class"), (key, k)
    assert final[5, :, 0].sum() > 0 and (final[5, :, 1] > 0).sum() >= 3  # (a handful of samples cannot show all nine patch classes)


def test_head_table_follows_the_channel_info():
    from cerberus_amd.valid_stats import heads_of

    assert heads_of(CHANNEL_INFO) == OrderedDict((k, ({"INST": 0, "TYPE": 1}.get(k.rsplit("-", 1)[1], 2), c)) for k, c in HEADS.items())


def test_scalar_formulas_equal_the_reference_scalars():
    from cerberus_amd.valid_stats import summarize

    g, steps = golden_steps()
    got = summarize(nested(steps[-1][5].astype(np.int64)))
    names = [str(n) for n in g["scalar_names"]]
    assert list(got.keys()) == names  # the same key set, in the reference's order
    for n, v in zip(names, g["scalar_values"]):
        assert isinstance(got[n], np.floating) and got[n] == v, (n, got[n], v)
    assert "Lumen-INST-1-accu" in got and "Lumen-INST-avg-dice" not in got and "Nuclei-TYPE-avg-accu" in got and "Patch-Class-0-dice" in got


def test_stored_noise_counts_respect_the_cap():
    g, _ = golden_steps()
    assert [str(n) for n in g["k_head_names"]] == [k for k in HEADS if k != "Patch-Class"]
    assert float(g["noise"]) == 1e-4 and float(g["k_cap"]) == 1e-3
    for n, k, f in zip(g["k_head_names"], g["k_head"], g["k_head_flagged"]):
        assert f > 0 and 0 <= k <= 1e-3 * f, (str(n), int(k), int(f))
