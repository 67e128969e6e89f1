"""cerb_valid_stats_accumulate for class counts other than those of models/paramset.yml: an INST head with one and with three probability channels
(the one-pixel path for any channel count), TYPE and Patch-Class heads with 12 classes (the 16-class instantiations) and a Patch-Class head with 3
(the 3-class one), against the numpy restatement of tests/valid_stats_helpers.py, on a tile the four-pixel path takes and on an odd one."""
from collections import OrderedDict

import numpy as np
import pytest

from valid_stats_helpers import MAXC, dummy_array, restate

pytestmark = pytest.mark.gpu


def _step(heads, n, h, w, seed):
    rs = np.random.RandomState(seed)
    f32 = np.float32
    special = np.array([0.5, np.nextafter(f32(0.5), f32(1)), np.nan, 0.0, 1.0, 0.75], f32)
    pred, true = OrderedDict(), OrderedDict()
    for key, c in heads.items():
        if key.endswith("INST"):
            pred[key] = special[rs.randint(0, 6, (n, h, w, c - 1))]
        elif key.endswith("TYPE"):
            pred[key] = rs.randint(0, c, (n, h, w)).astype(np.uint8 if seed & 1 else np.int64)
        else:
            pred[key] = rs.randint(0, c, (n, h, w)).astype(f32)
        true[key] = rs.randint(0, c + 2, (n, h, w)).astype(np.int32 if seed & 1 else f32)  # two labels above the range
    has = rs.rand(n, len(heads)) < 0.8
    has[0, :] = True
    return pred, true, dummy_array(has, heads)


@pytest.mark.parametrize("patch_classes", [3, 12])
def test_other_class_counts_equal_the_restatement(patch_classes):
    from cerberus_amd.valid_stats import ValidStats

    info = OrderedDict([("A", {"INST": 4}), ("B", {"INST": 2}), ("C", {"INST": 16}), ("A#TYPE", {"TYPE": 12}), ("B#TYPE", {"TYPE": 2}), ("C#TYPE", {"TYPE": 16}),
                        ("Patch-Class", {"OUT": patch_classes})])
    heads = OrderedDict([("A-INST", 4), ("B-INST", 2), ("C-INST", 16), ("A-TYPE", 12), ("B-TYPE", 2), ("C-TYPE", 16), ("Patch-Class", patch_classes)])
    st = ValidStats(info)
    assert OrderedDict((k, v[1]) for k, v in st.heads.items()) == heads
    exp = np.zeros((len(heads), MAXC, 4), np.int64)
    for seed, (n, h, w) in enumerate([(3, 16, 24), (2, 9, 7), (1, 40, 52)]):
        pred, true, dummy = _step(heads, n, h, w, seed)
        restate(exp, pred, true, dummy, (h, w), heads)
        st.update({"pred": pred, "true": true, "dummy": dummy}, hw=(h, w))
        got = st.counters_int()
        assert np.array_equal(got, exp), (seed, np.argwhere(got != exp)[:5])
    for i, (key, c) in enumerate(heads.items()):  # every class the head keeps counted something, and nothing beyond them was written
        k0 = 0 if key == "Patch-Class" else 1
        assert (exp[i, k0:c, 1] > 0).all() and (exp[i, k0:c, 3] > 0).all() and not exp[i, c:].any() and not exp[i, :k0].any(), key
