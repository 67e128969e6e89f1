"""Generate tests/golden/remap_label.npz: the REFERENCE's own misc/utils.py::remap_label (lines 133-164) on small label maps -- the inputs and its
outputs in both modes.

    python tests/tools/gen_golden_remap_label.py [--out FILE]     (reference checkout: $CERBERUS_REFERENCE, default <repository>/../reference)

cv2 is oracle/cv2_standin.py and the modules misc/utils.py imports but this path never calls are inert stubs, as in gen_golden_tissue_mask.py.  Only
DATA is written: per case 'c<i>/in' (int32), 'c<i>/plain' and 'c<i>/by_size' (the reference's outputs, int32).

Cases (SEED): rectangles of random size pasted in id order on maps of at most 64 x 64 -- later ones overwrite earlier ones, so instances are cut and
some vanish; ids come from a sparse random set (gaps), one case reaches 70000; two cases paste pairs of equal-sized, non-overlapping squares so that
by_size meets equal areas; one case is a single instance, one has a background-free map.  Nothing is written unless at least two cases have an id gap
and at least two have an equal-area tie among the ids that occur.  The empty map is not a case: the reference returns its input object there."""
import os
import sys
from unittest.mock import MagicMock

import numpy as np

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
REF = os.environ.get("CERBERUS_REFERENCE", os.path.join(os.path.dirname(ROOT), "reference"))
SEED = 20261019


def _import_reference():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, REF)
    from oracle import cv2_standin

    sys.modules["cv2"] = cv2_standin
    # remap_label itself is numpy only: scikit-image, where missing, is stubbed like the rest
    for m in ["pandas", "tqdm", "termcolor", "matplotlib", "matplotlib.pyplot", "skimage", "skimage.filters", "skimage.morphology"]:
        if m not in sys.modules:
            try:
                __import__(m)
            except Exception:
                sys.modules[m] = MagicMock()
    import warnings

    warnings.simplefilter("ignore", DeprecationWarning)
    from misc import utils as ref_utils  # noqa: E402  (reference)

    return ref_utils


def rect_map(rs, h, w, n, max_id, side=(3, 14)):
    lab = np.zeros((h, w), np.int32)
    ids = np.sort(rs.choice(np.arange(1, max_id + 1), size=n, replace=False))
    for i in ids:
        a, b = rs.randint(side[0], side[1], 2)
        y, x = rs.randint(0, h - 1), rs.randint(0, w - 1)
        lab[y:y + a, x:x + b] = i
    return lab


def tie_map(rs, h, w, ids):
    """non-overlapping 5 x 5 and 4 x 4 squares on a grid: many equal areas"""
    lab = np.zeros((h, w), np.int32)
    cells = [(y, x) for y in range(0, h - 7, 8) for x in range(0, w - 7, 8)]
    rs.shuffle(cells)
    for k, i in enumerate(ids):
        y, x = cells[k]
        s = 5 if k % 3 else 4
        lab[y + 1:y + 1 + s, x + 1:x + 1 + s] = i
    return lab


def cases():
    rs = np.random.RandomState(SEED)
    out = [rect_map(rs, 64, 64, 30, 200), rect_map(rs, 37, 61, 18, 70000), tie_map(rs, 64, 48, [3, 9, 10, 40, 41, 77, 300, 301, 302, 1000]),
           tie_map(rs, 48, 64, list(range(5, 45, 3)))]
    one = np.zeros((9, 13), np.int32)
    one[2:6, 3:9] = 17
    out.append(one)
    full = np.repeat(np.array([[4, 2], [9, 2]], np.int32), 6, axis=0).repeat(5, axis=1)  # no background pixel
    out.append(full)
    return out


def main():
    out = os.path.join(ROOT, "tests", "golden", "remap_label.npz")
    if "--out" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1]
    ref = _import_reference()
    data, gaps, ties = {}, 0, 0
    for i, lab in enumerate(cases()):
        ids, area = np.unique(lab[lab > 0], return_counts=True)
        gaps += int(ids.size and ids.max() != ids.size)
        ties += int(np.unique(area).size != area.size)
        plain, by_size = ref.remap_label(lab.copy()), ref.remap_label(lab.copy(), by_size=True)
        assert plain.dtype == np.int32 and by_size.dtype == np.int32
        data["c%d/in" % i], data["c%d/plain" % i], data["c%d/by_size" % i] = lab, plain, by_size
    assert gaps >= 2 and ties >= 2, (gaps, ties)
    np.savez_compressed(out, **data)
    print("%s: %d cases, %d with id gaps, %d with equal-area ties, %d bytes" % (out, len(data) // 3, gaps, ties, os.path.getsize(out)))


if __name__ == "__main__":
    main()
