"""Device time of ONE gen_targets_batch call on a 16 x 448 x 448 batch with the six heads of models/paramset.yml (about 250 nuclei, 12 glands and
12 lumina per sample; the annotations of tests/tools/gen_golden_targets.py's 448 sample, redrawn per sample).  Stream events around the call
after a warm-up call, median of 20.  The call contains its one host synchronisation (module docstring of cerberus_amd/targets.py), so the
figure is what a training loop would wait for.

    python scripts/time_gen_targets.py [--batch 16] [--reps 20]
"""
import argparse
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))


def main():
    from gen_golden_targets import mirrored

    from cerberus_amd.targets import gen_targets_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    anns = []
    for n in range(a.batch):
        rs = np.random.RandomState(1000 + n)
        nuc = mirrored(rs, 448, 448, 250, 4, 9, 48)
        gla = mirrored(rs, 448, 448, 12, 25, 50, 48)
        lum = np.where(gla > 0, mirrored(rs, 448, 448, 12, 8, 18, 48), 0)
        anns.append(np.stack([lum, gla, nuc, np.where(nuc > 0, rs.randint(1, 7, (448, 448)), 0), np.where(gla > 0, rs.randint(1, 3, (448, 448)), 0),
                              np.full((448, 448), 5)], -1))
    ann = torch.from_numpy(np.stack(anns).astype(np.int32)).cuda()
    channel = ["Lumen-INST", "Gland-INST", "Nuclei-INST", "Nuclei-TYPE", "Gland-TYPE", "Patch-Class"]
    c2t = OrderedDict([("Lumen-INST", "IP-ERODED-CONTOUR-3"), ("Gland-INST", "IP-ERODED-CONTOUR-11"), ("Nuclei-INST", "IP-ERODED-CONTOUR-3"),
                       ("Nuclei-TYPE", "TP"), ("Gland-TYPE", "TP"), ("Patch-Class", "PC")])
    out = gen_targets_batch(ann, channel, c2t, (448, 448))  # warm-up: workspaces, code objects
    torch.cuda.synchronize()
    labels = [int((np.unique(x[..., 2]).size - 1)) for x in anns]
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = gen_targets_batch(ann, channel, c2t, (448, 448))
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    ms = np.array(ms)
    print("gen_targets_batch %d x 448 x 448, 6 heads (nuclei ids per sample %d..%d): median %.3f ms  min %.3f  max %.3f  (n = %d); weight map max %.3f"
          % (a.batch, min(labels), max(labels), float(np.median(ms)), ms.min(), ms.max(), len(ms), float(out["Nuclei-INST#WEIGHT-MAP"].max())))


if __name__ == "__main__":
    main()
