"""One validation step on a 16 x 448 x 448 batch with the six heads of models/paramset.yml, three ways:

  parent route   cerberus_amd.train.valid_step (every head map to the host) + the numpy restatement of the reference's accumulator
                 (tests/valid_stats_helpers.py::restate) -- what a validation loop had to do before cerberus_amd.valid_stats; host clock.
  device route   cerberus_amd.valid_stats.valid_step_stats; host clock around the call and a device synchronise.
  forward alone  the eval-mode infer_tiles of the same batch already on the device; stream events.
  launch alone   cerb_valid_stats_accumulate on maps already on the device (ValidStats.prepare once, --launches PreparedStep.launch() calls back to back between two
                 stream events), in the formats of the device route (uint8 type maps, float32 targets, Patch-Class target one value per sample)
                 and with gen_targets' int32 maps.  Bytes = what the kernel has to read once, from the shapes; rate against the HBM peak.

    python scripts/time_valid_stats.py [--batch 16] [--size 448] [--reps 10] [--host-reps 3] [--launches 200]
"""
import argparse
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12      # bytes/s, specification
HBM_MEASURED = 6.29e12  # bytes/s, a float4 copy


def main():
    from valid_stats_helpers import HEADS, MAXC, restate

    from cerberus_amd.net_desc import create_model
    from cerberus_amd.train import valid_step
    from cerberus_amd.valid_stats import ValidStats, valid_step_stats
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    a = ap.parse_args()
    n, s = a.batch, a.size
    rs = np.random.RandomState(7)
    model = create_model(**default_model_kwargs())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(0).items()}, strict=True)
    run_info = ({"net": {"desc": model}}, None)
    batch = {"img": torch.from_numpy(rs.randint(0, 256, (n, s, s, 3)).astype(np.uint8))}
    for key, c in HEADS.items():
        t = rs.randint(0, c, (n, 1, 1, 1)) if key == "Patch-Class" else (rs.rand(n, s, s, 1) < 0.4) * rs.randint(1, c, (n, s, s, 1))
        batch[key] = torch.from_numpy(t.astype(np.float32))
    has = np.empty((n, len(HEADS)), dtype=object)
    has[:] = [list(HEADS)]
    has_all = has.copy()   # the launch-alone runs count all six heads
    has[:, -1] = None      # the routes run the case the reference defines: no Patch-Class target in the batch (with one, valid_step hands back [N, H, H, W] arrays)
    batch["dummy_target"] = has
    natural = {k: batch[k].numpy() for k in HEADS}

    def clock(fn, reps):
        fn()  # warm-up: code objects, workspaces, the allocator's blocks
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return np.array(ts)

    parent_parts = []

    def parent():
        t0 = time.perf_counter()
        raw = valid_step(dict(batch), run_info)["raw"]
        t1 = time.perf_counter()
        acc = restate(np.zeros((len(HEADS), MAXC, 4), np.int64), raw["pred"], natural, raw["dummy"], (s, s))
        parent_parts.append(((t1 - t0) * 1e3, (time.perf_counter() - t1) * 1e3))
        return acc

    stats = ValidStats(OrderedDict((name, {hname: och}) for name, hname, och, _ in model._decoders))
    t_parent = clock(parent, a.host_reps)
    t_device = clock(lambda: valid_step_stats(dict(batch), run_info, stats), a.reps)
    stats.reset()
    valid_step_stats(dict(batch), run_info, stats)
    same = bool(np.array_equal(stats.counters_int(), parent()))
    parts = np.array(parent_parts[1:1 + a.host_reps])

    tiles = batch["img"].cuda()
    ev = []
    model.infer_tiles(tiles, [s, s], type_dtype=torch.uint8)
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pred = model.infer_tiles(tiles, [s, s], type_dtype=torch.uint8)
        e1.record()
        e1.synchronize()
        ev.append(e0.elapsed_time(e1))
    t_fwd = np.array(ev)

    print("validation step, %d x %d x %d, six heads" % (n, s, s))
    print("  parent route  valid_step + host accumulator : median %8.2f ms  (valid_step %.2f + accumulator %.2f; n = %d)"
          % (float(np.median(t_parent)), float(np.median(parts[:, 0])), float(np.median(parts[:, 1])), len(t_parent)))
    print("  device route  valid_step_stats              : median %8.2f ms  min %.2f  max %.2f  (n = %d); counters equal the parent route's: %s"
          % (float(np.median(t_device)), t_device.min(), t_device.max(), len(t_device), same))
    print("  eval forward alone (infer_tiles, events)    : median %8.2f ms  min %.2f  max %.2f" % (float(np.median(t_fwd)), t_fwd.min(), t_fwd.max()))

    pix = n * s * s
    forms = OrderedDict()
    forms["device route's maps (uint8 type, float32 true)"] = (pred, {k: batch[k].cuda() for k in HEADS}, pix * (3 * 12 + 2 * 5 + 4) + n * 4)
    forms["gen_targets' maps (uint8 type, int32 true)"] = (pred, {k: (batch[k].expand(n, s, s, 1) if k == "Patch-Class" else batch[k]).to(torch.int32).cuda().contiguous()
                                                                  for k in HEADS}, pix * (3 * 12 + 2 * 5 + 8))
    pred64 = model.infer_tiles(tiles, [s, s])
    forms["valid_step's maps (int64 type, float32 true)"] = (pred64, {k: (batch[k].expand(n, s, s, 1) if k == "Patch-Class" else batch[k]).cuda().contiguous() for k in HEADS},
                                                           pix * (3 * 12 + 2 * 12 + 8))
    for what, (p, t, nbytes) in forms.items():
        # two copies of every map, launched in turn: 2 x the bytes of a step do not fit the 256 MB Infinity Cache, so each launch reads HBM
        step_a = stats.prepare(p, t, has_all, (s, s))
        step_b = stats.prepare({k: v.clone() for k, v in p.items()}, {k: v.clone() for k, v in t.items()}, has_all, (s, s))
        step_a.launch()
        step_b.launch()
        torch.cuda.synchronize()
        best = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(a.launches):
                (step_b if i & 1 else step_a).launch()
            e1.record()
            e1.synchronize()
            best.append(e0.elapsed_time(e1) / a.launches * 1e3)
        us = float(np.median(best))
        print("  statistics launch alone, %-48s: %7.1f us per launch (median of 5 x %d), %6.1f MB read -> %.2f TB/s = %.0f %% of the %.1f TB/s peak (%.0f %% of a measured copy)"
              % (what, us, a.launches, nbytes / 1e6, nbytes / us / 1e6, 100 * nbytes / (us * 1e-6) / HBM_PEAK, HBM_PEAK / 1e12, 100 * nbytes / (us * 1e-6) / HBM_MEASURED))


if __name__ == "__main__":
    main()
