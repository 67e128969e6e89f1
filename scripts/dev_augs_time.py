"""Times the training augmentations (cerberus_amd/augs.py, csrc/augs.hip) at the training geometry: N = 16 tiles, source 540 x 540, output 448 x 448,
annotation of C = 5 channels (BASELINE.json configs[4] with the margin the affine warp needs).

  per kernel        device ms (stream events, median of --reps after a warm-up), every sample taking that operation at its heaviest setting
                    (5 x 5 blurs, per-channel noise); algorithmic bytes from the shapes (each pixel read once and written once; the warp reads one
                    source pixel per output pixel) and the GB/s they give
  augment_batch     device ms of the whole pass with a draw of the default policy (each sample takes ONE of blur / median / noise)
  train_batch       host clock, synchronised: sample_params + augment_batch + gen_targets_batch (which waits for the device once, for its weight maps)
  train_step        host clock, synchronised, in the same run: the step that consumes the batch, as it stands

    python scripts/dev_augs_time.py [--reps 30] [--out profiles/augs.json]
"""
import argparse
import json
import os
import sys
import time
from collections import OrderedDict

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, SRC, OUT, C_ANN = 16, 540, 448, 5
CHANNEL = ["Lumen-INST", "Gland-INST", "Nuclei-INST", "Nuclei-TYPE", "Gland-TYPE"]
C2T = OrderedDict([("Lumen-INST", "IP-ERODED-CONTOUR-3"), ("Gland-INST", "IP-ERODED-CONTOUR-11"), ("Nuclei-INST", "IP-ERODED-CONTOUR-3"),
                   ("Nuclei-TYPE", "TP"), ("Gland-TYPE", "TP")])


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def clock(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def annotated_batch(seed):
    """tiles with a few lumina, glands and a few hundred nuclei each, a class per instance in the type channels"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:SRC, :SRC]
    ann = np.zeros((N, SRC, SRC, C_ANN), np.int32)
    for i in range(N):
        for ch, count, rad, tch in ((0, 4, 30, None), (1, 6, 55, 4), (2, 300, 7, 3)):
            for k in range(count):
                cy, cx = rng.randint(0, SRC, 2)
                r = rad * rng.uniform(0.7, 1.3)
                y0, y1, x0, x1 = max(cy - int(r) - 1, 0), min(cy + int(r) + 2, SRC), max(cx - int(r) - 1, 0), min(cx + int(r) + 2, SRC)
                disc = (yy[y0:y1, x0:x1] - cy) ** 2 + (xx[y0:y1, x0:x1] - cx) ** 2 <= r * r
                ann[i, y0:y1, x0:x1, ch][disc] = k + 1
                if tch is not None:
                    ann[i, y0:y1, x0:x1, tch][disc] = 1 + k % 2
    img = rng.randint(0, 256, (N, SRC, SRC, 3)).astype(np.uint8)
    return torch.from_numpy(img).cuda(), torch.from_numpy(ann).cuda()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "augs.json"))
    a = ap.parse_args()
    from cerberus_amd import augs
    from cerberus_amd.losses import PARAMSET_LOSS
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.targets import gen_targets_batch
    from cerberus_amd.train import Adam, train_step
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    img, ann = annotated_batch(1)
    rng = np.random.RandomState(2)
    p = augs.sample_params(N, (SRC, SRC), (OUT, OUT), rng)
    warped, _ = augs.warp_crop(img, ann, p["map"], (OUT, OUT))
    px = N * OUT * OUT
    key = np.arange(1, N + 1, dtype=np.uint64)
    rows = [
        ("warp", lambda: augs.warp_crop(img, ann, p["map"], (OUT, OUT)), 2 * (3 + 4 * C_ANN) * px),
        ("gaussian_blur 5x5", lambda: augs.gaussian_blur(warped, 5, 5), 6 * px),
        ("gaussian_blur 3x3", lambda: augs.gaussian_blur(warped, 3, 3), 6 * px),
        ("median_blur 5", lambda: augs.median_blur(warped, 5), 6 * px),
        ("median_blur 3", lambda: augs.median_blur(warped, 3), 6 * px),
        ("gaussian_noise per-channel", lambda: augs.gaussian_noise(warped, 8.0, 1, key), 6 * px),
        ("gaussian_noise shared", lambda: augs.gaussian_noise(warped, 8.0, 0, key), 6 * px),
        ("hue", lambda: augs.add_to_hue(warped, 4.0), 6 * px),
        ("saturation", lambda: augs.add_to_saturation(warped, 0.1), 6 * px),
        ("brightness", lambda: augs.add_to_brightness(warped, 10.0), 6 * px),
        ("channel_sums", lambda: augs.channel_sums(warped), 3 * px),
        ("contrast (with its channel_sums)", lambda: augs.add_to_contrast(warped, 1.1, apply_contrast=True), 9 * px),
    ]
    out = {"device": torch.cuda.get_device_name(0), "n": N, "src": SRC, "out": OUT, "ann_channels": C_ANN, "reps": a.reps,
           "note": "per-kernel rows include the single-operation wrapper's parameter upload and output allocation on the stream", "kernels": []}
    for name, fn, nbytes in rows:
        ms = events(fn, a.reps)
        row = {"kernel": name, "device_ms": round(ms, 4), "algorithmic_mb": round(nbytes / 1e6, 2), "gb_s": round(nbytes / ms / 1e6, 1)}
        out["kernels"].append(row)
        print(json.dumps(row), flush=True)
    for contrast in (False, True):
        ms = events(lambda: augs.augment_batch(img, ann, p, (OUT, OUT), apply_contrast=contrast), a.reps)
        out["augment_batch_ms" + ("_apply_contrast" if contrast else "")] = round(ms, 4)
    # one pass each over warp, one of blur / median / noise, and the colour operations applied (3 by default, 4 + the sums with contrast)
    out["augment_batch_algorithmic_mb"] = round((2 * (3 + 4 * C_ANN) + 6 + 3 * 6) * px / 1e6, 2)

    def batch():
        return augs.train_batch(img, ann, CHANNEL, C2T, (OUT, OUT), (OUT, OUT), rng)

    out["train_batch_host_ms"] = round(clock(batch, max(a.reps // 3, 5)), 3)
    crop = ann[:, :OUT, :OUT].contiguous()
    out["gen_targets_batch_host_ms"] = round(clock(lambda: gen_targets_batch(crop, CHANNEL, C2T, (OUT, OUT)), max(a.reps // 3, 5)), 3)
    tasks = ["Lumen", "Gland", "Nuclei", "Nuclei#TYPE", "Gland#TYPE"]
    m = create_model(**default_model_kwargs(considered_tasks=tasks))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(0, considered_tasks=tasks).items()}, strict=True)
    info = ({"net": {"desc": m, "optimizer": Adam(lr=1.0e-4), "extra_info": {"loss": PARAMSET_LOSS}}}, None)
    b = batch()
    res = [None]

    def step():
        res[0] = train_step(b, info)

    out["train_step_host_ms"] = round(clock(step, 6), 3)
    out["train_step_workload"] = "batch 16 x 448 x 448, five dense heads (no Patch-Class), fed by train_batch"
    out["train_step_overall_loss"] = res[0]["EMA"]["overall_loss"]
    out["augment_share_of_step"] = round(out["augment_batch_ms"] / out["train_step_host_ms"], 5)
    print(json.dumps({k: v for k, v in out.items() if k != "kernels"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
