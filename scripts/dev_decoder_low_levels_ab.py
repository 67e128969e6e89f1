"""Per-launch times of the decoder's two lowest levels, conv_wino4b (NHWC) against conv_wino4p (tile-planar), in ONE process of the developers' library
(section 1 of profiles/decoder_low_levels_planar_ab.txt).  cerb_api.hip reads CERB_PLANAR_LOWEST at every forward: 2 = the two last levels only, 1 = level 1
as well, 0 = all four.  bench.py's batch loop (32 tiles of 256^2), per-launch events of cerb_net_profile_*, one JSON line per arm.

    CERB_DEV_LIB=1 python scripts/dev_decoder_low_levels_ab.py"""
import os, sys, json
assert os.environ.get("CERB_DEV_LIB") == "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import bench
from cerberus_amd.net_desc import create_model
from cerberus_amd.weights import default_model_kwargs, make_state_dict

dev = torch.device("cuda", 0)
kw = default_model_kwargs()
sd = {k: torch.from_numpy(v) for k, v in make_state_dict(0).items()}
model = create_model(**kw)
model.load_state_dict(sd, strict=True)
model.prepare(dev)
REPS = 6
res = {}
order = ["2", "0", "1", "2", "0", "1"]
for rnd, low in enumerate(order):
    os.environ["CERB_PLANAR_LOWEST"] = low
    dt, step, n = bench.batch_loop(model, dev, 0, 10, 3, None, "nccl")
    acc = {}
    tot = 0.0
    for _ in range(REPS):
        model.profile(True)
        step()
        torch.cuda.synchronize()
        recs = model.profile_records()
        model.profile(False)
        for name, kern, fl, ms in recs:
            tot += ms
            if name.startswith("dec.0") or name.startswith("dec.1"):
                a = acc.setdefault(name, [kern, []])
                a[1].append(ms)
    row = {"lowest": low, "round": rnd, "ms_per_step_timed": round(dt / 10 * 1e3, 4), "sum_of_kernels_ms": round(tot / REPS, 4),
           "launch": {k: {"family": v[0], "median_ms": round(sorted(v[1])[len(v[1]) // 2], 4), "min_ms": round(min(v[1]), 4)} for k, v in acc.items()}}
    row["dec01_sum_ms"] = round(sum(x["median_ms"] for x in row["launch"].values()), 4)
    print(json.dumps(row), flush=True)
