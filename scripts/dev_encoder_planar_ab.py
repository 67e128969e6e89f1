"""Per-launch times of the encoder's residual stages, NHWC (conv_wino4 / conv_wino4b) against tile-planar (conv_wino4p), in ONE process of the developers'
library (section 1 of profiles/encoder_planar_ab.txt).  cerb_api.hip reads CERB_ENC_PLANAR at every forward: a bit mask of the stages 1..4 allowed on the
planar path.  bench.py's batch loop (32 tiles of 256^2), per-launch events of cerb_net_profile_*, one JSON line per arm.  A stage's sum holds its
convolutions (the stride-2 ones at its entry included), its exit pass and, for stage 1, the max-pool.

    CERB_DEV_LIB=1 python scripts/dev_encoder_planar_ab.py [mask mask ...]"""
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
order = sys.argv[1:] or ["0", "15", "0", "15"]
for rnd, mask in enumerate(order):
    os.environ["CERB_ENC_PLANAR"] = mask
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
            if name.startswith("backbone.layer") or name == "maxpool":
                acc.setdefault(name, [kern, []])[1].append(ms)
    med = {k: sorted(v[1])[len(v[1]) // 2] for k, v in acc.items()}
    stage = {}
    for k, v in med.items():
        s = "1" if k == "maxpool" else k[len("backbone.layer")]
        stage[s] = stage.get(s, 0.0) + v
    fam = {}
    for k, v in acc.items():
        f = fam.setdefault(v[0], [0, 0.0])
        f[0] += 1
        f[1] += med[k]
    row = {"mask": mask, "round": rnd, "ms_per_step_timed": round(dt / 10 * 1e3, 4), "sum_of_kernels_ms": round(tot / REPS, 4),
           "stage_ms": {k: round(v, 4) for k, v in sorted(stage.items())}, "encoder_ms": round(sum(stage.values()), 4),
           "family": {k: [v[0], round(v[1], 4)] for k, v in sorted(fam.items())},
           "launch": {k: round(v, 4) for k, v in med.items()}}
    print(json.dumps(row), flush=True)
