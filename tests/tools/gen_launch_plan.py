"""Record tests/golden/launch_plan.json: the ordered launch list the forward and training schedules produce, per configuration.

    python tests/tools/gen_launch_plan.py [--out FILE]          (needs the GPU)

For every configuration of configs() the default six-head model is built from make_state_dict(SEED), the convolution algorithm is set explicitly (so
the load-time precision probe plays no part), the step runs once unprofiled and once profiled, and the profile's (layer name, kernel family, flops)
triples are kept in order together with NetDesc.flops(n, h, w).  Only public NetDesc methods are used: the file can be recorded before a change to
the schedules and replayed after it (tests/test_launch_plan_gpu.py), launch by launch.

The sizes are the smallest that reach each branch of the kernel rule (cerberus_amd/csrc/conv_plan.h):
  n=2 tile 64    maps of 32, 16, 8, 4 px: F(2x2) below 16 x 16, encoder stage 3 not planar
  n=1 tile 128   level-2 maps exactly 64 x 64: the conv_wino4b / planar boundary
  n=2 tile 208   lowest decoder level 26 x 26: not whole 4 x 4 tiles, level 0 stays NHWC under planar levels
  n=1 tile 256   the headline geometry: encoder stages 1..3 planar, stage 4 NHWC
  n=1 tile 448, output 144   packed items on 56^2 / 28^2, region of interest on
At tiles 256 and 448 every single deviation from the defaults runs too; three training steps on a train-packed model close the list.

The file holds string tables ("names", "families") and per configuration the records as [name index, family index, flops].
"""
import json
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
SEED = 5
PLAN = os.path.join(ROOT, "tests", "golden", "launch_plan.json")
HEADS = {"Lumen-INST": 3, "Gland-INST": 3, "Nuclei-INST": 3, "Nuclei-TYPE": 7, "Gland-TYPE": 3, "Patch-Class": 9}
DEVIATIONS = [("set_planar", 0), ("set_packed_items", 0), ("set_crop_roi", 0), ("set_head_algo", 0), ("set_head_algo", 2), ("set_conv_algo", 0),
              ("set_conv_algo", 1), ("set_conv_algo", 5), ("set_conv_algo", 7)]


def configs():
    """[{id, kind, n, tile, out, algo, switch}]: switch = (method name, value) applied after set_conv_algo, or None"""
    out = []
    for n, tile, crop in ((2, 64, 64), (1, 128, 128), (2, 208, 208), (1, 256, 256), (1, 448, 144)):
        out.append({"id": "infer-n%d-t%d" % (n, tile), "kind": "infer", "n": n, "tile": tile, "out": crop, "algo": 6, "switch": None})
    for n, tile, crop in ((1, 256, 256), (1, 448, 144)):
        for name, value in DEVIATIONS:
            algo = value if name == "set_conv_algo" else 6
            out.append({"id": "infer-n%d-t%d-%s%d" % (n, tile, name[4:], value), "kind": "infer", "n": n, "tile": tile, "out": crop, "algo": algo,
                        "switch": None if name == "set_conv_algo" else [name, value]})
    for n, tile, algo in ((2, 128, 6), (2, 128, 1), (1, 448, 6)):
        out.append({"id": "train-n%d-t%d-algo%d" % (n, tile, algo), "kind": "train", "n": n, "tile": tile, "out": tile, "algo": algo, "switch": None})
    return out


def _train_batch(n, win):
    """random targets as tests/test_train_loss_gpu.py::test_training_step_with_packed_items_equals_block_items builds them"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(77)
    batch = {"tiles": torch.randint(0, 256, (n, win, win, 3), dtype=torch.uint8, device="cuda", generator=g), "targets": {}, "flags": {},
             "keep": torch.rand((n, 512), device="cuda", generator=g) < 0.7}
    for h, c in HEADS.items():
        if h == "Patch-Class":
            batch["targets"][h] = torch.randint(0, c, (n,), device="cuda", generator=g).float()
        else:
            fg = torch.rand((n, win, win), device="cuda", generator=g) < 0.3
            batch["targets"][h] = (fg * torch.randint(1, c, (n, win, win), device="cuda", generator=g)).float()
        batch["flags"][h] = torch.ones(n, device="cuda")
    return batch


def run_config(cfg, state_dict=None):
    """-> ([(layer name, kernel family, flops)], NetDesc.flops(n, tile, tile)) of one configuration"""
    import torch

    from cerberus_amd.losses import PARAMSET_LOSS
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    if state_dict is None:
        state_dict = {k: torch.from_numpy(v) for k, v in make_state_dict(SEED).items()}
    m = create_model(**default_model_kwargs())
    m.load_state_dict(state_dict, strict=True)
    n, tile = cfg["n"], cfg["tile"]
    if cfg["kind"] == "train":
        m.train()  # the handle is created by the first switch: it has to be packed for training
    m.set_conv_algo(cfg["algo"])
    if cfg["switch"]:
        getattr(m, cfg["switch"][0])(cfg["switch"][1])
    if cfg["kind"] == "train":
        b = _train_batch(n, tile)
        step = lambda: m.train_grads(b["tiles"], b["targets"], b["flags"], PARAMSET_LOSS, b["keep"])
    else:
        tiles = torch.randint(0, 256, (n, tile, tile, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).cuda()
        step = lambda: m.infer_tiles(tiles, cfg["out"])
    step()
    m.profile(True)
    step()
    torch.cuda.synchronize()
    recs = [(r[0], r[1], r[2]) for r in m.profile_records()]
    m.profile(False)
    return recs, m.flops(n, tile, tile)


def load_plan(path=PLAN):
    """-> {config id: (config, [(name, family, flops)], flops(n, h, w))}"""
    with open(path) as f:
        doc = json.load(f)
    out = {}
    for c in doc["configs"]:
        recs = [(doc["names"][a], doc["families"][b], fl) for a, b, fl in c["records"]]
        out[c["config"]["id"]] = (c["config"], recs, c["flops_nhw"])
    return out


def main():
    import torch

    from cerberus_amd.weights import make_state_dict

    path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else PLAN
    sd = {k: torch.from_numpy(v) for k, v in make_state_dict(SEED).items()}
    names, families, docs = {}, {}, []
    for cfg in configs():
        recs, fl = run_config(cfg, sd)
        rows = [[names.setdefault(a, len(names)), families.setdefault(b, len(families)), c] for a, b, c in recs]
        docs.append({"config": cfg, "flops_nhw": fl, "records": rows})
        print("%-40s %4d launches, %d families" % (cfg["id"], len(recs), len(set(r[1] for r in recs))), flush=True)
    with open(path, "w") as f:
        f.write('{"seed": %d,\n "names": %s,\n "families": %s,\n "configs": [\n' % (SEED, json.dumps(list(names)), json.dumps(list(families))))
        f.write(",\n".join("  " + json.dumps(d) for d in docs))
        f.write("\n ]}\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
