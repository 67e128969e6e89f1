"""Instance metrics of a run_infer_tile.py output directory against annotations, on the GPU (cerberus_amd/inst_metrics.py): per image and pooled
DQ, SQ, PQ, AJI, Dice2 and Dice1, per-class PQ with --types.  Prints one JSON line and writes <pred_dir>/stats.csv.

    python compute_stats.py --pred_dir=output/ --true_dir=annotations/ --tissue=nuclei [--types=7]

Predictions: <pred_dir>/<tissue>_mat/<name>.mat as run_infer_tile.py writes them ('inst_map'; 'id' and 'type' give the class of every instance).
Annotations: <true_dir>/<name>.mat or <name>.npy (a pickled dict) with 'inst_map' and, for --types, 'inst_type': one class per instance in
ascending id order.  A name that exists on one side only is an error, by name."""
import csv
import json
import os
import sys

from cerberus_amd.cli import STATS_OPTIONS, parse

FIGURES = ("dq", "sq", "pq", "aji", "dice2", "dice1")


def _load(path):
    import numpy as np

    if path.endswith(".npy"):
        d = np.load(path, allow_pickle=True)
        d = d.item() if d.dtype == object else {"inst_map": d}
    else:
        import scipy.io as sio

        d = sio.loadmat(path)
    if "inst_map" not in d:
        sys.exit("%s holds no 'inst_map'" % path)
    return d


def _stems(folder, exts):
    out = {}
    for f in sorted(os.listdir(folder)):
        stem, ext = os.path.splitext(f)
        if ext in exts:
            out[stem] = os.path.join(folder, f)
    return out


def pair_files(pred_dir, true_dir, tissue):
    """[(name, pred path, true path)] sorted by name; exits naming every file that has no partner."""
    pdir = os.path.join(pred_dir, "%s_mat" % tissue.lower())
    for d in (pdir, true_dir):
        if not os.path.isdir(d):
            sys.exit("no such directory: %s" % d)
    pred, true = _stems(pdir, (".mat",)), _stems(true_dir, (".mat", ".npy"))
    lonely = ["%s (no annotation in %s)" % (pred[k], true_dir) for k in pred if k not in true]
    lonely += ["%s (no prediction in %s)" % (true[k], pdir) for k in true if k not in pred]
    if lonely:
        sys.exit("files on one side only:\n  " + "\n  ".join(lonely))
    if not pred:
        sys.exit("no .mat files in %s" % pdir)
    return [(k, pred[k], true[k]) for k in sorted(pred)]


def _types_by_id(inst_map, ids, types):
    """class vector indexed by instance id from parallel id / class lists"""
    import numpy as np

    ids = np.asarray(ids).astype(np.int64).ravel()
    types = np.asarray(types).astype(np.int64).ravel()
    if ids.size != types.size:
        sys.exit("%d instance ids but %d classes" % (ids.size, types.size))
    out = np.zeros(int(max(int(inst_map.max()), int(ids.max()) if ids.size else 0)) + 1, np.int32)
    out[ids] = types
    return out


def main(argv=None):
    args = parse("compute_stats.py", STATS_OPTIONS, argv, version="cerberus_amd compute_stats")
    if not args["--pred_dir"] or not args["--true_dir"]:
        sys.exit("--pred_dir and --true_dir are required")
    n_cls = int(args["--types"]) if args["--types"] else 0
    if n_cls == 1 or n_cls < 0:
        sys.exit("--types counts the background too: at least 2")
    files = pair_files(args["--pred_dir"], args["--true_dir"], args["--tissue"])
    if args["--gpu"]:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args["--gpu"].split(",")[0])
    import numpy as np

    from cerberus_amd.inst_metrics import InstanceStats

    stats = InstanceStats(n_cls)
    for name, pp, tp in files:
        pm, tm = _load(pp), _load(tp)
        pred = np.asarray(pm["inst_map"]).astype(np.int32)
        true = np.asarray(tm["inst_map"]).astype(np.int32)
        if pred.shape != true.shape:
            sys.exit("%s: prediction %s and annotation %s differ in shape" % (name, pred.shape, true.shape))
        if n_cls:
            if "inst_type" not in tm or "type" not in pm or "id" not in pm:
                sys.exit("%s: --types needs 'inst_type' in the annotation and 'id' / 'type' in the prediction" % name)
            t_ids = np.unique(true)
            stats.update(true, pred, _types_by_id(true, t_ids[t_ids > 0], tm["inst_type"]), _types_by_id(pred, pm["id"], pm["type"]))
        else:
            stats.update(true, pred)
    groups = stats.groups()
    rows = []
    for (name, _, _), per in zip(files, stats.per_image()):
        row = {"name": name}
        row.update((k, per["all"][k]) for k in FIGURES)
        row.update(("pq_class%d" % g, per[g]["pq"]) for g in groups[1:])
        rows.append(row)
    scal = stats.scalars()
    pooled = {"name": "pooled"}
    pooled.update((k, scal["all-%s" % k]) for k in FIGURES)
    pooled.update(("pq_class%d" % g, scal["class%d-pq" % g]) for g in groups[1:])
    result = {"tissue": args["--tissue"].lower(), "images": len(files), "per_image": rows, "pooled": pooled,
              "mean": dict((k, scal["all-%s-mean" % k]) for k in FIGURES), "counters": stats.counters()["all"]}
    if n_cls:
        result["mpq"] = scal["mpq"]
    out_csv = os.path.join(args["--pred_dir"], "stats.csv")
    with open(out_csv, "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=list(pooled.keys()))
        wr.writeheader()
        for row in rows + [pooled]:
            wr.writerow(row)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
