"""Instance metrics of a run_infer_tile.py output directory against annotations, on the GPU (cerberus_amd/inst_metrics.py): per image and pooled
DQ, SQ, PQ, AJI, Dice2 and Dice1, per-class PQ with --types.  Prints one JSON line and writes <pred_dir>/stats.csv.

    python compute_stats.py --pred_dir=output/ --true_dir=annotations/ --tissue=nuclei [--types=7]

Predictions: <pred_dir>/<tissue>_mat/<name>.mat as run_infer_tile.py writes them ('inst_map'; 'id' and 'type' give the class of every instance).
Annotations: <true_dir>/<name>.mat or <name>.npy (a pickled dict) with 'inst_map' and, for --types, 'inst_type': one class per instance in
ascending id order; or polygons, <name>.json (the reference's save_json) / <name>.geojson (QuPath's export), filled into a label map of the
prediction's shape on the device.  A name that exists on one side only is an error, by name.

    python compute_stats.py --pred_dat=output/dat/slide.dat --true_ann=<slide .dat | .json | .geojson | label-map .npz> [--tissue=nuclei] [--types=7]

scores a slide from its instance dictionary alone: the contours of both sides are filled into label maps on the device (cerberus_amd/rasterize.py; the
project's own integer fill: even-odd interior plus outline, no holes), classes are the instances' 'type' entries, and <slide>_stats.csv is written
beside the .dat."""
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
    pred, true = _stems(pdir, (".mat",)), _stems(true_dir, (".mat", ".npy", ".json", ".geojson"))
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


POLYGON_EXTS = (".json", ".geojson")


def filled_annotation(path, tissue, shape=None):
    """(CUDA int32 label map, class vector by id or None) of one tissue of a polygon annotation file (.dat, .json, .geojson), filled on the device
    (cerberus_amd/rasterize.py).  shape None: the file's own 'proc_dimensions'.  Exits naming the file when it does not hold the tissue."""
    from cerberus_amd.rasterize import dict_tissues, label_maps_from_dict, load_annotations

    try:
        d, holes = load_annotations(path, tissue=tissue.capitalize())
    except ValueError as e:
        sys.exit(str(e))
    if holes:
        print("%s: %d interior rings (holes) dropped" % (path, holes), file=sys.stderr)
    keys = {k.lower(): k for k in dict_tissues(d)}
    if tissue.lower() not in keys:
        sys.exit("%s holds no %s instances (it has: %s)" % (path, tissue.lower(), ", ".join(sorted(keys)) or "none"))
    if shape is None and "proc_dimensions" not in d:
        sys.exit("%s holds no 'proc_dimensions': the shape of its label map is unknown" % path)
    return label_maps_from_dict(d, shape=shape, tissues=[keys[tissue.lower()]])[keys[tissue.lower()]]


def _npz_annotation(path, tissue, want_types):
    """(int32 label map, class vector by id or None) of a label-map .npz (keys Nuclei / Gland / Lumen, type_<Tissue>-TYPE class maps)"""
    import numpy as np

    z = np.load(path, allow_pickle=False)
    key = tissue.capitalize()
    if key not in z.files:
        sys.exit("%s holds no %r" % (path, key))
    lab = np.ascontiguousarray(z[key].astype(np.int32))
    if not want_types:
        return lab, None
    tkeys = [k for k in z.files if k.startswith("type_") and key in k]
    if not tkeys:
        sys.exit("%s: --types needs a type_%s-TYPE class map" % (path, key))
    from cerberus_amd.inst_metrics import majority_types

    return lab, majority_types(lab, np.ascontiguousarray(z[tkeys[0]].astype(np.uint8)))


def _score_dat(args, n_cls):
    """--pred_dat / --true_ann: one slide, both sides filled on the device from their contours (a label-map .npz is taken as it is)"""
    pred_path, true_path, tissue = args["--pred_dat"], args["--true_ann"], args["--tissue"]
    for p in (pred_path, true_path):
        if not os.path.isfile(p):
            sys.exit("no such file: %s" % p)
    ext = os.path.splitext(true_path)[1].lower()
    if os.path.splitext(pred_path)[1].lower() != ".dat" or ext not in (".dat", ".npz") + POLYGON_EXTS:
        sys.exit("--pred_dat takes a .dat file and --true_ann a .dat, .json, .geojson or .npz file")
    if args["--gpu"]:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args["--gpu"].split(",")[0])
    from cerberus_amd.inst_metrics import InstanceStats

    pred, pred_types = filled_annotation(pred_path, tissue)
    shape = tuple(int(v) for v in pred.shape)
    true, true_types = _npz_annotation(true_path, tissue, n_cls) if ext == ".npz" else filled_annotation(true_path, tissue, shape)
    if tuple(true.shape) != shape:
        sys.exit("prediction %s and annotation %s differ in shape" % (shape, tuple(true.shape)))
    stats = InstanceStats(n_cls)
    if n_cls:
        if pred_types is None or true_types is None:
            sys.exit("--types needs a 'type' for the instances of both files")
        stats.update(true, pred, true_types, pred_types)
    else:
        stats.update(true, pred)
    name = os.path.splitext(os.path.basename(pred_path))[0]
    return _report(args, stats, [(name, pred_path, true_path)], n_cls, os.path.splitext(pred_path)[0] + "_stats.csv")


def main(argv=None):
    args = parse("compute_stats.py", STATS_OPTIONS, argv, version="cerberus_amd compute_stats")
    if args["--pred_dat"] or args["--true_ann"]:
        if args["--pred_dir"] or args["--true_dir"]:
            sys.exit("--pred_dat / --true_ann score one slide's .dat; they do not go with --pred_dir / --true_dir")
        if not args["--pred_dat"] or not args["--true_ann"]:
            sys.exit("--pred_dat and --true_ann are required together")
    elif not args["--pred_dir"] or not args["--true_dir"]:
        sys.exit("--pred_dir and --true_dir are required")
    n_cls = int(args["--types"]) if args["--types"] else 0
    if n_cls == 1 or n_cls < 0:
        sys.exit("--types counts the background too: at least 2")
    if args["--pred_dat"]:
        return _score_dat(args, n_cls)
    files = pair_files(args["--pred_dir"], args["--true_dir"], args["--tissue"])
    if args["--gpu"]:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args["--gpu"].split(",")[0])
    import numpy as np

    from cerberus_amd.inst_metrics import InstanceStats

    stats = InstanceStats(n_cls)
    for name, pp, tp in files:
        pm = _load(pp)
        pred = np.asarray(pm["inst_map"]).astype(np.int32)
        if tp.endswith(POLYGON_EXTS):  # polygons: filled on the device at the prediction's shape
            true, true_types = filled_annotation(tp, args["--tissue"], pred.shape)
            tm = {} if true_types is None else {"inst_type": true_types}
        else:
            tm = _load(tp)
            true = np.asarray(tm["inst_map"]).astype(np.int32)
        if pred.shape != tuple(true.shape):
            sys.exit("%s: prediction %s and annotation %s differ in shape" % (name, pred.shape, tuple(true.shape)))
        if n_cls:
            if "inst_type" not in tm or "type" not in pm or "id" not in pm:
                sys.exit("%s: --types needs 'inst_type' in the annotation and 'id' / 'type' in the prediction" % name)
            if tp.endswith(POLYGON_EXTS):
                type_true = tm["inst_type"]  # (already indexed by id)
            else:
                t_ids = np.unique(true)
                type_true = _types_by_id(true, t_ids[t_ids > 0], tm["inst_type"])
            stats.update(true, pred, type_true, _types_by_id(pred, pm["id"], pm["type"]))
        else:
            stats.update(true, pred)
    return _report(args, stats, files, n_cls, os.path.join(args["--pred_dir"], "stats.csv"))


def _report(args, stats, files, n_cls, out_csv):
    """the JSON line and the CSV of the images scored"""
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
    with open(out_csv, "w", newline="") as fh:
        wr = csv.DictWriter(fh, fieldnames=list(pooled.keys()))
        wr.writeheader()
        for row in rows + [pooled]:
            wr.writerow(row)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
