"""Instance morphometry and gland-level relations of a finished inference run, on the GPU (cerberus_amd/inst_features.py): one CSV per tissue with
the shape of every instance (moments, axes, crack perimeter, convex hull, solidity, ...), the gland of every nucleus and lumen, and per gland its
nuclei per class, its lumen fraction and its nearest glands.  Prints one JSON line with the counts per image.

    python compute_features.py --pred_dir=output/ [--knn=4]        # <pred_dir>/{nuclei,gland,lumen}_mat/<name>.mat of run_infer_tile.py
    python compute_features.py --npz=output/slide.npz [--knn=4]    # the label maps of run_infer_wsi.py --save_label_maps
    python compute_features.py --dat=output/dat/slide.dat [--knn=4]  # the instance dictionary alone: its contours are filled on the device

Writes <pred_dir>/features/<name>_{nuclei,gland,lumen}.csv (for --npz and --dat: features/ beside the file, <name> = the file's stem).  A tissue without a
.mat file (or key) is left out.  On a slide the gland and lumen maps may be at half the nuclei map's resolution; any other ratio is refused."""
import json
import os
import sys

from cerberus_amd.cli import FEATURES_OPTIONS, parse

TISSUES = ("nuclei", "gland", "lumen")


def _mat_names(pred_dir):
    """{name: {tissue: path}} over the three <tissue>_mat directories"""
    names = {}
    for t in TISSUES:
        d = os.path.join(pred_dir, "%s_mat" % t)
        if not os.path.isdir(d):
            continue
        for f in sorted(os.listdir(d)):
            stem, ext = os.path.splitext(f)
            if ext == ".mat":
                names.setdefault(stem, {})[t] = os.path.join(d, f)
    return names


def _types_by_id(inst_map, ids, types):
    import numpy as np

    ids = np.asarray(ids).astype(np.int64).ravel()
    types = np.asarray(types).astype(np.int64).ravel()
    if ids.size != types.size:
        sys.exit("%d instance ids but %d classes" % (ids.size, types.size))
    out = np.zeros(int(max(int(inst_map.max()) if inst_map.size else 0, int(ids.max()) if ids.size else 0)) + 1, np.int32)
    out[ids] = np.maximum(types, 0)  # (run_infer_tile.py writes -1 for an instance without a class)
    return out


def _load_mats(paths):
    """{tissue: int32 map}, nuclei class vector by id or None"""
    import numpy as np
    import scipy.io as sio

    maps, types = {}, None
    for t, p in paths.items():
        d = sio.loadmat(p)
        if "inst_map" not in d:
            sys.exit("%s holds no 'inst_map'" % p)
        maps[t] = np.ascontiguousarray(np.asarray(d["inst_map"]).astype(np.int32))
        if t == "nuclei" and "id" in d and "type" in d and np.asarray(d["id"]).size:
            types = _types_by_id(maps[t], d["id"], d["type"])
    return maps, types


def _load_npz(path):
    """{tissue: int32 map}, nuclei class MAP or None"""
    import numpy as np

    z = np.load(path, allow_pickle=False)
    maps = {t: np.ascontiguousarray(z[k].astype(np.int32)) for t, k in zip(TISSUES, ("Nuclei", "Gland", "Lumen")) if k in z.files}
    if not maps:
        sys.exit("%s holds none of the keys Nuclei, Gland, Lumen" % path)
    tkeys = [k for k in z.files if k.startswith("type_") and "Nuclei" in k]
    types = np.ascontiguousarray(z[tkeys[0]].astype(np.uint8)) if tkeys and "nuclei" in maps else None
    return maps, types


def _load_dat(path):
    """{tissue: CUDA int32 map}, nuclei class vector by id or None -- the maps filled on the device from the dictionary's contours
    (cerberus_amd/rasterize.py).  The slide driver keeps gland and lumen at half the resolution and stores their contours doubled: when every gland and
    lumen coordinate is even, those two maps are filled at half the resolution (div = 2), which gives back the driver's own maps."""
    import numpy as np

    from cerberus_amd.rasterize import dict_tissues, label_maps_from_dict, load_annotations

    d, _ = load_annotations(path)
    if "proc_dimensions" not in d:
        sys.exit("%s holds no 'proc_dimensions'" % path)
    keys = {k.lower(): k for k in dict_tissues(d)}
    have = [t for t in TISSUES if t in keys]
    if not have:
        sys.exit("%s holds none of the keys Nuclei, Gland, Lumen" % path)
    coarse = [np.asarray(e["contour"]) for t in ("gland", "lumen") if t in keys for e in d[keys[t]].values() if e.get("contour") is not None]
    half = bool(coarse) and all(not (c & 1).any() for c in coarse)
    got = label_maps_from_dict(d, tissues=[keys[t] for t in have], div={keys[t]: 2 for t in ("gland", "lumen") if t in keys and half})
    maps = {t: got[keys[t]][0] for t in have}
    return maps, (got[keys["nuclei"]][1] if "nuclei" in have else None)


def _shift(name, maps):
    """the shift between the nuclei grid and the gland / lumen grid; exits, by name, on maps that do not fit together"""
    from cerberus_amd.inst_features import shift_for

    for t, m in maps.items():
        if m.ndim != 2:
            sys.exit("%s: the %s map has shape %s, not [H, W]" % (name, t, m.shape))
    if "gland" in maps and "lumen" in maps and maps["gland"].shape != maps["lumen"].shape:
        sys.exit("%s: gland map %s and lumen map %s differ in shape" % (name, maps["gland"].shape, maps["lumen"].shape))
    if "nuclei" in maps and "gland" in maps:
        try:
            return shift_for(maps["nuclei"].shape, maps["gland"].shape)
        except ValueError as e:
            sys.exit("%s: %s" % (name, e))
    return 0


def main(argv=None):
    args = parse("compute_features.py", FEATURES_OPTIONS, argv, version="cerberus_amd compute_features")
    if sum(bool(args[k]) for k in ("--pred_dir", "--npz", "--dat")) != 1:
        sys.exit("exactly one of --pred_dir, --npz and --dat is required")
    try:
        k = int(args["--knn"])
    except ValueError:
        sys.exit("--knn takes an integer, got %r" % args["--knn"])
    if k < 0 or k > 8:
        sys.exit("--knn must lie in 0 .. 8, got %d" % k)
    jobs = []
    if args["--pred_dir"]:
        if not os.path.isdir(args["--pred_dir"]):
            sys.exit("no such directory: %s" % args["--pred_dir"])
        names = _mat_names(args["--pred_dir"])
        if not names:
            sys.exit("no .mat files in %s/{nuclei,gland,lumen}_mat" % args["--pred_dir"].rstrip("/"))
        out_dir = os.path.join(args["--pred_dir"], "features")
        jobs = [(name, lambda p=paths: _load_mats(p)) for name, paths in sorted(names.items())]
    else:
        src = args["--npz"] or args["--dat"]
        if not os.path.isfile(src):
            sys.exit("no such file: %s" % src)
        out_dir = os.path.join(os.path.dirname(os.path.abspath(src)), "features")
        jobs = [(os.path.splitext(os.path.basename(src))[0], (lambda: _load_npz(src)) if args["--npz"] else (lambda: _load_dat(src)))]
    if args["--dat"] and args["--gpu"]:  # (this loader fills its maps on the device)
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args["--gpu"].split(",")[0])
    loaded = []
    for name, load in jobs:  # every refusal before the first byte goes to the GPU
        maps, types = load()
        loaded.append((name, maps, types, _shift(name, maps)))
    if args["--gpu"]:
        os.environ.setdefault("HIP_VISIBLE_DEVICES", args["--gpu"].split(",")[0])
    from cerberus_amd.inst_features import tissue_features, write_csv

    os.makedirs(out_dir, exist_ok=True)
    images = []
    for name, maps, types, shift in loaded:
        tabs = tissue_features(maps.get("nuclei"), maps.get("gland"), maps.get("lumen"), nuclei_type=types, shift=shift, k=k)
        row = {"name": name, "shift": shift}
        for t, cols in tabs.items():
            write_csv(os.path.join(out_dir, "%s_%s.csv" % (name, t)), cols)
            row[t] = int(cols["id"].numel())
        images.append(row)
    result = {"images": images, "knn": k, "out_dir": out_dir}
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
