"""Measures the instance-feature calls (cerberus_amd/inst_features.py, csrc/inst_features.hip) and writes profiles/inst_features.json.

Maps: a --side x --side (8192) nuclei label map and a gland label map of the same size, labelled by the project's own post-processing from
cerberus_amd.synth_maps' structured probability maps (~600 nuclei per Mpx; 12 glands per Mpx).  Each figure: one warm call, then --reps calls
between stream events; median, min and max reported.

  inst_table   cerb_inst_table on the same map -- the yardstick: both are one pass over the same bytes
  inst_shape   cerb_inst_shape (the clear of the shape rows + the pass)
  hull_rows    cerb_inst_hull_rows, the whole call: clear of the extents, pass 1 over the map, pass 2 per instance (areas only, no point list)
  relate       cerb_inst_relate of the nuclei table over the gland map
  knn          cerb_points_knn, n = 8192 seeded points, k = 4
  shape_ab     run-aggregated against per-pixel atomics (CERB_INST_SHAPE_PER_PIXEL, the developers' library only): a child process on the same maps,
               the two forms alternating call by call; `equal` = both gave the same rows

    python scripts/dev_inst_features_time.py [--side 8192] [--reps 20] [--out profiles/inst_features.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4), "reps": reps}


def label_maps(side):
    from cerberus_amd import synth_maps as synth
    from cerberus_amd.postproc import postproc_device

    out = {}
    for tissue, maps in (("Nuclei", synth.nuclei_maps(side, side, 21, 600.0)), ("Gland", synth.gland_maps(side, side, 22))):
        lab, _ = postproc_device(torch.from_numpy(maps).cuda(), tissue, exact_ties=False)
        out[tissue] = lab.contiguous()
        del maps
    torch.cuda.synchronize()
    return out


def shape_calls(lab):
    """(n, table, closures over preallocated buffers) for one map"""
    from cerberus_amd import _lib
    from cerberus_amd.postproc import inst_table_device

    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h, w = int(lab.shape[0]), int(lab.shape[1])
    n = int(lab.max().item())
    table = inst_table_device(lab, None, n)
    tab2 = torch.empty_like(table)
    shape = torch.empty((n, 8), dtype=torch.int64, device="cuda")
    bh = torch.where(table[:, 0] > 0, (table[:, 4] - table[:, 3]).clamp(min=0), torch.zeros_like(table[:, 0]))
    offs = (torch.cumsum(bh, 0) - bh).contiguous()
    ext = torch.empty((max(int(bh.sum().item()), 1), 2), dtype=torch.int32, device="cuda")

    def f_table():
        _lib.check(L.cerb_inst_table(lab.data_ptr(), lab.stride(0), None, 0, h, w, n, tab2.data_ptr(), st))

    def f_shape():
        _lib.check(L.cerb_inst_shape(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), shape.data_ptr(), st))

    def f_hull():
        _lib.check(L.cerb_inst_hull_rows(lab.data_ptr(), lab.stride(0), h, w, n, table.data_ptr(), offs.data_ptr(), ext.data_ptr(), None, shape.data_ptr(), st))

    return n, table, shape, f_table, f_shape, f_hull


def ab_child(path, reps):
    """(developers' library) aggregated against per-pixel atomics on the maps the parent saved, alternating"""
    out = {}
    for tissue in ("Nuclei", "Gland"):
        lab = torch.from_numpy(np.load(os.path.join(path, tissue + ".npy"))).cuda()
        n, table, shape, _, f_shape, _ = shape_calls(lab)
        rows, ts = {}, {"aggregated": [], "per_pixel": []}
        for rep in range(reps + 1):  # (the first pair warms both forms)
            for form in ("aggregated", "per_pixel"):
                if form == "per_pixel":
                    os.environ["CERB_INST_SHAPE_PER_PIXEL"] = "1"
                else:
                    os.environ.pop("CERB_INST_SHAPE_PER_PIXEL", None)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                f_shape()
                e1.record()
                e1.synchronize()
                if rep:
                    ts[form].append(e0.elapsed_time(e1))
                else:
                    rows[form] = shape[:, :5].clone()
        os.environ.pop("CERB_INST_SHAPE_PER_PIXEL", None)
        out[tissue] = {form: {"median_ms": round(float(np.median(v)), 4), "min_ms": round(float(np.min(v)), 4), "max_ms": round(float(np.max(v)), 4), "reps": reps}
                       for form, v in ts.items()}
        out[tissue]["equal"] = bool(torch.equal(rows["aggregated"], rows["per_pixel"]))
    print("AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inst_features.json"))
    ap.add_argument("--ab-child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a.ab_child, a.reps)
    from cerberus_amd import _lib

    maps = label_maps(a.side)
    out = {"device": torch.cuda.get_device_name(0), "side": a.side, "timing": "stream events round one call, one warm call first; ms"}
    tables = {}
    for tissue, lab in maps.items():
        n, table, shape, f_table, f_shape, f_hull = shape_calls(lab)
        tables[tissue] = table
        fg = int((lab > 0).sum().item())
        out[tissue] = {"instances": n, "foreground_share": round(fg / float(lab.numel()), 4), "inst_table": events(f_table, a.reps),
                       "inst_shape": events(f_shape, a.reps), "hull_rows": events(f_hull, a.reps)}
        print(json.dumps({tissue: out[tissue]}), flush=True)
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ntab, glab = tables["Nuclei"], maps["Gland"]
    n_child, n_parent = int(ntab.shape[0]), int(tables["Gland"].shape[0])
    parent_of = torch.empty(n_child, dtype=torch.int32, device="cuda")
    prow = torch.empty((n_parent, 10), dtype=torch.int64, device="cuda")
    out["relate"] = dict(events(lambda: _lib.check(L.cerb_inst_relate(ntab.data_ptr(), n_child, None, glab.data_ptr(), glab.stride(0), a.side, a.side, 0, n_parent,
                                                                      parent_of.data_ptr(), prow.data_ptr(), st)), a.reps), children=n_child, parents=n_parent)
    pts = torch.from_numpy(np.random.RandomState(5).randint(0, 16 * a.side, (8192, 2)).astype(np.int32)).cuda()
    idx = torch.empty((8192, 4), dtype=torch.int32, device="cuda")
    d2 = torch.empty((8192, 4), dtype=torch.int64, device="cuda")
    out["knn"] = dict(events(lambda: _lib.check(L.cerb_points_knn(pts.data_ptr(), 8192, 4, idx.data_ptr(), d2.data_ptr(), st)), a.reps), n=8192, k=4)
    print(json.dumps({"relate": out["relate"], "knn": out["knn"]}), flush=True)
    work = tempfile.mkdtemp(prefix="cerb_feat_")
    try:
        for tissue, lab in maps.items():
            np.save(os.path.join(work, tissue + ".npy"), lab.cpu().numpy())
        del maps, tables
        torch.cuda.empty_cache()
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", work, "--reps", str(a.reps)], capture_output=True, text=True,
                           timeout=900, env=dict(os.environ, CERB_DEV_LIB="1"))
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("AB ")]
        if p.returncode != 0 or not lines:
            raise RuntimeError("the A/B child failed: " + p.stderr[-2000:])
        out["shape_ab"] = json.loads(lines[-1][3:])
    finally:
        import shutil

        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps({"shape_ab": out["shape_ab"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
