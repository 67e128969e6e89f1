"""Measures the polygon fill (cerberus_amd/rasterize.py, csrc/overlay.hip: cerb_overlay_fill / _labels) and writes profiles/poly_fill.json.

  slide   a 40000 x 40000 int32 label map filled in windows (rasterize.fill_windows: 3 x 3 windows, the plane under 1 GiB) from the synthetic slide
          of scripts/dev_overlay_time.py (the instance COUNTS of a 40000^2 run: 885 k nuclei, 6 k glands, 3 k lumina; synthetic polygons of the
          usual sizes, not a model's contours), one part at a time: device time per kind of call -- clear, fill, stamp (width 1), labels -- summed
          over the windows, by stream events round every call.
  tile    the same four calls for one 2000 x 2000 map: a 1000 x 1000 tile's structured probability maps labelled and traced at x2 as the tile driver
          does (dev_overlay_time.tile_parts): real traced contours, a gland of a few thousand points over a box of many cells.
  labels  the labels pass reads 4 and writes 4 bytes per pixel: 8 B / px over its time is the bandwidth it reaches (no memory counters collected).
  host    the alternative on the same contours: PIL.ImageDraw.polygon into mode-"I" images, the map cut into 16 row bands drawn by 16 threads, plus the
          upload of the finished map.  A different fill rule (PIL's); timed, not compared.

Median and range over --reps runs after one warm-up run.

    python scripts/dev_poly_fill_time.py [--reps 20] [--host-reps 3] [--out profiles/poly_fill.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

CALLS = ("clear", "fill", "stamp", "labels")


def figures(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4), "reps": len(ts)}


def device_times(shape, group, out, reps):
    """{call: figures} for one group filled into `out` (CUDA int32 [H, W]) window by window; events round every call, summed per kind of call"""
    from cerberus_amd import _lib
    from cerberus_amd.rasterize import fill_windows
    from cerberus_amd.viz import _group_to_device

    L = _lib.lib()
    dev = out.device
    h, w = shape
    windows = fill_windows(h, w)
    n = len(group["counts"])
    pts, offs, cnts, _ = _group_to_device(dict(group, colours=np.zeros(n, np.uint32)), dev, "dev_poly_fill_time")
    table = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    ph, pw = max(y1 - y0 for _, y0, _, y1 in windows), max(x1 - x0 for x0, _, x1, _ in windows)
    ws = torch.empty(ph * pw, dtype=torch.int32, device=dev)
    st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    mul, div = int(group.get("mul", 1)), int(group.get("div", 1))
    took = {c: [] for c in CALLS}
    for rep in range(reps + 1):
        marks = []
        for x0, y0, x1, y1 in windows:
            wh, ww = y1 - y0, x1 - x0
            nb = int(L.cerb_overlay_workspace_bytes(wh, ww))
            view = out[y0:y1, x0:x1]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            _lib.check(L.cerb_overlay_clear(ws.data_ptr(), nb, wh, ww, st))
            ev[1].record()
            _lib.check(L.cerb_overlay_fill(pts.data_ptr(), offs.data_ptr(), cnts.data_ptr(), n, mul, div, x0, y0, 0, ws.data_ptr(), nb, wh, ww, st))
            ev[2].record()
            _lib.check(L.cerb_overlay_stamp(pts.data_ptr(), offs.data_ptr(), cnts.data_ptr(), n, mul, div, x0, y0, 1, 0, ws.data_ptr(), nb, wh, ww, st))
            ev[3].record()
            _lib.check(L.cerb_overlay_labels(table.data_ptr(), n, 0, ws.data_ptr(), nb, view.data_ptr(), int(out.stride(0)) * 4, wh, ww, st))
            ev[4].record()
            marks.append(ev)
        torch.cuda.synchronize(dev)
        if rep:  # (the first run warms up)
            for i, c in enumerate(CALLS):
                took[c].append(sum(ev[i].elapsed_time(ev[i + 1]) for ev in marks))
    res = {c: figures(v) for c, v in took.items()}
    res["windows"], res["contours"], res["points"] = len(windows), n, int(np.asarray(group["counts"]).sum())
    res["labels_gb_per_s_at_8_bytes_per_px"] = round(8.0 * h * w / (res["labels"]["median_ms"] * 1e-3) / 1e9, 1)
    return res


def host_times(shape, group, reps, threads=16):
    """PIL.ImageDraw.polygon into "I" images, one row band per thread, then the upload: seconds per run"""
    from PIL import Image, ImageDraw

    h, w = shape
    pts = np.asarray(group["points"], np.int64).reshape(-1, 2)
    offs, cnts = np.asarray(group["offsets"], np.int64), np.asarray(group["counts"], np.int64)
    live = np.nonzero(cnts >= 3)[0]
    ymin = np.array([pts[o:o + c, 1].min() for o, c in zip(offs[live], cnts[live])]) if len(live) else np.zeros(0, np.int64)
    ymax = np.array([pts[o:o + c, 1].max() for o, c in zip(offs[live], cnts[live])]) if len(live) else np.zeros(0, np.int64)
    rows = -(-h // threads)
    bands = [(y0, min(y0 + rows, h)) for y0 in range(0, h, rows)]

    def draw_band(band):
        y0, y1 = band
        im = Image.new("I", (w, y1 - y0), 0)
        d = ImageDraw.Draw(im)
        for i in live[(ymax >= y0) & (ymin < y1)].tolist():
            p = pts[offs[i]:offs[i] + cnts[i]].copy()
            p[:, 1] -= y0
            d.polygon(p.ravel().tolist(), fill=i + 1, outline=i + 1)
        return np.asarray(im)

    draw_s, upload_s = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        with ThreadPoolExecutor(threads) as pool:
            parts = list(pool.map(draw_band, bands))
        t1 = time.perf_counter()
        dev = [torch.from_numpy(np.ascontiguousarray(p)).cuda() for p in parts]
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        draw_s.append(t1 - t0)
        upload_s.append(t2 - t1)
        del dev, parts
    return {"draw_s": [round(v, 3) for v in draw_s], "upload_s": [round(v, 3) for v in upload_s], "draw_s_median": round(float(np.median(draw_s)), 3),
            "upload_s_median": round(float(np.median(upload_s)), 3), "threads": threads, "bands": len(bands), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--side", type=int, default=40000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poly_fill.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dev_poly_fill_time.py measures on the GPU: none found")
    import dev_overlay_time as ov

    from cerberus_amd.viz import pack_parts

    out = {"device": torch.cuda.get_device_name(0), "reps": a.reps,
           "note": "device times by stream events round each call, summed over the windows of a run; median and range over the runs after one warm-up run"}
    # ---- one 2000^2 tile: traced contours
    parts, _ = ov.tile_parts(1000, 40)
    tile_map = torch.empty((2000, 2000), dtype=torch.int32, device="cuda")
    out["tile_2000"] = {}
    for tissue in ("gland", "lumen", "nuclei"):
        packed = pack_parts([p for p in parts if p[0].lower() == tissue])
        if not packed:
            continue
        g = packed[0]
        out["tile_2000"][tissue] = device_times((2000, 2000), g, tile_map, a.reps)
        out["tile_2000"][tissue]["largest_contour_points"] = int(np.asarray(g["counts"]).max()) if len(g["counts"]) else 0
        out["tile_2000"][tissue]["host_pil"] = host_times((2000, 2000), g, a.host_reps)
        print(json.dumps({"tile": tissue, **out["tile_2000"][tissue]}), flush=True)
    # ---- the 40000^2 slide in windows: synthetic polygons with a slide's instance counts
    side = a.side
    groups = ov.synthetic_slide_groups(np.random.RandomState(5), side, 1)
    slide_map = torch.empty((side, side), dtype=torch.int32, device="cuda")
    out["slide_%d" % side] = {}
    for g, tissue in zip(groups, ("gland", "lumen", "nuclei")):
        res = device_times((side, side), g, slide_map, a.reps)
        res["host_pil"] = host_times((side, side), g, a.host_reps)
        out["slide_%d" % side][tissue] = res
        print(json.dumps({"slide": tissue, **res}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
