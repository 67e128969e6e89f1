"""Measures the device JPEG encoder (cerberus_amd/jpeg_encode.py, csrc/jpeg_encode.hip) and writes profiles/jpeg_encode.json.  Three parts, each a run
of its own (give each its own time limit), merged into the one file:

  --part pictures   one 2000 x 2000 tile picture (a 1000 x 1000 synthetic slide region up-scaled x2, as the tile driver's overlays are) and one
                    5000 x 5000 slide picture, 4:2:0, quality 75: stream events round cerb_jpeg_enc_coefs, round cerb_jpeg_enc_scan and round the whole
                    encode (the copy of the compressed bytes to pinned memory included), medians after a warm-up; the host clock round
                    Encoder.encode(...).bytes(); and PIL's Image.save of the same arrays on this host (median of 5).  Compressed sizes of both.
  --part job        run_infer_tile.py's work (InferManager.process_file_list) on 96 PNG tiles of 1000 x 1000, --overlay=device, with
                    --overlay_encode=host against device in ONE process on one warmed model: one warm run of each, then --reps alternating pairs.
  --part trace      --reps encodes of each picture and nothing else: the run to put under `rocprofv3 --kernel-trace --stats`;
  --stats-csv DIR   reads such a run's *kernel_stats.csv and *kernel_trace.csv back into the file (per-kernel time, together and per picture).

    python scripts/dev_jpeg_encode_time.py --part pictures|job|trace [--reps 3] [--out profiles/jpeg_encode.json]
"""
import argparse
import glob
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def pictures():
    from cerberus_amd.wsi import synth_slide

    tile = synth_slide(1000, 1000, seed=100)
    tile = tile.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1).contiguous()
    return {"tile_2000": tile, "slide_5000": synth_slide(5000, 5000, seed=7).contiguous()}


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4), "reps": len(ts)}


def time_picture(pic, reps):
    import ctypes as C

    from PIL import Image

    from cerberus_amd import _lib
    from cerberus_amd import jpeg_encode as je

    h, w = int(pic.shape[0]), int(pic.shape[1])
    enc = je.Encoder(pic.device, w, h)
    L = _lib.lib()
    st = torch.cuda.current_stream()
    sp = C.c_void_p(st.cuda_stream)

    def coefs():
        _lib.check(L.cerb_jpeg_enc_coefs(pic.data_ptr(), pic.stride(0), w, h, 75, 2, enc._coefs.data_ptr(), enc._qt.data_ptr(), enc._planes.data_ptr(),
                                         enc._planes.numel(), sp))

    def scan():
        _lib.check(L.cerb_jpeg_enc_scan(enc._coefs.data_ptr(), w, h, 2, enc._scan_ws.data_ptr(), enc._scan_ws.numel(), enc._scan.data_ptr(), enc.scan_cap,
                                        enc._len.data_ptr(), sp))

    def by_events(fn):
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
        return stats(ts)

    out = {"picture": "%d x %d" % (h, w), "subsampling": "4:2:0", "quality": 75, "encoder_device_bytes": enc.device_bytes()}
    out["coefs_call_events"] = by_events(coefs)
    out["scan_call_events"] = by_events(scan)
    handles = []
    out["encode_events"] = by_events(lambda: handles.append(enc.encode(pic)))  # kernels + the two copies to pinned memory
    data = handles[-1].bytes()
    out["device_file_bytes"] = len(data)
    wall = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        enc.encode(pic).bytes()
        wall.append((time.perf_counter() - t0) * 1e3)
    out["encode_to_bytes_host_clock"] = stats(wall)
    # the host path of today: download + PIL
    arr = pic.cpu().numpy()
    pil, sizes = [], []
    for _ in range(6):
        buf = io.BytesIO()
        t0 = time.perf_counter()
        Image.fromarray(arr).save(buf, format="JPEG")
        pil.append((time.perf_counter() - t0) * 1e3)
        sizes.append(buf.tell())
    out["pil_save_host_clock"] = stats(pil[1:])
    out["pil_file_bytes"] = sizes[-1]
    dl = []
    for _ in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pic.cpu().numpy()
        dl.append((time.perf_counter() - t0) * 1e3)
    out["download_host_clock"] = stats(dl[1:])
    out["same_pixels_as_pil"] = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")),
                                                    np.asarray(Image.open(io.BytesIO(buf.getvalue())).convert("RGB"))))
    return out


def make_tiles(dst, n, side):
    from PIL import Image

    from cerberus_amd.wsi import synth_slide

    os.makedirs(dst, exist_ok=True)
    for i in range(n):
        Image.fromarray(synth_slide(side, side, seed=100 + i).cpu().numpy()).save(os.path.join(dst, "t%03d.png" % i))


def run_job(manager, inp, out, encode):
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.perf_counter()
    manager.process_file_list({"input_dir": inp, "output_dir": out, "batch_size": 10, "patch_input_shape": 448, "patch_output_shape": 144,
                               "patch_output_overlap": 0, "nr_inference_workers": 0, "nr_post_proc_workers": 0,
                               "postproc_list": ["gland", "lumen", "nuclei", "patch-class"], "rank": 0, "world_size": 1, "overlay": "device",
                               "overlay_encode": encode})
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def load(path):
    if os.path.exists(path):
        with open(path) as fh:
            return json.load(fh)
    return {}


def save(path, out):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print("wrote", path)


def read_stats(root):
    """{kernel: {calls, total_ms, mean_us}} of <root>/**/*kernel_stats.csv (rocprofv3 --kernel-trace --stats), the encoder's kernels only"""
    import csv

    got = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Name", "")
                if "jpeg_enc_" not in name:
                    continue
                short = name[name.index("jpeg_enc_"):].split("(")[0]
                calls, total = int(float(row.get("Calls", 0) or 0)), float(row.get("TotalDurationNs", 0) or 0)
                got[short] = {"calls": calls, "total_ms": round(total / 1e6, 4), "mean_us": round(total / max(calls, 1) / 1e3, 2)}
    # the two pictures apart: the kernel trace's own rows, grouped by the launch's grid (the larger grid is the 5000 x 5000 picture's)
    per = {}
    for path in glob.glob(os.path.join(root, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            for row in csv.DictReader(fh):
                name = row.get("Kernel_Name", "")
                if "jpeg_enc_" in name:
                    short = name[name.index("jpeg_enc_"):].split("(")[0]
                    per.setdefault(short, {}).setdefault(int(row["Grid_Size_X"]), []).append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    for short, grids in per.items():
        keys = sorted(grids)
        names = ["both"] if len(keys) == 1 else ["tile_2000", "slide_5000"]
        got.setdefault(short, {})["median_us"] = {n: round(float(np.median(grids[k])), 2) for n, k in zip(names, keys)}
    return got


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", default=None, choices=["pictures", "job", "trace"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=96)
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_encode.json"))
    a = ap.parse_args()
    out = load(a.out)
    if a.stats_csv:
        out["kernels_under_rocprofv3"] = dict(read_stats(a.stats_csv), note="--part trace under rocprofv3 --kernel-trace --stats, a run of its own: the encodes "
                                              "of one 2000 x 2000 and one 5000 x 5000 picture TOGETHER, warm-up encodes included")
        save(a.out, out)
        return
    assert torch.cuda.is_available(), "this script measures on the GPU"
    out["device"] = torch.cuda.get_device_name(0)
    if a.part == "trace":
        from cerberus_amd import jpeg_encode as je

        for name, pic in pictures().items():
            enc = je.Encoder(pic.device, pic.shape[1], pic.shape[0])
            for _ in range(a.reps + 1):
                n = len(enc.encode(pic).bytes())
            print(name, n, "bytes")
        return
    if a.part == "pictures":
        for name, pic in pictures().items():
            out[name] = time_picture(pic, max(a.reps, 20))
            print(json.dumps({name: out[name]}), flush=True)
        save(a.out, out)
        return
    from cerberus_amd.tile import InferManager
    from cerberus_amd.weights import DEFAULT_REQ_TARGET_CODE, default_model_kwargs

    work = tempfile.mkdtemp(prefix="cerb_jpeg_enc_")
    inp = os.path.join(work, "in")
    try:
        make_tiles(inp, a.tiles, a.side)
        manager = InferManager(checkpoint_path=None, decoder_dict=dict(DEFAULT_REQ_TARGET_CODE), model_args=default_model_kwargs())
        job = {"job": "%d PNG tiles of %d x %d, patch 448 / 144, batch 10, --overlay=device, CERB_TILE_IO_THREADS=%s" % (
            a.tiles, a.side, a.side, os.environ.get("CERB_TILE_IO_THREADS", "4")), "wall_s": {"host": [], "device": []}, "warm_run_s": {}}
        for mode in ("host", "device"):  # warm: code objects, allocator, page cache
            job["warm_run_s"][mode] = round(run_job(manager, inp, os.path.join(work, "out"), mode), 3)
        for _ in range(a.reps):
            for mode in ("host", "device"):
                job["wall_s"][mode].append(round(run_job(manager, inp, os.path.join(work, "out"), mode), 3))
                print(json.dumps({mode: job["wall_s"][mode][-1]}), flush=True)
        for mode in ("host", "device"):
            v = job["wall_s"][mode]
            job["wall_s"][mode + "_median"] = float(np.median(v))
            job["wall_s"][mode + "_spread"] = round(max(v) - min(v), 3)
        lo = {m: (min(job["wall_s"][m]), max(job["wall_s"][m])) for m in ("host", "device")}
        job["difference_outside_both_spreads"] = bool(lo["device"][1] < lo["host"][0] or lo["host"][1] < lo["device"][0])
        out["tile_job"] = job
        print(json.dumps(job), flush=True)
        save(a.out, out)
    finally:
        shutil.rmtree(work, ignore_errors=True)


if __name__ == "__main__":
    main()
