"""Measures the tile-stream encoder and the slide overlay pyramid (cerberus_amd/tiff_pyramid.py, viz.slide_overlay_pyramid, cerb_jpeg_enc_tiles) and
writes profiles/overlay_tiff.json.  Two parts, each a run of its own (give each its own time limit), merged into the one file:

  --part scan      the 5000 x 5000 synthetic slide picture of profiles/jpeg_encode.json, edge-padded to 5120 x 5120, 4:2:0, quality 75; its coefficients
                   are computed once, then cerb_jpeg_enc_tiles at tile 256 and at tile 512 and cerb_jpeg_enc_scan of the same coefficients are timed
                   with stream events, ALTERNATING in one process, medians of --reps after a warm-up, each with its spread.  --parent-lib names a
                   shared library built from the PARENT commit's csrc/jpeg_encode.hip alone (plus a one-line cerb_set_error); its cerb_jpeg_enc_scan
                   is timed beside this commit's.  Without it only this commit's scan is timed, and the file says so.
  --part pyramid   a side x side (default 20000) pyramidal TIFF of JPEG tiles at the processing resolution (stain-field texture, 256-pixel tiles,
                   quality 80: the texture of bench.py's ingest slide) with SYNTHETIC instance arrays (one 12-gon nucleus per 43 x 43 pixels, one
                   40-gon gland per 2000 x 2000) through slide_overlay_pyramid: wall time split into read, draw, reduce, encode, download and file
                   write (the device is waited for between the stages), file size, peak device bytes; then the HOST comparison: the same levels,
                   already drawn and reduced on the device and downloaded, encoded tile by tile with PIL on 16 threads and written through the same
                   PyramidWriter (so the host figure leaves out drawing and reducing).

    python scripts/dev_overlay_tiff_time.py --part scan|pyramid [--reps 20] [--side 20000] [--parent-lib PATH] [--out profiles/overlay_tiff.json]
"""
import argparse
import ctypes as C
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(ts):
    return {"median_ms": round(float(np.median(ts)), 4), "min_ms": round(float(np.min(ts)), 4), "max_ms": round(float(np.max(ts)), 4), "reps": len(ts)}


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


def part_scan(reps, parent_lib):
    from cerberus_amd import _lib
    from cerberus_amd.tiff_pyramid import tile_prefix, tiles_workspace_bytes
    from cerberus_amd.wsi import synth_slide

    L = _lib.lib()
    pic = synth_slide(5000, 5000, seed=7)
    idx = torch.arange(5120, device=pic.device).clamp(max=4999)
    pic = pic[idx][:, idx].contiguous()
    h = w = 5120
    sp = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sizes = [int(L.cerb_jpeg_enc_workspace_bytes(w, h, 2, k)) for k in range(4)]
    planes = torch.empty((sizes[0],), dtype=torch.uint8, device="cuda")
    coefs = torch.empty((sizes[1] // 2,), dtype=torch.int16, device="cuda")
    _lib.check(L.cerb_jpeg_enc_coefs(pic.data_ptr(), pic.stride(0), w, h, 75, 2, coefs.data_ptr(), None, planes.data_ptr(), planes.numel(), sp))
    scan_ws = torch.empty((sizes[2],), dtype=torch.uint8, device="cuda")
    scan_out = torch.empty((sizes[3],), dtype=torch.uint8, device="cuda")
    scan_len = torch.zeros((1,), dtype=torch.int64, device="cuda")
    calls, keep, totals = {}, [], {}

    def scan_of(lib):
        return lambda: _lib.check(lib.cerb_jpeg_enc_scan(coefs.data_ptr(), w, h, 2, scan_ws.data_ptr(), scan_ws.numel(), scan_out.data_ptr(), sizes[3],
                                                          scan_len.data_ptr(), sp))

    calls["scan_this_commit"] = scan_of(L)
    if parent_lib:
        P = C.CDLL(os.path.abspath(parent_lib))
        P.cerb_jpeg_enc_scan.argtypes = L.cerb_jpeg_enc_scan.argtypes
        calls["scan_parent_commit"] = scan_of(P)
    for tile in (256, 512):
        ws_b, cap = tiles_workspace_bytes(w, h, tile, 2)
        n = (w // tile) * (h // tile)
        ws = torch.empty((ws_b,), dtype=torch.uint8, device="cuda")
        out = torch.empty((cap,), dtype=torch.uint8, device="cuda")
        meta = torch.zeros((2 * n + 1,), dtype=torch.int64, device="cuda")
        prefix = tile_prefix(tile, 2)
        keep.append((ws, out, meta))
        calls["tiles_%d" % tile] = (lambda tile=tile, ws=ws, out=out, meta=meta, n=n, prefix=prefix, cap=cap: _lib.check(L.cerb_jpeg_enc_tiles(
            coefs.data_ptr(), w, h, tile, 2, prefix, len(prefix), ws.data_ptr(), ws.numel(), out.data_ptr(), cap, meta.data_ptr(), meta.data_ptr() + 8 * (n + 1), sp)))
        totals["tiles_%d" % tile] = (meta, n)
    for fn in calls.values():  # warm-up: code objects
        fn()
        fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(reps):  # alternating: neighbours on the machine disturb every variant alike
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    res = {"picture": "5000 x 5000 synthetic slide (seed 7) edge-padded to 5120 x 5120", "subsampling": "4:2:0", "quality": 75,
           "timed": "stream events round one call (memset + 4 launches), alternating in one process, after a warm-up"}
    for k in calls:
        res[k] = stats(ts[k])
    res["scan_bytes"] = int(scan_len.item())
    for k, (meta, n) in totals.items():
        res[k]["bytes"] = int(meta[n].item())
        res[k]["tiles"] = n
        res[k]["workgroups_entropy"] = n * (int(k.split("_")[1]) // 16)
    res["scan_this_commit"]["workgroups_entropy"] = h // 16
    base = "scan_parent_commit" if parent_lib else "scan_this_commit"
    res["compared_with"] = base if parent_lib else base + " (no --parent-lib given: the parent commit's library was NOT timed)"
    for k in ("tiles_256", "tiles_512"):
        res[k]["slower_outside_both_spreads"] = bool(res[k]["min_ms"] > res[base]["max_ms"])
        res[k]["faster_outside_both_spreads"] = bool(res[k]["max_ms"] < res[base]["min_ms"])
    return res


def make_slide(path, side):
    from PIL import Image

    from cerberus_amd import reader as rd
    from cerberus_amd.synth_tiles import stain_field

    rs = np.random.RandomState(17)
    atlas = [np.clip(stain_field(256, 100 + i).astype(np.int16) + rs.randint(-10, 11, (256, 256, 3)), 0, 255).astype(np.uint8) for i in range(64)]
    n = -(-side // 256)
    pick = rs.randint(0, 64, (n, n))
    img = np.empty((n * 256, n * 256, 3), np.uint8)
    for ty in range(n):
        for tx in range(n):
            img[ty * 256:(ty + 1) * 256, tx * 256:(tx + 1) * 256] = atlas[pick[ty, tx]]
    img = img[:side, :side]
    cache = {}

    def enc(t):
        key = t.tobytes()
        if key not in cache:
            b = io.BytesIO()
            Image.fromarray(t).save(b, format="JPEG", quality=80)
            cache[key] = b.getvalue()
        return cache[key]

    rd.write_tiled_tiff(path, [img], tile=256, mpp=0.5, encode=(enc, 7))


def make_instances(side):
    """(parts, extra): one 12-gon nucleus of radius 6 per 43 x 43 pixels (jittered), typed; one 40-gon gland of radius 400 per 2000 x 2000"""
    rs = np.random.RandomState(3)
    g = np.arange(21, side - 21, 43)
    cy, cx = np.meshgrid(g, g, indexing="ij")
    c = np.stack([cx.reshape(-1), cy.reshape(-1)], axis=1) + rs.randint(-12, 13, (cx.size, 2))
    a = np.arange(12) * (2 * np.pi / 12)
    ring = np.round(np.stack([np.cos(a), np.sin(a)], axis=1) * 6).astype(np.int64)
    pts = (c[:, None, :] + ring[None]).reshape(-1, 2)
    n = c.shape[0]
    cnts = np.full(n, 12, np.int32)
    parts = [("Nuclei", np.ones((n, 8), np.int64), cnts, pts, np.arange(n, dtype=np.int64) * 12, False, 1.0)]
    a = np.arange(40) * (2 * np.pi / 40)
    ring = np.round(np.stack([np.cos(a), np.sin(a)], axis=1) * 400).astype(np.int64)
    gl = {}
    for y in range(1000, side, 2000):
        for x in range(1000, side, 2000):
            gl["g%d_%d" % (y, x)] = {"contour": ring + (x, y)}
    return parts, {"Gland": gl}, n, len(gl)


def part_pyramid(side, tile):
    from concurrent.futures import ThreadPoolExecutor

    from PIL import Image

    from cerberus_amd.reader import TiffReader
    from cerberus_amd.tiff_pyramid import PyramidWriter
    from cerberus_amd.viz import slide_overlay_pyramid

    work = tempfile.mkdtemp(prefix="cerb_overlay_tiff_")
    src, dst, host = os.path.join(work, "slide.tif"), os.path.join(work, "overlay.tif"), os.path.join(work, "overlay_host.tif")
    t0 = time.perf_counter()
    make_slide(src, side)
    parts, extra, n_nuc, n_gl = make_instances(side)
    res = {"slide": "%d x %d JPEG-tiled TIFF at the processing resolution (256-pixel tiles, quality 80, stain-field texture), %.1f MB" % (side, side, os.path.getsize(src) / 1e6),
           "instances": "SYNTHETIC arrays, not an inference result: %d nuclei (12 points each), %d glands (40 points each)" % (n_nuc, n_gl),
           "tile": tile, "quality": 75, "build_s": round(time.perf_counter() - t0, 1)}
    reader = TiffReader(src)
    slide_overlay_pyramid(reader, 0.5, parts, extra, dst, tile=tile)  # warm: code objects, allocator, page cache
    runs = []
    for _ in range(2):
        tm = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sizes = slide_overlay_pyramid(reader, 0.5, parts, extra, dst, tile=tile, timings=tm)
        tm["wall_s"] = time.perf_counter() - t0
        runs.append({k: (round(v, 3) if isinstance(v, float) else v) for k, v in tm.items()})
        print(json.dumps(runs[-1]), flush=True)
    res["device_runs"] = runs
    res["levels"] = [list(s) for s in sizes]
    t0 = time.perf_counter()
    slide_overlay_pyramid(reader, 0.5, parts, extra, dst, tile=tile)
    torch.cuda.synchronize()
    res["device_wall_s_without_stage_waits"] = round(time.perf_counter() - t0, 3)
    # the host's side of the comparison: the drawn levels as the device file holds them are NOT re-read (lossy); the levels are rebuilt on the device
    # without encoding, downloaded, and then encoded by PIL tile by tile
    from cerberus_amd.viz import draw_contours_device, half_width_viz_info, pack_parts

    levels = []
    if side <= 32768:
        px = torch.from_numpy(reader.read_bounds((0, 0, side, side), 1.0, "baseline")).cuda()
        cur = draw_contours_device(px, pack_parts(parts, extra, half_width_viz_info(), ds=1))
        del px
        for w, h in sizes:
            levels.append(cur.cpu().numpy())
            if (w, h) != sizes[-1]:
                p = cur[torch.arange(h + h % 2, device="cuda").clamp(max=h - 1)][:, torch.arange(w + w % 2, device="cuda").clamp(max=w - 1)].to(torch.int32)
                s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
                cur = ((s >> 2) + (((s & 3) > 2) | (((s & 3) == 2) & ((s >> 2) & 1 == 1))).to(torch.int32)).to(torch.uint8)
        del cur
        torch.cuda.empty_cache()

        def enc_tile(job):
            k, y, x = job
            a = levels[k]
            t = a[y:y + tile, x:x + tile]
            if t.shape[:2] != (tile, tile):
                t = np.pad(t, ((0, tile - t.shape[0]), (0, tile - t.shape[1]), (0, 0)), mode="edge")
            b = io.BytesIO()
            Image.fromarray(np.ascontiguousarray(t)).save(b, format="JPEG", quality=75, subsampling=2)
            return b.getvalue()

        t0 = time.perf_counter()
        wr = PyramidWriter(host, side, side, tile, 75, 2, mpp=0.5)
        n_tiles = 0
        with ThreadPoolExecutor(16) as pool:
            for k, a in enumerate(levels):
                jobs = [(k, y, x) for y in range(0, a.shape[0], tile) for x in range(0, a.shape[1], tile)]
                datas = list(pool.map(enc_tile, jobs, chunksize=16))
                for i, d in enumerate(datas):  # (complete streams, not abbreviated ones: libtiff takes both)
                    wr.add_tiles(k, [i], d, [0], [len(d)])
                n_tiles += len(jobs)
        wr.close()
        res["host_pil_16_threads"] = {"wall_s": round(time.perf_counter() - t0, 3), "tiles": n_tiles, "file_bytes": os.path.getsize(host),
                                      "covers": "PIL encode of every tile on 16 threads + the file write; NOT the read, the drawing or the reduction"}
    for p in (src, dst, host):
        if os.path.exists(p):
            os.remove(p)
    os.rmdir(work)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", required=True, choices=["scan", "pyramid"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--side", type=int, default=20000)
    ap.add_argument("--tile", type=int, default=256)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay_tiff.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "this script measures on the GPU"
    out = load(a.out)
    out["device"] = torch.cuda.get_device_name(0)
    out[a.part] = part_scan(a.reps, a.parent_lib) if a.part == "scan" else part_pyramid(a.side, a.tile)
    print(json.dumps({a.part: out[a.part]}), flush=True)
    save(a.out, out)


if __name__ == "__main__":
    main()
