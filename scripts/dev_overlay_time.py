"""Measures the device overlays (cerberus_amd/viz.py, csrc/overlay.hip) and writes profiles/overlay.json.

  tile job          run_infer_tile.py's work (InferManager.process_file_list) on 96 PNG tiles of 1000 x 1000 seeded pixels, --overlay=host against
                    --overlay=device in ONE process on one warmed model: one warm run of each, then --reps alternating pairs; host clock around the call
                    (it returns when every file is written).  The host mode is the path of before this option, untouched.
  --job-only MODE   the same job once, nothing else: the run to put under `rocprofv3 --kernel-trace --stats` for the GPU time (kernel durations summed,
                    model loading included); --stats-csv DIR reads such a run's *kernel_stats.csv back into the JSON.
                    The seeded test weights find about ONE instance per tile of seeded pixels: the job times everything around the per-contour loop
                    (x2 up-scaling, conversions, JPEG, .mat files), not the loop.  The next three figures use structured maps for that reason.
  tile overlay      clear + stamp + resolve (draw_contours_device on arrays already on the device) by stream events for one 2000 x 2000 picture:
                    a 1000 x 1000 tile whose probability maps hold ~600 nuclei, 14 glands and 30 lumina (cerberus_amd.synth_maps), labelled and
                    traced at x2 as the tile driver does, up = 2.
  slide overlay     the same for a 5000 x 5000 picture standing for a 40000 x 40000 slide at ds = 8 with the instance COUNT such a slide has in
                    BASELINE runs (885 k nuclei, 6 k glands, 3 k lumina); the contours are synthetic polygons of the usual sizes, not a model's output.
  PIL difference    over --diff-tiles such structured tiles: host drawing time per tile (visualize_instances_dict_orig on the x2 picture) and the share of
                    painted pixels (either picture differs from the plain x2 source) in which the two pictures differ.  Information only.

    python scripts/dev_overlay_time.py [--reps 3] [--tiles 96] [--out profiles/overlay.json]
"""
import argparse
import glob
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


def make_tiles(dst, n, side):
    from PIL import Image

    from cerberus_amd.wsi import synth_slide

    os.makedirs(dst, exist_ok=True)
    for i in range(n):
        Image.fromarray(synth_slide(side, side, seed=100 + i).cpu().numpy()).save(os.path.join(dst, "t%03d.png" % i))


def run_job(manager, inp, out, mode):
    shutil.rmtree(out, ignore_errors=True)
    t0 = time.perf_counter()
    manager.process_file_list({"input_dir": inp, "output_dir": out, "batch_size": 10, "patch_input_shape": 448, "patch_output_shape": 144,
                               "patch_output_overlap": 0, "nr_inference_workers": 0, "nr_post_proc_workers": 0,
                               "postproc_list": ["gland", "lumen", "nuclei", "patch-class"], "rank": 0, "world_size": 1, "overlay": mode})
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def tile_parts(side, seed):
    """What process_file_list builds for one image with overlay='device' -- (parts, info_all) -- for a tile whose probability maps hold the structures
    of a real tile (cerberus_amd.synth_maps: ~600 nuclei per Mpx, glands, lumina; class maps in coarse blocks).  The seeded test weights find about one
    instance in a tile of seeded pixels, which would time an empty loop."""
    from cerberus_amd import synth_maps as synth
    from cerberus_amd.postproc import info_from_table, inst_contours_device, inst_table_device
    from cerberus_amd.wsi import WSIRunner

    rs = np.random.RandomState(seed)
    maps = {"Nuclei-INST": synth.nuclei_maps(side, side, seed, 600.0, noise=0.02), "Gland-INST": synth.blob_maps(side, side, seed + 1, 14, 20.0, 70.0, rim=4.0, sharp=1.0, noise=0.02, holes=0.3),
            "Lumen-INST": synth.blob_maps(side, side, seed + 2, 30, 8.0, 30.0, rim=2.0, sharp=1.0, noise=0.02)}
    blocks = -(-side // 16)
    types = {"Nuclei": np.kron(rs.randint(0, 7, (blocks, blocks)), np.ones((16, 16), np.int64)).astype(np.uint8)[:side, :side],
             "Gland": np.kron(rs.randint(0, 3, (blocks, blocks)), np.ones((16, 16), np.int64)).astype(np.uint8)[:side, :side]}
    inst, _ = WSIRunner.postprocess({k: torch.from_numpy(v).cuda() for k, v in maps.items()}, wsi_mode=False)
    res = {"inst": inst, "type": {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in types.items()}}
    parts, info_all, prev = [], {}, None

    def up2(t):
        return t.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1).contiguous()

    for tissue in ("Gland", "Lumen", "Nuclei"):
        lab = res["inst"][tissue]
        tmap = res["type"].get(tissue)
        if tissue != "Lumen" and tmap is not None:
            prev = up2(tmap)
        lab2 = up2(lab)
        tab_dev = inst_table_device(lab2, prev)
        cnts, pts, offs = inst_contours_device(lab2, tab_dev)
        tab = tab_dev.cpu().numpy()
        parts.append((tissue, tab, cnts, pts, offs, prev is not None, 1.0))
        info_all[tissue] = info_from_table(tab, cnts, pts, offs, prev is not None)
    return parts, info_all


def to_device(groups):
    out = []
    for g in groups:
        d = dict(g)
        d["points"] = torch.from_numpy(np.ascontiguousarray(np.asarray(g["points"]).astype(np.int32))).cuda()
        d["offsets"] = torch.from_numpy(np.asarray(g["offsets"], np.int64)).cuda()
        d["counts"] = torch.from_numpy(np.asarray(g["counts"], np.int32)).cuda()
        d["colours"] = torch.from_numpy(np.asarray(g["colours"], np.uint32).view(np.int32)).cuda()
        out.append(d)
    return out


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


def synthetic_slide_groups(rng, side, ds):
    """Instance arrays in slide coordinates with the counts of a 40000^2 slide: polygons round random centres."""
    from cerberus_amd.viz import DEFAULT_VIZ_INFO, colour_word

    groups = []
    for tissue, n, k, radius in (("gland", 6000, 40, 150.0), ("lumen", 3000, 24, 50.0), ("nuclei", 885000, 12, 8.0)):
        cen = rng.randint(0, side, (n, 1, 2))
        ang = np.linspace(0, 2 * np.pi, k, endpoint=False)[None, :, None]
        r = radius * rng.uniform(0.6, 1.4, (n, k, 1))
        pts = (cen + r * np.concatenate([np.cos(ang), np.sin(ang)], axis=2)).astype(np.int64).reshape(-1, 2)
        counts = np.full(n, k, np.int32)
        vi = DEFAULT_VIZ_INFO[tissue]
        cols = np.array([colour_word(c) for c in list(vi["type_colour"].values())[1:] + [vi["inst_colour"]]], np.uint32)
        groups.append({"points": pts, "offsets": np.cumsum(counts, dtype=np.int64) - counts, "counts": counts, "colours": cols[rng.randint(0, len(cols), n)],
                       "width": 2, "mul": 1, "div": ds, "origin": (0, 0)})
    return groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tiles", type=int, default=96)
    ap.add_argument("--side", type=int, default=1000)
    ap.add_argument("--diff-tiles", type=int, default=12)
    ap.add_argument("--job-only", default=None, choices=["host", "device"])
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "overlay.json"))
    a = ap.parse_args()
    if a.stats_csv and os.path.exists(a.out):  # the profiled runs came after the timing run: add their sums to its file
        with open(a.out) as fh:
            out = json.load(fh)
        out["tile_job_gpu_kernel_s"] = dict(read_stats(a.stats_csv), note="kernel durations summed over one profiled process per mode (rocprofv3 --kernel-trace "
                                            "--stats, a run of its own): model loading and its calibration tile included")
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        print(json.dumps(out["tile_job_gpu_kernel_s"]))
        return
    from PIL import Image

    from cerberus_amd.tile import InferManager
    from cerberus_amd.viz import draw_contours_device, pack_parts, up2_nearest, visualize_instances_dict_orig
    from cerberus_amd.weights import DEFAULT_REQ_TARGET_CODE, default_model_kwargs

    work = tempfile.mkdtemp(prefix="cerb_overlay_")
    inp = os.path.join(work, "in")
    try:
        make_tiles(inp, a.tiles, a.side)
        manager = InferManager(checkpoint_path=None, decoder_dict=dict(DEFAULT_REQ_TARGET_CODE), model_args=default_model_kwargs())
        if a.job_only:
            print(json.dumps({"mode": a.job_only, "wall_s": round(run_job(manager, inp, os.path.join(work, "out"), a.job_only), 3)}), flush=True)
            return
        out = {"device": torch.cuda.get_device_name(0), "job": "%d PNG tiles of %d x %d, patch 448 / 144, batch 10, CERB_TILE_IO_THREADS=%s" % (
            a.tiles, a.side, a.side, os.environ.get("CERB_TILE_IO_THREADS", "4")), "tile_job_wall_s": {"host": [], "device": []}}
        for mode in ("host", "device"):  # warm: code objects, allocator, page cache
            out.setdefault("tile_job_warm_run_s", {})[mode] = round(run_job(manager, inp, os.path.join(work, "out"), mode), 3)
        for _ in range(a.reps):
            for mode in ("host", "device"):
                out["tile_job_wall_s"][mode].append(round(run_job(manager, inp, os.path.join(work, "out"), mode), 3))
                print(json.dumps({mode: out["tile_job_wall_s"][mode][-1]}), flush=True)
        for mode in ("host", "device"):
            v = out["tile_job_wall_s"][mode]
            out["tile_job_wall_s"][mode + "_median"] = float(np.median(v))
            out["tile_job_wall_s"][mode + "_spread"] = round(max(v) - min(v), 3)
        # ---- PIL against the device picture; host drawing time
        diff, painted, host_ms, n_inst, first = 0, 0, [], 0, None
        for i in range(a.diff_tiles):
            img = np.array(Image.open(os.path.join(inp, "t%03d.png" % (i % a.tiles))).convert("RGB"))
            parts, info_all = tile_parts(a.side, 40 + 3 * i)
            if first is None:
                first = (img, parts)
            plain = up2_nearest(img)
            t0 = time.perf_counter()
            host = visualize_instances_dict_orig(plain, info_all)
            host_ms.append((time.perf_counter() - t0) * 1e3)
            dev = draw_contours_device(img, pack_parts(parts), 2).cpu().numpy()
            either = (host != plain).any(axis=2) | (dev != plain).any(axis=2)
            painted += int(either.sum())
            diff += int((host != dev).any(axis=2).sum())
            n_inst += sum(len(v) for v in info_all.values())
        out["pil_difference"] = {"tiles": a.diff_tiles, "instances": n_inst, "maps": "structured probability maps (synth_maps), not the test weights' output", "painted_pixels": painted, "differing_pixels": diff,
                                 "share_of_painted": round(diff / max(painted, 1), 4), "host_draw_ms_per_tile_median": round(float(np.median(host_ms)), 2),
                                 "host_draw_ms_per_tile_max": round(float(np.max(host_ms)), 2)}
        # ---- one 2000^2 tile picture by events
        img, parts = first
        groups = to_device(pack_parts(parts))
        src = torch.from_numpy(img).cuda()
        out["tile_overlay_2000"] = dict(events(lambda: draw_contours_device(src, groups, 2), 30), contours=int(sum(int((g["counts"] > 0).sum()) for g in groups)),
                                        segments=int(sum(int(g["counts"].sum()) for g in groups)), picture="%d x %d" % (2 * img.shape[0], 2 * img.shape[1]))
        # ---- a 5000^2 slide picture by events
        rng = np.random.RandomState(5)
        groups = to_device(synthetic_slide_groups(rng, 40000, 8))
        thumb = torch.from_numpy(rng.randint(0, 256, (5000, 5000, 3)).astype(np.uint8)).cuda()
        out["slide_overlay_5000"] = dict(events(lambda: draw_contours_device(thumb, groups, 1), 20), contours=int(sum(len(g["counts"]) for g in groups)),
                                         segments=int(sum(int(g["counts"].sum()) for g in groups)), picture="5000 x 5000", div=8,
                                         note="instance counts of a 40000^2 slide; synthetic polygons, not a model's contours")
        print(json.dumps(out), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(out, fh, indent=1)
            fh.write("\n")
        print("wrote", a.out)
    finally:
        shutil.rmtree(work, ignore_errors=True)


def read_stats(root):
    """{mode: seconds}: the summed kernel durations of <root>/<mode>/**/*kernel_stats.csv (rocprofv3 --kernel-trace --stats)."""
    import csv

    got = {}
    for mode in ("host", "device"):
        total = 0
        for path in glob.glob(os.path.join(root, mode, "**", "*kernel_stats.csv"), recursive=True):
            with open(path) as fh:
                for row in csv.DictReader(fh):
                    total += int(float(row.get("TotalDurationNs", 0) or 0))
        got[mode] = round(total / 1e9, 3) if total else None
    return got


if __name__ == "__main__":
    main()
