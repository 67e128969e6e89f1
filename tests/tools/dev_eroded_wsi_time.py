"""What the eroded labelling (PostProcInstErodedMap, codes IP-ERODED-3 / -11) costs at slide scale, beside the contour scheme (GPU; recorded in DESIGN.md
par.4.6, not gated).  A structured 8192^2 nuclei map at 1500 nuclei / Mpx -- the 2048^2 map of synth_maps.nuclei_maps tiled 4 x 4 on the device, so both
schemes see the same blobs from the same seed -- goes through sharded_postprocess at run_infer_wsi.py's default max_band_px: channel 0 alone as the
one-channel canvas of a two-class head, both channels as the contour scheme's canvas (postproc_device, exact_ties=False).  Warm-up, then the median of 5
runs, device events on the stream around each call (the calls read instance counts on the host: the events span those waits too).

    python tests/tools/dev_eroded_wsi_time.py [--side 8192] [--density 1500] [--seed 41] [--runs 5]"""
import argparse
import os
import sys
from collections import OrderedDict

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def timed(fn, runs):
    fn()  # warm-up: code objects, the labelling workspace
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--side", type=int, default=8192)
    ap.add_argument("--density", type=float, default=1500.0)
    ap.add_argument("--seed", type=int, default=41)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("dev_eroded_wsi_time.py measures on the GPU; there is none")
    from cerberus_amd import synth_maps
    from cerberus_amd.shard_postproc import sharded_postprocess

    max_band_px = int(float(os.environ.get("CERB_ONE_CALL_MPX", "400")) * 1e6)  # run_infer_wsi.ONE_CALL_PX
    base = min(2048, args.side)
    rep = max(1, args.side // base)
    tile = torch.from_numpy(synth_maps.nuclei_maps(base, base, args.seed, args.density, noise=0.02)).cuda()
    two = tile.repeat(rep, rep, 1).contiguous()
    one = two[..., :1].contiguous()
    del tile
    side = int(two.shape[0])

    def run(canvas):
        inst, info = sharded_postprocess(OrderedDict([("Nuclei-INST", canvas)]), 0, 1, None, wsi_mode=True, max_band_px=max_band_px)
        return info["Nuclei"]

    t_er, all_er, info_er = timed(lambda: run(one), args.runs)
    t_ct, all_ct, info_ct = timed(lambda: run(two), args.runs)
    mpx = side * side / 1e6
    print("map %d^2 (%.1f Mpx), %.0f nuclei / Mpx, seed %d, max_band_px %d" % (side, mpx, args.density, args.seed, max_band_px))
    print("eroded  (one channel,  postproc_eroded_device): median %.1f ms of %s | %.1f Mpx/s | %s" % (t_er, ["%.1f" % v for v in all_er], mpx / t_er * 1e3, info_er))
    print("contour (two channels, postproc_device, exact_ties=False): median %.1f ms of %s | %.1f Mpx/s | %s" % (t_ct, ["%.1f" % v for v in all_ct], mpx / t_ct * 1e3, info_ct))
    print("ratio eroded / contour: %.2f" % (t_er / t_ct))


if __name__ == "__main__":
    main()
