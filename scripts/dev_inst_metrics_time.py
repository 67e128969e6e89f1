"""Times the instance-metrics pass (cerberus_amd/inst_metrics.py, csrc/inst_metrics.hip) on label maps made by the project's own nuclei labelling of
cerberus_amd.synth_maps probability maps:

  1024 x 1024            a map against the labelling of the same probabilities shifted by 2 px
  8192 x 8192, self      a map against itself
  8192 x 8192, shifted   a map against a copy shifted by 2 px

per case: pair_table + panoptic_quality (host clock, synchronised: uploads excluded, the maps are on the device), the three pixel passes alone (stream
events; Gpx/s, bytes read per pixel from the shapes against the algorithmic 8 B/px of reading each map once), the share of table updates that reach
global memory, and two baselines: the same contingency table from torch primitives on the same GPU (one int64 key per pixel, torch.unique with
counts) and -- 1024 x 1024 only -- the numpy restatement on the host (tests/inst_metrics_ref.py).

    python scripts/dev_inst_metrics_time.py [--big 8192] [--reps 30] [--out profiles/inst_metrics.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def clock(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


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
    return float(np.median(ts))


_PROB = {}


def label_pair(size, seed, density, shifted):
    from cerberus_amd.postproc import postproc_device
    from cerberus_amd.synth_maps import nuclei_maps

    key = (size, seed, density)
    if key not in _PROB:
        _PROB.clear()
        _PROB[key] = nuclei_maps(size, size, seed, density_per_mpx=density)  # host numpy; made once per map
    prob = torch.from_numpy(_PROB[key]).cuda()
    true, _ = postproc_device(prob, "Nuclei", exact_ties=False)
    if not shifted:
        return true, true.clone()
    pred, _ = postproc_device(torch.roll(prob, (2, 0), (0, 1)).contiguous(), "Nuclei", exact_ties=False)
    return true, pred


def torch_table(t, p):
    both = (t > 0) & (p > 0)
    key = (t.to(torch.int64) << 32) | p.to(torch.int64)
    return torch.unique(key[both], return_counts=True)


def run_case(name, t, p, reps, host_ref):
    from cerberus_amd import _lib, inst_metrics as im

    L = _lib.lib()
    h, w = int(t.shape[0]), int(t.shape[1])
    px = h * w
    res = {"case": name, "h": h, "w": w}
    tab = im.pair_table(t, p)
    pq = im.panoptic_quality(tab)
    res.update(n_true=int(tab.true_ids.numel()), n_pred=int(tab.pred_ids.numel()), n_pairs=tab.n_pairs, retries=tab.retries, pq=pq["pq"], tp=pq["tp"])
    ms = clock(lambda: im.panoptic_quality(im.pair_table(t, p)), reps)
    res["pair_table_pq_ms"] = ms
    res["pair_table_pq_gpx_s"] = px / ms / 1e6
    nt, npd = int(t.max()), int(p.max())
    ms_bound = clock(lambda: im.panoptic_quality(im.pair_table(t, p, max_true_id=nt, max_pred_id=npd)), reps)
    res["pair_table_pq_bounds_given_ms"] = ms_bound
    # the pixel passes alone
    area_ms = events(lambda: (im._areas(t, nt), im._areas(p, npd)), reps)
    it, _ = im._ranks(im._areas(t, nt))
    ip, _ = im._ranks(im._areas(p, npd))
    cap = im._capacity_for(4 * min(nt + npd, px // 16)) * (4 ** tab.retries)
    table = torch.empty(int(L.cerb_inst_pairs_workspace_bytes(cap)) // 8, dtype=torch.int64, device=t.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    pair_ms = events(lambda: _lib.check(L.cerb_inst_pairs(t.data_ptr(), t.stride(0), p.data_ptr(), p.stride(0), h, w, it.data_ptr(), nt, ip.data_ptr(), npd,
                                                          table.data_ptr(), cap, stream)), reps)
    res.update(area_passes_ms=area_ms, pair_pass_ms=pair_ms, pair_table_slots=cap, pair_pass_gpx_s=px / pair_ms / 1e6,
               pixel_passes_gpx_s=px / (area_ms + pair_ms) / 1e6)
    # bytes from the shapes: each area pass reads its map once (4 B/px), the pair pass both (8 B/px); the pair pass also clears its table
    res["bytes_per_px_read"] = 16.0
    res["bytes_per_px_algorithmic"] = 8.0
    res["table_clear_bytes_per_px"] = cap * 16.0 / px
    res["pixel_passes_tb_s"] = 16.0 * px / ((area_ms + pair_ms) * 1e-3) / 1e12
    a = tab.atomics
    res["table_updates_lds"] = a["lds"]
    res["table_updates_global"] = a["global"]
    res["share_global"] = a["global"] / max(a["lds"] + a["global"], 1)
    res["updates_per_px"] = (a["lds"] + a["global"]) / px
    # baseline: torch primitives on the same GPU
    keys, counts = torch_table(t, p)
    same = bool(torch.equal(((tab.pairs[:, 0] << 32) | tab.pairs[:, 1]), keys) and torch.equal(tab.pairs[:, 2], counts))
    res["torch_unique_ms"] = clock(lambda: torch_table(t, p), reps)
    res["torch_unique_same_table"] = same
    res["speedup_over_torch_unique"] = res["torch_unique_ms"] / ms
    if host_ref:
        import inst_metrics_ref as ref

        tn, pn = t.cpu().numpy(), p.cpu().numpy()
        t0 = time.perf_counter()
        want = ref.stats(tn, pn)
        res["numpy_restatement_ms"] = (time.perf_counter() - t0) * 1e3
        res["numpy_restatement_same_tp"] = bool(want["tp"] == pq["tp"])
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--big", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--density", type=float, default=1500.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inst_metrics.json"))
    a = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "density_per_mpx": a.density, "cases": []}
    t, p = label_pair(1024, 3, a.density, True)
    out["cases"].append(run_case("1024 shifted", t, p, a.reps, True))
    del t, p
    t, p = label_pair(a.big, 4, a.density, False)
    out["cases"].append(run_case("%d self" % a.big, t, p, a.reps, False))
    del t, p
    torch.cuda.empty_cache()
    t, p = label_pair(a.big, 4, a.density, True)
    out["cases"].append(run_case("%d shifted" % a.big, t, p, a.reps, False))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
