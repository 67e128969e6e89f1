"""Integration: the reference's command lines end to end on synthetic inputs (SURVEY.md par.4 'integration' row)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_run_infer_tile_cli(tmp_path):
    import scipy.io as sio
    from PIL import Image

    inp, out = tmp_path / "in", tmp_path / "out"
    inp.mkdir()
    rs = np.random.RandomState(3)
    for name, hw in (("a", (300, 421)), ("b", (256, 256))):
        Image.fromarray(rs.randint(0, 256, hw + (3,)).astype(np.uint8)).save(str(inp / (name + ".png")))
    cmd = [sys.executable, os.path.join(ROOT, "run_infer_tile.py"), "--synthetic", "--input_dir=%s" % inp, "--output_dir=%s" % out, "--batch_size=8",
           "--patch_input_shape=256", "--patch_output_shape=256"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    for t in ("gland", "lumen", "nuclei"):
        m = sio.loadmat(str(out / ("%s_mat" % t) / "a.mat"))
        assert m["inst_map"].shape == (300, 421)  # label map at source resolution (infer/tile.py:274-281)
        assert set(m.keys()) >= {"inst_map", "type", "id"}
    assert sio.loadmat(str(out / "pclass_mat" / "b.mat"))["pclass"].shape == (256, 256)
    ov = np.array(Image.open(str(out / "overlay" / "b.jpg")))
    assert ov.shape[2] == 3 and ov.shape[0] == 2 * 256  # x2 nearest-upscaled source with the instance outlines
    # resume-by-skip (infer/tile.py:225-238) is kept verbatim, including the reference's quirk: it looks for
    # "patch-class_mat/<name>.mat" (the class map is written to "pclass_mat/"), so with the CLI's target list every image
    # is always re-processed; without patch-class in the list the skip works and the reference's assert fires.
    r2 = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r2.returncode == 0 and "Done Assembling a" in r2.stdout


def test_run_infer_wsi_cli_synthetic(tmp_path):
    spec = tmp_path / "slides"
    spec.mkdir()
    (spec / "s1.txt").write_text("synthetic:700x900:5")
    out = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--output_dir=%s" % out,
           "--batch_size=6", "--patch_input_shape=448", "--patch_output_shape=144", "--save_label_maps"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    # the same slide as a .npy file on disk (memory-mapped, uploaded chunk by chunk underneath the inference): identical maps
    import torch

    from cerberus_amd.wsi import synth_slide

    npy = tmp_path / "npy"
    npy.mkdir()
    np.save(str(npy / "s1.npy"), synth_slide(700, 900, seed=5).cpu().numpy())
    r2 = subprocess.run([c.replace(str(spec), str(npy)).replace(".txt", ".npy").replace(str(out), str(tmp_path / "out2")) for c in cmd],
                        capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r2.returncode == 0, r2.stderr[-2000:]
    za, zb = np.load(str(out / "s1.npz")), np.load(str(tmp_path / "out2" / "s1.npz"))
    for k in za.files:
        assert np.array_equal(za[k], zb[k]), k
    z = np.load(str(out / "s1.npz"))
    assert z["Nuclei"].shape == (700, 900) and z["Gland"].shape == (350, 450) and z["Lumen"].shape == (350, 450)
    assert z["type_Nuclei-TYPE"].dtype == np.uint8
    import joblib

    dat = joblib.load(str(out / "dat" / "s1.dat"))
    assert set(dat.keys()) >= {"Nuclei", "Gland", "Lumen", "proc_resolution", "base_resolution", "proc_dimensions", "base_dimensions"}
    assert list(dat["proc_dimensions"]) == [700, 900] and dat["proc_resolution"]["units"] == "mpp"
    for t in ("Nuclei", "Gland", "Lumen"):
        for uid, d in dat[t].items():
            assert len(uid) == 32 and d["box"].shape == (4,) and d["contour"].ndim == 2 and d["contour"].shape[1] == 2 and (("type" in d) == (t != "Lumen"))


def test_run_infer_wsi_cli_reference_tiling(tmp_path):
    """`--reference_tiling`: the nuclei dictionary comes from the reference's tile sets and margin rules (cerberus_amd/ref_tiling.py) instead of
    band ownership.  A 700 x 900 slide fits one 4032-pixel tile, where the scheme has no seam: the dictionary must then hold exactly the
    instances of the default run (same boxes, types and contours), under fresh uuids; gland / lumen entries are untouched."""
    import joblib

    spec = tmp_path / "slides"
    spec.mkdir()
    (spec / "s1.txt").write_text("synthetic:700x900:5")
    base = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--batch_size=6",
            "--patch_input_shape=448", "--patch_output_shape=144"]
    outs = []
    for tag, extra in (("a", []), ("b", ["--reference_tiling"])):
        out = tmp_path / tag
        r = subprocess.run(base + ["--output_dir=%s" % out] + extra, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(joblib.load(str(out / "dat" / "s1.dat")))
    a, b = outs

    def key(d):
        return (tuple(int(v) for v in d["box"]), int(d.get("type", -1)), tuple(np.asarray(d["contour"]).ravel().tolist()))

    assert sorted(key(d) for d in a["Nuclei"].values()) == sorted(key(d) for d in b["Nuclei"].values())
    assert len(a["Gland"]) == len(b["Gland"]) and len(a["Lumen"]) == len(b["Lumen"])


def test_run_infer_wsi_cli_with_tissue_mask(tmp_path):
    """--msk_dir: slides without a mask are skipped, patches without tissue never run (their canvas pixels stay 0), the tissue
    map and the dictionary are written (infer/wsi.py:533-569, 688-853)."""
    import joblib
    import scipy.io as sio
    from PIL import Image

    spec, msk, out = tmp_path / "slides", tmp_path / "masks", tmp_path / "out"
    spec.mkdir()
    msk.mkdir()
    (spec / "s1.txt").write_text("synthetic:1000x1300:5")
    (spec / "nomask.txt").write_text("synthetic:600x600:6")
    m = np.zeros((100, 130), np.uint8)  # 1/10 resolution; two tissue regions in the left part of the slide
    m[5:45, 4:50] = 255
    m[60:95, 20:70] = 255
    Image.fromarray(np.stack([m] * 3, -1)).save(str(msk / "s1.png"))
    cmd = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % spec, "--msk_dir=%s" % msk, "--wsi_file_ext=.txt",
           "--output_dir=%s" % out, "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps", "--save_mask"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Number of WSIs in list: 1" in r.stdout and not (out / "dat" / "nomask.dat").exists()
    z = np.load(str(out / "s1.npz"))
    assert z["Nuclei"].shape == (1000, 1300)
    # patch columns 3.. (x >= 768) hold no mask pixel (mask columns >= 70 are empty, 70 * 10 = 700 < 768): nothing ran there
    assert z["pclass"][:, 768 // 4:].max() == 0 and z["Nuclei"][:, 768:].max() == 0 and z["type_Nuclei-TYPE"][:, 768:].max() == 0
    assert "Gland_region0" in z.files and "Gland_region1" in z.files and list(z["topleft_region1"]) == [200, 600]
    assert z["Gland_region0"].shape == (200, 230)  # the region's box (400 x 460 px at slide resolution) at x0.5
    t = sio.loadmat(str(out / "tissue" / "s1.mat"))["pclass"]
    assert t.shape == (250, 325) and t[:, 175:].max() == 0  # mask columns >= 70 -> tissue-map columns >= 175
    assert np.array_equal(np.array(Image.open(str(out / "mask" / "s1.png"))) > 0, m > 0)
    dat = joblib.load(str(out / "dat" / "s1.dat"))
    assert set(dat.keys()) >= {"Nuclei", "proc_resolution", "base_resolution", "proc_dimensions", "base_dimensions"}
    for tname in ("Gland", "Lumen"):
        for d in dat.get(tname, {}).values():
            assert d["box"].shape == (4,) and d["contour"].shape[1] == 2


def _bench(cmd, timeout=900):
    import json

    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


CONTRACT_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
                 "roofline")


def test_bench_contract_single_and_two_ranks(tmp_path):
    """bench.py (default mode: the whole slide job, here on a 3072^2 slide) prints ONE JSON line with the contract's keys; under
    torch.distributed.run with two ranks (both on this box's single GPU, host-staged gloo collectives -- RCCL refuses two ranks on
    one device) the SAME slide is sharded into two bands (strong scaling) and labelled band-locally with a halo exchange."""
    one = _bench([sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline", "--slide", "3072"])
    for k in CONTRACT_KEYS:
        assert k in one, k
    ts = one["train_step"]  # BASELINE configs[4] rides along in the default line: batch 16 x 448^2, three timed steps
    assert "error" not in ts and ts["ms_per_step"] > 0 and abs(ts["tiles_s"] - 16 / (ts["ms_per_step"] * 1e-3)) / ts["tiles_s"] < 0.01, ts
    assert ts["roofline"]["kernel"].startswith("wgrad") and 0.3 < ts["roofline"]["frac"] <= 1.0
    assert one["n_gpus"] == 1 and one["steps"] == 3 and one["unit"] == "Mpx/s" and one["scaling"] == "strong" and one["vs_baseline"] is None
    assert one["config"]["slide"] == [3072, 3072] and one["config"]["tiles"] == 144
    rf = one["roofline"]
    assert rf["bound"] == "mfma" and rf["peak"] == 157.3 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 0.01
    assert 0.25 < rf["frac"] <= 1.0, rf  # the share of the fp32 MFMA roof the kernel's own instructions fill
    # F(4x4,3x3) executes 36 of the direct convolution's 144 multiplies per 4x4 outputs (F(2x2,3x3): 16 of 36)
    assert abs(rf["algorithmic_tflops"] - rf["achieved"] * (4.0 if rf["kernel"].startswith("conv_wino4") else 36 / 16)) < 0.5
    assert abs(one["value"] - 3072 * 3072 / (one["ms_per_step"] * 1e-3) / 1e6) / one["value"] < 0.01
    assert one["config"]["inference_Mpx_s"] > one["value"] and one["config"]["whole_job_s"] >= one["config"]["inference_s"]
    assert abs(one["config"]["whole_job_s"] - one["ms_per_step"] * 1e-3) < 2e-3, one["config"]  # a step is one whole job: K steps, K jobs
    kern = {r["kernel"]: r for r in one["kernels"]}
    assert "head_group" in kern and abs(sum(r["share"] for r in one["kernels"]) - 1.0) < 0.01
    for t in ("Nuclei", "Gland", "Lumen"):
        assert one["postproc"][t]["n_inst"] > 10 and one["postproc"][t]["n_truncated"] == 0, one["postproc"]
    # round 6: the line names the algorithm the headline ran on, what the load-time probe and the head kernels' guard saw, and carries the other algorithms' figures
    cfg = one["config"]
    assert cfg["conv_algo"] == 6 and cfg["precision"]["probed"] and not cfg["precision"]["auto"] and 1.0 < cfg["precision"]["calibration_logit_absmax"] < 100.0
    assert cfg["precision"]["logit_guard"]["batches"] > 0 and cfg["precision"]["logit_guard"]["batches_above"] == 0
    assert 1.0 < cfg["precision"]["logit_guard"]["largest_abs_logit"] < 100.0
    oa = cfg["other_conv_algos"]
    assert "error" not in oa and 0 < oa["0"]["inference_Mpx_s"] < oa["1"]["inference_Mpx_s"] and oa["0"]["batch_step_ms"] > oa["1"]["batch_step_ms"] > 0, oa
    assert "error" not in one["ingest"] and one["ingest"]["best"]["of_resident"] > 0.3, one["ingest"]
    assert "error" not in one["ingest_deflate"] and one["ingest_deflate"]["best"]["of_resident"] > 0.3 and "libcerberus_host.so" in one["ingest_deflate"]["file"]["format"], one["ingest_deflate"]
    two = _bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29533",
                  "bench.py", "--gpus", "2", "--steps", "3", "--warmup", "1", "--backend", "gloo", "--slide", "3072"])
    assert two["n_gpus"] == 2 and "cpu_baseline" not in two and two["scaling"] == "strong"
    assert abs(two["value"] - 3072 * 3072 / (two["ms_per_step"] * 1e-3) / 1e6) / two["value"] < 0.01
    # same slide, same instances: band-local labelling with the halo exchange finds exactly what one GPU finds
    for t in ("Nuclei", "Gland", "Lumen"):
        assert two["postproc"][t]["n_inst"] == one["postproc"][t]["n_inst"], (t, one["postproc"][t], two["postproc"][t])
    assert two["multi_gpu"]["halo_exchange"]["bytes_into_rank0"] > 0 and two["multi_gpu"]["root_gather"]["bytes_into_rank0"] > 0


def test_bench_contract_eight_ranks_time_sharing_one_gpu():
    """The driver's 8-GPU launch line (`python -m torch.distributed.run --nnodes=1 --nproc-per-node 8 ... bench.py --gpus 8`) with the
    host-staged gloo backend, all eight ranks on this box's single GPU: one 8192^2 slide sharded into eight bands of four patch rows,
    band-local labelling with halo exchange, two all-gathers for the slide-global ids, label / class-map gather onto rank 0.  The eight-rank
    job must find exactly the instances one rank finds, with no instance cut by a band window (n_truncated == 0): the only evidence for
    BASELINE.json configs[3] this pool can give until a multi-GPU node runs it over RCCL."""
    env8 = dict(os.environ, MASTER_ADDR="127.0.0.1", CERB_WSI_BATCH="16")  # eight handles share one GPU's HBM: small batches
    import json

    def run(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=1500, cwd=ROOT, env=env8)
        assert r.returncode == 0, r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])

    one = run([sys.executable, "bench.py", "--full", "--steps", "4", "--warmup", "1", "--no-cpu-baseline", "--no-train-leg", "--no-ingest-leg", "--slide", "8192"])
    eight = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port", "29541",
                 "bench.py", "--gpus", "8", "--full", "--steps", "4", "--warmup", "1", "--backend", "gloo", "--slide", "8192", "--streams", "1"])  # (eight ranks share ONE GPU's HBM here: no second handle each)
    assert eight["n_gpus"] == 8 and eight["scaling"] == "strong" and eight["config"]["tiles"] == 1024 and "cpu_baseline" not in eight and "train_step" not in eight
    assert abs(eight["value"] - 8192 * 8192 / (eight["ms_per_step"] * 1e-3) / 1e6) / eight["value"] < 0.01
    for t in ("Nuclei", "Gland", "Lumen"):
        assert eight["postproc"][t]["n_inst"] == one["postproc"][t]["n_inst"] > 10, (t, one["postproc"][t], eight["postproc"][t])
        assert eight["postproc"][t]["n_truncated"] == 0 and eight["postproc"][t]["n_unresolved"] == 0, eight["postproc"][t]
    mg = eight["multi_gpu"]
    assert mg["halo_exchange"]["bytes_into_rank0"] > 0 and mg["root_gather"]["bytes_into_rank0"] > 0
    # round 6: the dictionary from per-rank tables + contours -- the eight ranks' owned instances make exactly the entries the one-GPU run writes,
    # and the root receives >= 20x fewer bytes than the label bands + class maps it no longer needs
    pr = eight["dat"]["per_rank_arrays"]
    assert pr["entries"] == one["dat"]["entries"] == eight["dat"]["entries"], (pr["entries"], one["dat"]["entries"])
    assert pr["bytes_into_rank0"]["ratio"] >= 20.0 and pr["tables_and_contours_s_slowest_rank"] > 0, pr


def test_bench_nccl_branch_at_world_one(tmp_path):
    """The RCCL code path on the hardware there is: `init_process_group("nccl", device_id=...)`, the warm-up gather, run_distributed's
    all-gathers and the label / class-map gathers on CUDA tensors all execute with ONE rank (RCCL accepts a single-rank communicator),
    and the result equals the plain single-process run: the same instance counts, and the same outputs in the samples --dump-outputs
    writes (class maps and probability canvases equal, label maps equal up to a renaming of the ids)."""
    da, db = tmp_path / "ref", tmp_path / "one"
    ref = _bench([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-train-leg", "--no-ingest-leg", "--slide", "2048",
                  "--dump-outputs", str(da)])
    one = _bench([sys.executable, "bench.py", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-train-leg", "--no-ingest-leg", "--slide", "2048", "--force-dist", "--backend", "nccl",
                  "--dump-outputs", str(db)])
    assert one["n_gpus"] == 1 and one["multi_gpu"] is not None and "root_gather" in one["multi_gpu"]
    for t in ("Nuclei", "Gland", "Lumen"):
        assert one["postproc"][t]["n_inst"] == ref["postproc"][t]["n_inst"]
    names = sorted(os.listdir(str(da)))
    assert names == sorted(os.listdir(str(db))) and sum(os.path.getsize(str(da / n)) for n in names) <= 64 << 20, names
    for t in ("Nuclei", "Gland", "Lumen"):
        assert "labels_%s.npy" % t in names and "canvas_%s-INST.npy" % t in names, names
    assert any(n.startswith("classes_") for n in names), names
    for n in names:
        a, b = np.load(str(da / n)), np.load(str(db / n))
        assert a.dtype in (np.float32, np.float64) and a.dtype == b.dtype and a.shape == b.shape and a.size > 0, n
        if n.startswith("labels_"):  # one id on one side <-> one id on the other, background on both sides alike
            pairs = np.unique(np.stack([a, b], 1), axis=0)
            assert len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1])) and np.array_equal(a == 0, b == 0), n
            assert (a > 0).any(), n
        else:
            assert np.array_equal(a, b), n


def test_bench_batch_mode_two_ranks():
    """--mode batch: the inner loop of configs[1], weak scaling (every rank its own 32 tiles)."""
    one = _bench([sys.executable, "bench.py", "--mode", "batch", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"])
    assert one["scaling"] == "weak" and abs(one["value"] - 32 * 256 * 256 / (one["ms_per_step"] * 1e-3) / 1e6) / one["value"] < 0.01
    two = _bench([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29535",
                  "bench.py", "--mode", "batch", "--gpus", "2", "--steps", "3", "--warmup", "1", "--backend", "gloo"])
    assert two["n_gpus"] == 2 and 0.6 < two["value"] / one["value"] < 1.25  # two ranks time-share one GPU here


def test_bench_train_mode_single_and_two_ranks():
    """bench.py --mode train: whole training steps of BASELINE configs[4] (batch 16 x 448^2 per rank); with two ranks (gloo, both on this
    box's one GPU) the gradients are averaged in buckets between the backward pass and Adam, and rank 0 reports the whole job."""
    import json

    def run(cmd):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1")
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        return json.loads(lines[0])

    one = run([sys.executable, "bench.py", "--mode", "train", "--steps", "2", "--warmup", "1"])
    assert one["unit"] == "tiles/s" and one["n_gpus"] == 1 and one["dtype"] == "f32" and one["scaling"] == "weak"
    rf, cb = one["roofline"], one["cpu_baseline"]
    assert rf["kernel"].startswith("wgrad") and rf["bound"] == "mfma" and 0.3 < rf["frac"] <= 1.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 0.01
    assert any(r["kernel"] == "bn_bwd" and r["bound"] == "hbm" and 0.1 < r["frac"] < 1.0 for r in one["kernels"])
    assert cb["kind"] == "port" and cb["unit"] == "tiles/s" and 0 < cb["value"] < one["value"]
    assert abs(one["value"] - 16 / (one["ms_per_step"] * 1e-3)) / one["value"] < 0.01
    assert 0 < one["config"]["last_overall_loss"] < 100
    two = run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29541",
               "bench.py", "--mode", "train", "--gpus", "2", "--steps", "2", "--warmup", "1", "--backend", "gloo"])
    assert two["n_gpus"] == 2 and abs(two["value"] - 2 * 16 / (two["ms_per_step"] * 1e-3)) / two["value"] < 0.01
    assert 0 < two["config"]["last_overall_loss"] < 100


def test_run_infer_wsi_cli_two_ranks_equals_one_rank(tmp_path):
    """run_infer_wsi.py end to end under torch.distributed.run with two ranks (both on this box's GPU, CERB_DIST_BACKEND=gloo = the
    host-staged collectives of cerberus_amd/hostdist.py) against the single-process run of the same slide.
    With a tissue mask the bands are gathered to the root, which labels them: every output is identical.  Without one the bands are
    labelled where they are (halo exchange, slide-global ids, label bands gathered): the stitched class maps are identical; the label
    maps of this random-weight network are slide-sized blobs, beyond the halo the band protocol resolves (tests/test_host_logic.py and
    tests/tools/dev_fuzz_drivers.py check that protocol on structured maps), so only their presence and shape are checked here."""
    import joblib
    from PIL import Image

    spec, msk = tmp_path / "slides", tmp_path / "masks"
    spec.mkdir()
    msk.mkdir()
    (spec / "s1.txt").write_text("synthetic:1500x1100:9")
    m = np.zeros((150, 110), np.uint8)
    m[10:140, 8:70] = 255
    Image.fromarray(np.stack([m] * 3, -1)).save(str(msk / "s1.png"))
    base = ["--synthetic", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", CERB_DIST_BACKEND="gloo")
    port = 29547
    for tag, extra in (("mask", ["--msk_dir=%s" % msk]), ("nomask", [])):
        one, two = tmp_path / (tag + "1"), tmp_path / (tag + "2")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--output_dir=%s" % one] + base + extra, capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                            str(port), os.path.join(ROOT, "run_infer_wsi.py"), "--output_dir=%s" % two] + base + extra, capture_output=True, text=True,
                           timeout=900, cwd=ROOT, env=env)
        port += 1
        assert r.returncode == 0, r.stderr[-3000:]
        za, zb = np.load(str(one / "s1.npz")), np.load(str(two / "s1.npz"))
        assert set(za.files) == set(zb.files)
        for k in za.files:
            assert za[k].shape == zb[k].shape, k
            if tag == "mask" or k not in ("Nuclei", "Gland", "Lumen"):
                assert np.array_equal(za[k], zb[k]), (tag, k)
        da, db = joblib.load(str(one / "dat" / "s1.dat")), joblib.load(str(two / "dat" / "s1.dat"))
        assert set(da.keys()) == set(db.keys())
        if tag == "mask":
            for t in ("Nuclei", "Gland", "Lumen"):
                ca = sorted(tuple(np.round(d["centroid"], 3)) for d in da.get(t, {}).values())
                cb = sorted(tuple(np.round(d["centroid"], 3)) for d in db.get(t, {}).values())
                assert ca == cb, t


def test_run_infer_wsi_reads_pyramidal_tiff_at_proc_mag(tmp_path):
    """A tiled pyramidal TIFF scanned at 0.25 um/px processed at --wsi_proc_mag=0.5 (infer/wsi.py:521-527) is read from its x2 level
    through cerberus_amd.reader + SlabUploader and gives exactly what the same pixels give as a .npy array; the dat records the scan
    resolution and baseline size the reader reports."""
    import joblib

    from cerberus_amd.reader import write_tiled_tiff

    rs = np.random.RandomState(4)
    base = rs.randint(0, 256, (1100, 1500, 3)).astype(np.uint8)
    l1 = np.clip(np.rint(base.astype(np.float32).reshape(550, 2, 750, 2, 3).mean(axis=(1, 3))), 0, 255).astype(np.uint8)
    a, b = tmp_path / "tif", tmp_path / "npy"
    a.mkdir()
    b.mkdir()
    write_tiled_tiff(str(a / "s1.tif"), [base, l1], tile=256, mpp=0.25)
    np.save(str(b / "s1.npy"), l1)
    # a second slide of the directory with JPEG 2000 tiles (Aperio compression 33005, lossless here): OpenJPEG behind the reader, same pixels -> same outputs
    import io

    from PIL import Image, features

    names = ["s1"]
    if features.check_codec("jpg_2000"):
        def j2k(t):
            buf = io.BytesIO()
            Image.fromarray(t).save(buf, format="JPEG2000", no_jp2=True, irreversible=False)
            return buf.getvalue()

        base2 = np.ascontiguousarray(base[::-1])
        l2 = np.ascontiguousarray(l1[::-1])
        write_tiled_tiff(str(a / "s2.tif"), [base2, l2], tile=256, mpp=0.25, encode=(j2k, 33005))
        np.save(str(b / "s2.npy"), l2)
        names.append("s2")
    outs = []
    for d, ext in ((a, ".tif"), (b, ".npy")):
        out = tmp_path / ("out" + ext[1:])
        r = subprocess.run([sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % d, "--wsi_file_ext=%s" % ext,
                            "--output_dir=%s" % out, "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256", "--wsi_proc_mag=0.5",
                            "--save_label_maps"], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(out)
    for name in names:
        za, zb = np.load(str(outs[0] / (name + ".npz"))), np.load(str(outs[1] / (name + ".npz")))
        assert set(za.files) == set(zb.files)
        for k in za.files:
            assert np.array_equal(za[k], zb[k]), (name, k)
    da, db = joblib.load(str(outs[0] / "dat" / "s1.dat")), joblib.load(str(outs[1] / "dat" / "s1.dat"))
    assert da["proc_dimensions"].tolist() == [550, 750] and da["base_dimensions"].tolist() == [1100, 1500]
    assert abs(da["base_resolution"]["resolution"] - 0.25) < 1e-3 and da["proc_resolution"]["resolution"] == 0.5
    assert db["base_dimensions"].tolist() == [550, 750]


def test_bench_gpus_two_self_spawned_without_a_launcher():
    """`python bench.py --gpus 2` WITHOUT torch.distributed.run: the script re-executes itself as two ranks (cerberus_amd/launch.py; gloo with
    --oversubscribe because this box has one GPU and RCCL refuses two ranks on a device) and the line says n_gpus 2 with both ranks listed --
    round 3's bench ignored --gpus and printed a one-GPU line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    import json

    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--backend", "gloo", "--oversubscribe", "--slide", "3072", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    two = json.loads(lines[0])
    mg = two["multi_gpu"]
    assert two["n_gpus"] == 2 and mg["world"] == 2 and [x["rank"] for x in mg["ranks"]] == [0, 1] and mg["backend"].startswith("gloo")
    assert len(set(x["pid"] for x in mg["ranks"])) == 2 and all(x["uuid"] for x in mg["ranks"])
    assert mg["halo_exchange"]["bytes_into_rank0"] > 0
    # RCCL never oversubscribes: asking for 2 ranks on a 1-GPU box over nccl is refused, not degraded
    import torch

    if torch.cuda.device_count() < 2:
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--slide", "3072"], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert r.returncode == 2 and not [l for l in r.stdout.splitlines() if l.startswith("{")]
    one = _bench([sys.executable, "bench.py", "--mode", "batch", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"])
    assert one["multi_gpu"]["world"] == 1 and one["multi_gpu"]["ranks"][0]["uuid"]


def test_run_infer_tile_two_devices_self_spawned_equals_one(tmp_path):
    """`run_infer_tile.py --gpu=0,1` (infer/base.py:46: the reference uses every listed GPU): two self-spawned ranks share the file list
    (here both on this box's GPU) and write exactly the files of the one-rank run."""
    import scipy.io as sio
    from PIL import Image

    inp = tmp_path / "in"
    inp.mkdir()
    rs = np.random.RandomState(5)
    for name, hw in (("a", (300, 421)), ("b", (256, 256)), ("c", (500, 260))):
        Image.fromarray(rs.randint(0, 256, hw + (3,)).astype(np.uint8)).save(str(inp / (name + ".png")))
    outs = []
    for tag, gpu, env in (("one", "0", dict(os.environ)), ("two", "0,1", dict(os.environ, CERB_OVERSUBSCRIBE="1"))):
        out = tmp_path / tag
        cmd = [sys.executable, os.path.join(ROOT, "run_infer_tile.py"), "--synthetic", "--gpu=%s" % gpu, "--input_dir=%s" % inp, "--output_dir=%s" % out,
               "--batch_size=8", "--patch_input_shape=256", "--patch_output_shape=256"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT, env={k: v for k, v in env.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")})
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(out)
    for name in ("a", "b", "c"):
        for t in ("gland", "lumen", "nuclei"):
            ma, mb = sio.loadmat(str(outs[0] / ("%s_mat" % t) / (name + ".mat"))), sio.loadmat(str(outs[1] / ("%s_mat" % t) / (name + ".mat")))
            assert np.array_equal(ma["inst_map"], mb["inst_map"]), (name, t)
        assert np.array_equal(sio.loadmat(str(outs[0] / "pclass_mat" / (name + ".mat")))["pclass"], sio.loadmat(str(outs[1] / "pclass_mat" / (name + ".mat")))["pclass"])


def test_run_infer_wsi_writes_a_log_per_slide_and_self_spawns(tmp_path):
    """--logging_dir: one `<slide>_<date>_std.log` per slide with the reference's phase lines (infer/wsi.py:583, 624, 684, 719, 856, 957-980);
    `--gpu=0,1` without a launcher = two self-spawned ranks (host-staged gloo on this one-GPU box) writing the same class maps."""
    import glob

    spec = tmp_path / "slides"
    spec.mkdir()
    (spec / "s1.txt").write_text("synthetic:1500x1100:9")
    base = ["--synthetic", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    one, two = tmp_path / "one", tmp_path / "two"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--output_dir=%s" % one, "--logging_dir=%s" % (tmp_path / "log1")] + base,
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    logs = glob.glob(str(tmp_path / "log1" / "s1_*_std.log"))
    assert len(logs) == 1
    text = open(logs[0]).read()
    for phrase in ("Processing s1 ...", "Preparing Input Output Placement:", "Inference Time:", "Tissue Region Post Proc Time:", "Gland & Lumen Post Proc Time:",
                   "Overall Time:", "Finish"):
        assert phrase in text, phrase
    assert " - INFO - " in text
    # second run: the slide is skipped and the log says so
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--output_dir=%s" % one, "--logging_dir=%s" % (tmp_path / "log1b")] + base,
                       capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0 and "already processed" in open(glob.glob(str(tmp_path / "log1b" / "s1_*_std.log"))[0]).read()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--gpu=0,1", "--output_dir=%s" % two, "--logging_dir=%s" % (tmp_path / "log2")] + base,
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=dict(env, CERB_DIST_BACKEND="gloo", CERB_OVERSUBSCRIBE="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "ranks: 2 over gloo" in r.stdout
    za, zb = np.load(str(one / "s1.npz")), np.load(str(two / "s1.npz"))
    for k in za.files:
        if k not in ("Nuclei", "Gland", "Lumen"):
            assert np.array_equal(za[k], zb[k]), k
    text = open(glob.glob(str(tmp_path / "log2" / "s1_*_std.log"))[0]).read()
    assert "Nuclei Post Proc Time:" in text  # the band protocol times the tissues apart


def test_second_slide_of_a_directory_is_planned_against_the_same_free_hbm_as_alone(tmp_path):
    """A directory of slides is the reference's normal job (run_infer_wsi.py:76-83 there).  plan_slide prices a slide against the FREE HBM, so nothing
    of the previous slide may still hold memory when the next one is priced: the runner, canvases and label maps (alive until their names were
    re-bound), the labelling workspace cache, the allocator's cached blocks.  The budget logged for slide b after slide a (~5 GB of canvases, labels
    and workspace) must be the budget logged for b alone."""
    import glob
    import re

    def budget_of_b(names):
        d = tmp_path / ("in_" + "".join(names))
        d.mkdir()
        for n in names:
            (d / (n + ".txt")).write_text({"a": "synthetic:6144x6144:3", "b": "synthetic:1024x1280:4"}[n])
        tag = "".join(names)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % d, "--wsi_file_ext=.txt", "--output_dir=%s" % (tmp_path / ("out_" + tag)),
                            "--logging_dir=%s" % (tmp_path / ("log_" + tag)), "--batch_size=8", "--patch_input_shape=256", "--patch_output_shape=256"],
                           capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-3000:]
        text = open(glob.glob(str(tmp_path / ("log_" + tag) / "b_*_std.log"))[0]).read()
        return int(re.search(r"Memory plan: SlidePlan\(budget=(\d+)", text).group(1))

    alone, after_a = budget_of_b(["b"]), budget_of_b(["a", "b"])
    # what legitimately stays from slide a: the second handle's packed weights and tables (~1 GB).  Before: 6.3 GB at this batch size (two forward
    # workspaces counted as used AND priced again; 50 GB at batch 64), plus slide a's own canvases while its names were alive
    assert abs(alone - after_a) < 1.5e9, (alone, after_a)


def test_run_infer_wsi_with_a_mask_labels_nuclei_in_row_bands_when_the_slide_exceeds_one_call(tmp_path):
    """--msk_dir on a slide larger than one labelling call (400 Mpx; a 49152 x 65536 scan is past the 2^31 pixels a call can address at all, and the
    masked path used to hand the whole nuclei canvas to ONE call): the nuclei go through the row bands of the mask-less path -- exact ownership,
    slide-global ids -- while gland / lumen stay per tissue region.  Here CERB_ONE_CALL_MPX moves the line under a 3072 x 2304 slide: label maps and
    dictionary entries of the banded run equal the one-call run's.  Weights: tests/tools/model_dir.py (islands a window can hold)."""
    import glob

    import joblib
    from PIL import Image

    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    from model_dir import stain_atlas, write_sparse_model_dir

    atlas = stain_atlas(16)
    H, W = 3072, 2304
    pick = np.random.RandomState(3).randint(0, 16, (H // 256, W // 256))
    img = np.concatenate([np.concatenate([atlas[i] for i in row], axis=1) for row in pick], axis=0)
    spec, msk = tmp_path / "slides", tmp_path / "masks"
    spec.mkdir()
    msk.mkdir()
    np.save(str(spec / "s1.npy"), img)
    m = np.zeros((H // 16, W // 16), np.uint8)
    m[:, : int(0.65 * W / 16)] = 255
    m[40:60, :] = 0  # two tissue regions
    Image.fromarray(np.stack([m] * 3, -1)).save(str(msk / "s1.png"))
    write_sparse_model_dir(str(tmp_path / "model"), np.stack(atlas[:4]))
    base = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--model=%s" % (tmp_path / "model"), "--input_dir=%s" % spec, "--msk_dir=%s" % msk, "--wsi_file_ext=.npy",
            "--batch_size=8", "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps"]
    outs = []
    for tag, env in (("one", dict(os.environ)), ("banded", dict(os.environ, CERB_ONE_CALL_MPX="5"))):
        r = subprocess.run(base + ["--output_dir=%s" % (tmp_path / tag), "--logging_dir=%s" % (tmp_path / ("log_" + tag))], capture_output=True, text=True, timeout=900,
                           cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        outs.append((np.load(str(tmp_path / tag / "s1.npz")), joblib.load(str(tmp_path / tag / "dat" / "s1.dat")),
                     open(glob.glob(str(tmp_path / ("log_" + tag) / "s1_*_std.log"))[0]).read()))
    (za, da, la), (zb, db, lb) = outs
    assert "row bands under the tissue mask" not in la
    import re

    nb = re.search(r"Nuclei labelled in (\d+) row bands under the tissue mask", lb)
    assert nb and int(nb.group(1)) >= 2 and "WARNING" not in lb, lb[-1500:]
    assert set(za.files) == set(zb.files) and "Nuclei" in za.files
    from cerberus_amd.shard_postproc import same_partition

    for k in za.files:
        if k == "Nuclei":  # the same instances; a single call numbers them by their markers' first pixels, the bands by the instances' own
            assert same_partition(za[k], zb[k])
        else:
            assert np.array_equal(za[k], zb[k]), k
    assert len(np.unique(zb["Nuclei"])) > 50
    assert not za["Nuclei"][:, int(0.65 * W / 16) * 16 + 256:].any()  # patches outside the mask did not run

    def entries(d):
        return sorted((tuple(int(v) for v in e["box"]), tuple(float(v) for v in np.asarray(e["centroid"], np.float64)), np.asarray(e["contour"], np.int64).tobytes(),
                       int(e.get("type", -1))) for e in d["Nuclei"].values())

    assert entries(da) == entries(db) and len(da["Nuclei"]) > 50


def test_run_infer_wsi_streams_a_slide_that_does_not_fit_the_hbm_budget(tmp_path):
    """the slide driver prices the band against the free HBM (capped here through CERB_HBM_BUDGET_GB) before it allocates
    anything; a slide that does not fit resident runs as sequential sub-bands (cerberus_amd/stream_bands.py) and must write the SAME label maps and
    class maps as the resident run, bit for bit; a budget that fits neither way ends with a ValueError that names the bytes, not with an OOM."""
    from cerberus_amd.stream_bands import plan_slide
    from cerberus_amd.tile import InferManager
    from cerberus_amd.weights import DEFAULT_REQ_TARGET_CODE, default_model_kwargs

    H, W, batch = 4300, 1100, 6
    net = InferManager(checkpoint_path=None, decoder_dict=dict(DEFAULT_REQ_TARGET_CODE), model_args=default_model_kwargs()).net
    resident = plan_slide(net, (H, W), 256, 256, batch, budget=1e15, want_twin=False, max_band_px=400 * 1000 * 1000).need
    spec = tmp_path / "slides"
    spec.mkdir()
    (spec / "s1.txt").write_text("synthetic:%dx%d:11" % (H, W))
    cmd = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--batch_size=%d" % batch,
           "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps"]
    env = dict(os.environ, CERB_WSI_STREAMS="1")
    r = subprocess.run(cmd + ["--output_dir=%s" % (tmp_path / "a"), "--logging_dir=%s" % (tmp_path / "la")], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    env_s = dict(env, CERB_HBM_BUDGET_GB="%.6f" % ((resident - 2e6) / 1e9))
    r = subprocess.run(cmd + ["--output_dir=%s" % (tmp_path / "b"), "--logging_dir=%s" % (tmp_path / "lb")], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env_s)
    assert r.returncode == 0, r.stderr[-2000:]
    logs = "".join(open(os.path.join(str(tmp_path / "lb"), f)).read() for f in os.listdir(str(tmp_path / "lb")))
    assert "mode='streamed'" in logs and "sub-bands streamed through HBM" in logs, logs[-1500:]
    assert "mode='resident'" in "".join(open(os.path.join(str(tmp_path / "la"), f)).read() for f in os.listdir(str(tmp_path / "la")))
    za, zb = np.load(str(tmp_path / "a" / "s1.npz")), np.load(str(tmp_path / "b" / "s1.npz"))
    assert set(za.files) == set(zb.files)
    for k in za.files:
        assert za[k].shape == zb[k].shape, k
        # class maps: bit for bit.  Label maps: the seeded test weights give slide-sized blobs, which no window can hold (the protocol reports them:
        # n_truncated / n_unresolved > 0, their pixels are dropped below the owner's band) -- exact equality of label maps is
        # tests/test_drivers_gpu.py::test_slide_streamed_in_sub_bands_equals_the_resident_run's job, on structured maps
        if k.startswith("type_") or k == "pclass":
            assert np.array_equal(za[k], zb[k]), k
    # round 6: the same on TWO ranks -- the budget sits just under rank 0's resident need, so rank 0 plans two sub-bands, rank 1 plans
    # resident, and the agreement makes both walk the streamed path (rank 1 in one sub-band): class maps equal the one-rank resident run's bit for bit,
    # with the maps gathered (--save_label_maps) and, without them, a dictionary of the same tissues from the per-rank arrays
    need0 = plan_slide(net, (H, W), 256, 256, batch, rank=0, world=2, budget=1e15, want_twin=False).need
    env_2 = dict(env, CERB_HBM_BUDGET_GB="%.6f" % ((need0 - 2e6) / 1e9), MASTER_ADDR="127.0.0.1", CERB_DIST_BACKEND="gloo")
    two = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29581"] + cmd[1:]
    r = subprocess.run(two + ["--output_dir=%s" % (tmp_path / "d"), "--logging_dir=%s" % (tmp_path / "ld")], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env_2)
    assert r.returncode == 0, r.stderr[-3000:]
    logs = "".join(open(os.path.join(str(tmp_path / "ld"), f)).read() for f in os.listdir(str(tmp_path / "ld")))
    assert "mode='streamed'" in logs and "sub-bands streamed through HBM" in logs, logs[-1500:]
    zd = np.load(str(tmp_path / "d" / "s1.npz"))
    assert set(za.files) == set(zd.files)
    for k in za.files:
        assert za[k].shape == zd[k].shape, k
        if k.startswith("type_") or k == "pclass":
            assert np.array_equal(za[k], zd[k]), k
    two_nomaps = [a for a in two if a != "--save_label_maps"]
    two_nomaps[two_nomaps.index("29581")] = "29582"
    r = subprocess.run(two_nomaps + ["--output_dir=%s" % (tmp_path / "e")], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env_2)
    assert r.returncode == 0, r.stderr[-3000:]
    import joblib
    import scipy.io as sio

    assert not (tmp_path / "e" / "s1.npz").exists()
    da, de = joblib.load(str(tmp_path / "a" / "dat" / "s1.dat")), joblib.load(str(tmp_path / "e" / "dat" / "s1.dat"))
    assert set(da.keys()) == set(de.keys())
    assert np.array_equal(sio.loadmat(str(tmp_path / "a" / "tissue" / "s1.mat"))["pclass"], sio.loadmat(str(tmp_path / "e" / "tissue" / "s1.mat"))["pclass"])
    env_x = dict(env, CERB_HBM_BUDGET_GB="1.0")
    r = subprocess.run(cmd + ["--output_dir=%s" % (tmp_path / "c")], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env_x)
    assert r.returncode != 0 and "ValueError" in r.stderr and "GB resident" in r.stderr, r.stderr[-1500:]


def test_bench_train_nccl_branch_at_world_one():
    """the training step's bucketed gradient all-reduce (cerberus_amd/train.py: allreduce_grads, models/opt.py has no DDP of its
    own) over a ONE-rank RCCL communicator: `bench.py --mode train --force-dist --backend nccl` must open the communicator, reduce every bucket on
    the device and train like the run without a process group (a one-rank sum / 1 is the identity)."""
    ref = _bench([sys.executable, "bench.py", "--mode", "train", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"])
    one = _bench([sys.executable, "bench.py", "--mode", "train", "--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--force-dist", "--backend", "nccl"])
    mg = one["multi_gpu"]
    assert one["n_gpus"] == 1 and mg["world"] == 1 and mg["backend"].startswith("rccl") and ref["multi_gpu"]["backend"] is None
    # (the Patch-Class dropout mask is drawn per step, unseeded: two processes agree on the loss to a few per cent, not to the bit)
    assert abs(one["config"]["last_overall_loss"] - ref["config"]["last_overall_loss"]) < 0.05 * ref["config"]["last_overall_loss"]
    phases = {r["kernel"]: r["ms_per_step"] for r in one["kernels"]}
    assert phases.get("(allreduce)", 0.0) > 0.0  # the buckets really went through the communicator


def test_run_infer_wsi_nccl_world_one_equals_no_dist(tmp_path):
    """Every collective of the N-rank slide path -- skip-flag broadcast, barriers, the band protocol's all-gathers, the label / class-map
    gathers, and (second run) --reference_tiling's tile exchange + gather_object -- over a ONE-rank RCCL communicator (CERB_FORCE_DIST=1,
    `--gpu=0`): first contact with 8 GPUs then changes N and nothing else.  Label maps, class maps and the instance dictionary's geometry must
    equal the run without a process group bit for bit."""
    import joblib

    spec = tmp_path / "slides"
    spec.mkdir()
    (spec / "s1.txt").write_text("synthetic:900x1100:5")
    base = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--gpu=0", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--batch_size=6",
            "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps"]
    for extra, tag in (([], "plain"), (["--reference_tiling"], "reftile")):
        outs = {}
        for mode in ("nodist", "nccl"):
            env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29561")
            if mode == "nccl":
                env.update(CERB_FORCE_DIST="1", CERB_DIST_BACKEND="nccl")
            out = tmp_path / ("%s_%s" % (tag, mode))
            r = subprocess.run(base + extra + ["--output_dir=%s" % out], capture_output=True, text=True, timeout=600, cwd=ROOT, env=env)
            assert r.returncode == 0, r.stderr[-2000:]
            assert ("ranks: 1 over rccl" in r.stdout) == (mode == "nccl"), r.stdout[-1500:]
            outs[mode] = out
        za, zb = np.load(str(outs["nodist"] / "s1.npz")), np.load(str(outs["nccl"] / "s1.npz"))
        assert set(za.files) == set(zb.files)
        for k in za.files:
            assert np.array_equal(za[k], zb[k]), (tag, k)
        da, db = joblib.load(str(outs["nodist"] / "dat" / "s1.dat")), joblib.load(str(outs["nccl"] / "dat" / "s1.dat"))
        for t in ("Nuclei", "Gland", "Lumen"):
            ba = sorted(tuple(int(v) for v in d["box"]) for d in da[t].values())
            bb = sorted(tuple(int(v) for v in d["box"]) for d in db[t].values())
            assert ba == bb, (tag, t, len(ba), len(bb))


def _dat_entries(path):
    import joblib

    d = joblib.load(path)
    out = {}
    for t in ("Nuclei", "Gland", "Lumen"):
        out[t] = sorted((tuple(int(v) for v in e["box"]), tuple(float(v) for v in np.asarray(e["centroid"], np.float64)), np.asarray(e["contour"], np.int64).tobytes(),
                         e.get("type"), None if "type_prob" not in e else round(float(e["type_prob"]), 12)) for e in d.get(t, {}).values())
    return out, d


def test_run_infer_wsi_dat_from_per_rank_arrays(tmp_path):
    """run_infer_wsi.py WITHOUT --save_label_maps on a process group: the ranks build instance tables + contours for the instances they own and rank 0
    only receives arrays + the quarter-resolution tissue map (cerberus_amd/shard_postproc.py gather_parts).  Over a one-rank RCCL communicator the
    dat/<slide>.dat equals the file of the run without a process group entry for entry (uuid keys aside) and tissue/<slide>.mat bit for bit; two
    ranks over host-staged gloo (both on this GPU) write the same tissue map and a dictionary with the same tissues (this random-weight network
    paints slide-sized blobs that no halo resolves: the instance-level equality of several ranks is tests/test_drivers_gpu.py's, on structured maps)."""
    import scipy.io as sio

    spec = tmp_path / "slides"
    spec.mkdir()
    (spec / "s1.txt").write_text("synthetic:1500x1100:5")
    base = ["--synthetic", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256"]
    outs = {}
    for mode in ("nodist", "nccl1", "gloo2"):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29571")
        cmd = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py")]
        if mode == "nccl1":
            env.update(CERB_FORCE_DIST="1", CERB_DIST_BACKEND="nccl")
            cmd += ["--gpu=0"]
        elif mode == "gloo2":
            env.update(CERB_DIST_BACKEND="gloo")
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", "29572",
                   os.path.join(ROOT, "run_infer_wsi.py")]
        out = tmp_path / mode
        r = subprocess.run(cmd + base + ["--output_dir=%s" % out], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-3000:]
        assert not (out / "s1.npz").exists()
        outs[mode] = out
    want, dw = _dat_entries(str(outs["nodist"] / "dat" / "s1.dat"))
    have, dh = _dat_entries(str(outs["nccl1"] / "dat" / "s1.dat"))
    assert sum(len(v) for v in want.values()) > 0
    for t in want:
        assert have[t] == want[t], (t, len(have[t]), len(want[t]))
    two, d2 = _dat_entries(str(outs["gloo2"] / "dat" / "s1.dat"))
    assert set(d2.keys()) == set(dw.keys()) == set(dh.keys())
    pm = sio.loadmat(str(outs["nodist"] / "tissue" / "s1.mat"))["pclass"]
    for mode in ("nccl1", "gloo2"):
        assert np.array_equal(sio.loadmat(str(outs[mode] / "tissue" / "s1.mat"))["pclass"], pm), mode


def test_run_infer_tile_nccl_world_one_equals_no_dist(tmp_path):
    """Tile mode shards files and has no data-path collective; its ranks still open the communicator (identity all-gather, leaving barrier).  With
    CERB_FORCE_DIST=1 and `--gpu=0` that happens over a one-rank RCCL communicator, and the written maps equal the run without one."""
    import scipy.io as sio
    from PIL import Image

    inp = tmp_path / "in"
    inp.mkdir()
    rs = np.random.RandomState(4)
    Image.fromarray(rs.randint(0, 256, (300, 280, 3)).astype(np.uint8)).save(str(inp / "a.png"))
    base = [sys.executable, os.path.join(ROOT, "run_infer_tile.py"), "--synthetic", "--gpu=0", "--input_dir=%s" % inp, "--batch_size=8", "--patch_input_shape=256",
            "--patch_output_shape=256"]
    outs = {}
    for mode in ("nodist", "nccl"):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29563")
        if mode == "nccl":
            env.update(CERB_FORCE_DIST="1", CERB_DIST_BACKEND="nccl")
        out = tmp_path / mode
        r = subprocess.run(base + ["--output_dir=%s" % out], capture_output=True, text=True, timeout=300, cwd=ROOT, env=env)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("ranks: 1 over rccl" in r.stdout) == (mode == "nccl"), r.stdout[-1500:]
        outs[mode] = out
    for t in ("gland", "lumen", "nuclei", "pclass"):
        a, b = sio.loadmat(str(outs["nodist"] / ("%s_mat" % t) / "a.mat")), sio.loadmat(str(outs["nccl"] / ("%s_mat" % t) / "a.mat"))
        key = "pclass" if t == "pclass" else "inst_map"
        assert np.array_equal(a[key], b[key]), t


def test_bench_configs2_slide_20000_full_size_one_vs_three_local_bands():
    """BASELINE configs[2] at FULL size: the whole slide job on a synthetic 20000^2 slide -- 6,241 tiles inferred, slide-sized maps
    labelled on the GPU -- once with the nuclei map labelled in one call and once in three local bands through the band protocol: no instance cut by
    a window (n_truncated == 0), the SAME instance counts either way, and the tail consuming the class canvases this job's inference wrote
    (bench.py checks their checksums against the canvases).  The one-band line is what profiles/r05_bench_wsi_20000.json holds."""
    common = [sys.executable, "bench.py", "--slide", "20000", "--steps", "4", "--warmup", "1", "--no-train-leg", "--no-ingest-leg", "--no-cpu-baseline", "--no-dat", "--no-ref-tiling"]
    one = _bench(common + ["--max-band-mpx", "420", "--full"], timeout=1500)
    three = _bench(common + ["--max-band-mpx", "150"], timeout=1500)
    assert one["config"]["slide"] == [20000, 20000] and one["config"]["tiles"] == 6241 and "configs[2]" in one["config"]["workload"]
    assert one["postproc"]["Nuclei"]["local_bands"] == 1 and three["postproc"]["Nuclei"]["local_bands"] >= 3
    for t in ("Nuclei", "Gland", "Lumen"):
        a, b = one["postproc"][t], three["postproc"][t]
        assert a["n_truncated"] == 0 and b["n_truncated"] == 0 and a["n_unresolved"] == 0 and b["n_unresolved"] == 0, (t, a, b)
        assert a["n_inst"] == b["n_inst"] > 1000, (t, a["n_inst"], b["n_inst"])
    ti = one["config"]["tail_inputs"]
    assert ti["class_canvas_checksum"] and ti["class_canvas_checksum"] == three["config"]["tail_inputs"]["class_canvas_checksum"]
    assert one["value"] > 50 and one["roofline"]["frac"] > 0.3


def test_bench_slide_20000_labels_the_canvases_its_own_inference_wrote():
    """`bench.py --tail-from-inference` -- the tail labels the INST canvases the timed inference of the SAME job wrote
    (the seeded weights with a sparse-foreground bias calibration: ~3 % of a noise slide's pixels are foreground), at BASELINE configs[2]'s full
    20000^2: the inference -> labelling data dependency at slide scale.  One labelling call against three local bands: no instance cut by a window,
    no unresolved border instance, the same instance counts -- and well above zero, i.e. the labelling really had network-made instances to own."""
    common = [sys.executable, "bench.py", "--slide", "20000", "--steps", "4", "--warmup", "1", "--no-train-leg", "--no-ingest-leg", "--no-cpu-baseline", "--no-dat", "--no-ref-tiling",
              "--tail-from-inference"]
    one = _bench(common + ["--max-band-mpx", "420"], timeout=1500)
    three = _bench(common + ["--max-band-mpx", "150"], timeout=1500)
    assert "timed inference wrote" in one["config"]["tail_inputs"]["INST probability maps"]
    assert one["postproc"]["Nuclei"]["local_bands"] == 1 and three["postproc"]["Nuclei"]["local_bands"] >= 3
    for t in ("Nuclei", "Gland", "Lumen"):
        for line in (one, three):
            assert line["postproc"][t]["n_truncated"] == 0 and line["postproc"][t]["n_unresolved"] == 0, (t, line["postproc"][t])
        assert one["postproc"][t]["n_inst"] == three["postproc"][t]["n_inst"], (t, one["postproc"][t], three["postproc"][t])
    assert one["postproc"]["Nuclei"]["n_inst"] > 10000, one["postproc"]["Nuclei"]
    assert one["config"]["precision"]["logit_guard"]["batches_above"] == 0


def test_run_infer_wsi_logit_guard_counts_and_reruns(tmp_path):
    """The slide driver's use of the data-aware guard (cerb_forward_io.logit_absmax): with the bar lowered under this model's logits (CERB_LOGIT_SATURATION=5,
    the probe switched off so that the handle stays on F(4x4)) every batch is counted in the slide's log, and CERB_LOGIT_GUARD=rerun re-runs them on
    F(2x2) -- the run completes, says so, and writes the same class maps up to rounding-sized ties."""
    spec = tmp_path / "slides"
    spec.mkdir()
    (spec / "s1.txt").write_text("synthetic:900x1100:5")
    base = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % spec, "--wsi_file_ext=.txt", "--batch_size=6",
            "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps"]
    outs = {}
    for mode, extra in (("plain", {}), ("count", {"CERB_LOGIT_SATURATION": "5", "CERB_AUTO_PRECISION": "0"}),
                        ("rerun", {"CERB_LOGIT_SATURATION": "5", "CERB_AUTO_PRECISION": "0", "CERB_LOGIT_GUARD": "rerun"})):
        out, logd = tmp_path / mode, tmp_path / (mode + "_log")
        r = subprocess.run(base + ["--output_dir=%s" % out, "--logging_dir=%s" % logd], capture_output=True, text=True, timeout=600, cwd=ROOT, env=dict(os.environ, **extra))
        assert r.returncode == 0, r.stderr[-2000:]
        outs[mode] = (out, "".join(open(os.path.join(str(logd), f)).read() for f in os.listdir(str(logd))))
    assert "Logit guard: 0 of " in outs["plain"][1]
    assert "Logit guard: 0 of " not in outs["count"][1] and "above 5" in outs["count"][1] and "re-run" not in outs["count"][1]
    assert "flagged batches re-run on F(2x2,3x3)" in outs["rerun"][1]
    za, zb, zc = (np.load(str(outs[m][0] / "s1.npz")) for m in ("plain", "count", "rerun"))
    for k in za.files:
        if k.startswith("type_") or k == "pclass":
            assert np.array_equal(za[k], zb[k]), k                      # counting changes nothing
            assert (za[k] != zc[k]).mean() < 1e-3, k                    # F(2x2) against F(4x4): argmax flips only at rounding-sized ties


def test_bench_ingest_mode_file_fed_run_equals_resident():
    """`bench.py --mode ingest` on a small slide: a JPEG-tiled pyramidal TIFF written with reader.write_tiled_tiff goes through reader ->
    decode pool -> SlabUploader's producer thread -> WSIRunner for every decode-thread count and with / without the upload-ahead thread; the leg itself asserts
    that each file-fed run writes checksum-identical canvases to the resident run of the same pixels and that the pixels do not depend on the thread count."""
    line = _bench([sys.executable, "bench.py", "--mode", "ingest", "--slide", "3072", "--streams", "1"], timeout=900)
    ing = line["ingest"]
    assert line["unit"] == "Mpx/s" and ing["slide"] == [3072, 3072] and ing["file"]["tiles"] == 144
    assert len(ing["decode"]["sweep"]) >= 3 and all(p_["Mpx_s"] > 10 for p_ in ing["decode"]["sweep"])
    modes = {(e["decode_threads"], e["upload_ahead"]) for e in ing["end_to_end_from_file"] if not e["decode_processes"]}
    assert any(not a for _, a in modes) and sum(1 for _, a in modes if a) >= 3
    assert any(e["decode_processes"] >= 4 for e in ing["end_to_end_from_file"]) and any("processes" in p_ for p_ in ing["decode"]["sweep"])
    assert not any(e["reduced_on_device"] for e in ing["end_to_end_from_file"])
    assert ing["best"]["of_resident"] > 0.3 and line["value"] == ing["best"]["Mpx_s"]
    # a 40x scan: 0.25 mpp on disk, read at 0.5 -- decoded by worker processes, reduced x2 on the device, canvases equal to those of the host-reduced rows
    line = _bench([sys.executable, "bench.py", "--mode", "ingest", "--slide", "2048", "--streams", "1", "--ingest-base-mpp", "0.25"], timeout=900)
    ing = line["ingest"]
    assert ing["slide"] == [2048, 2048] and ing["stored"] == {"pixels": [4096, 4096], "mpp": 0.25, "read_at_mpp": 0.5} and ing["file"]["tiles"] == 256
    assert all(e["reduced_on_device"] for e in ing["end_to_end_from_file"]) and ing["best"]["of_resident"] > 0.2


@pytest.mark.parametrize("codec", ["lzw"])  # (deflate tiles take the same native call: test_run_infer_wsi_reads_pyramidal_tiff_at_proc_mag reads them on the GPU box)
def test_bench_ingest_mode_lossless_tiles_through_the_native_reader(codec):
    """`bench.py --mode ingest --ingest-codec deflate | lzw`: a generic tiled TIFF (deflate tiles; LZW tiles with the horizontal predictor) goes through
    libcerberus_host.so's one-call-per-window reader (pread + decode + predictor + placement on pthreads) -> SlabUploader -> WSIRunner; the leg asserts that
    the decoded pixels ARE the source's, that they do not depend on the thread count, and that every file-fed run writes the resident run's canvases."""
    line = _bench([sys.executable, "bench.py", "--mode", "ingest", "--slide", "2048", "--streams", "1", "--ingest-codec", codec], timeout=900)
    ing = line["ingest"]
    assert line["config"]["tile_codec"] == codec and "libcerberus_host.so" in ing["file"]["format"] and ing["file"]["tiles"] == 64
    assert len(ing["decode"]["sweep"]) >= 3 and all("threads" in p_ and p_["Mpx_s"] > 10 for p_ in ing["decode"]["sweep"])
    assert all(e["decode_processes"] == 0 and not e["reduced_on_device"] for e in ing["end_to_end_from_file"])
    assert ing["best"]["of_resident"] > 0.3 and line["value"] == ing["best"]["Mpx_s"]
