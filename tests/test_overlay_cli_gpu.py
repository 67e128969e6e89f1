"""The overlay flags of the two drivers end to end: `run_infer_tile.py --overlay=device` against `--overlay=host` (same .mat files, a picture of
twice the source size) and `run_infer_wsi.py --save_overlay --overlay_ds=4` on a .png slide (a picture with the thumbnail's shape)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_run_infer_tile_overlay_device_writes_the_same_mats_and_a_picture_of_twice_the_size(tmp_path):
    import scipy.io as sio
    from PIL import Image

    inp = tmp_path / "in"
    inp.mkdir()
    rs = np.random.RandomState(3)
    sizes = (("a", (300, 421)), ("b", (256, 256)))  # the two images of tests/test_cli_gpu.py::test_run_infer_tile_cli
    for name, hw in sizes:
        Image.fromarray(rs.randint(0, 256, hw + (3,)).astype(np.uint8)).save(str(inp / (name + ".png")))
    outs = {}
    for mode in ("host", "device"):
        outs[mode] = tmp_path / ("out_" + mode)
        cmd = [sys.executable, os.path.join(ROOT, "run_infer_tile.py"), "--synthetic", "--input_dir=%s" % inp, "--output_dir=%s" % outs[mode], "--batch_size=8",
               "--patch_input_shape=256", "--patch_output_shape=256", "--overlay=%s" % mode]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
    n_inst = 0
    for name, hw in sizes:
        ov = np.array(Image.open(str(outs["device"] / "overlay" / (name + ".jpg"))))
        assert ov.shape == (2 * hw[0], 2 * hw[1], 3) and ov.shape == np.array(Image.open(str(outs["host"] / "overlay" / (name + ".jpg")))).shape
        for t in ("gland", "lumen", "nuclei", "pclass"):
            a, b = (sio.loadmat(str(outs[m] / ("%s_mat" % t) / (name + ".mat"))) for m in ("host", "device"))
            keys = sorted(k for k in a if not k.startswith("__"))
            assert keys == sorted(k for k in b if not k.startswith("__")) and keys
            for k in keys:
                assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), (name, t, k)
            n_inst += int(np.asarray(a.get("id", [])).size)
    assert n_inst > 0


def test_run_infer_wsi_save_overlay_writes_a_picture_with_the_thumbnail_shape(tmp_path):
    from PIL import Image

    from cerberus_amd import tissue
    from cerberus_amd.reader import WSIReader
    from cerberus_amd.wsi import synth_slide

    slides, out = tmp_path / "slides", tmp_path / "out"
    slides.mkdir()
    Image.fromarray(synth_slide(530, 610, seed=5).cpu().numpy()).save(str(slides / "s1.png"))
    cmd = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % slides, "--wsi_file_ext=.png", "--output_dir=%s" % out,
           "--logging_dir=%s" % (tmp_path / "log"), "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256", "--save_overlay", "--overlay_ds=4"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    thumb = tissue.thumbnail(WSIReader.open(input_img=str(slides / "s1.png")), 0.5, "mpp", 4)
    ov = np.array(Image.open(str(out / "overlay" / "s1.jpg")))
    assert ov.shape == thumb.shape and ov.dtype == np.uint8
    import joblib

    dat = joblib.load(str(out / "dat" / "s1.dat"))
    n_inst = sum(len(dat[t]) for t in ("Nuclei", "Gland", "Lumen"))
    print("instances drawn:", n_inst)
    if n_inst:  # strokes are on it: pixels far from the thumbnail's
        assert (np.abs(ov.astype(np.int32) - thumb.astype(np.int32)).max(axis=2) > 96).any()
