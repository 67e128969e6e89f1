"""`--overlay_encode=device` of the two drivers end to end, in the manner of tests/test_overlay_cli_gpu.py: the overlay the device drew is JPEG-encoded
there too, and the file opens to exactly the pixels of the file PIL wrote from the downloaded picture (equal coefficients make this exact); every other
output is byte-identical; the option is refused by name where no picture is on the device."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _run(cmd):
    return subprocess.run([sys.executable] + cmd, capture_output=True, text=True, timeout=300, cwd=ROOT)


def test_run_infer_tile_encodes_the_overlay_on_the_device_to_the_same_pixels(tmp_path):
    from PIL import Image

    inp = tmp_path / "in"
    inp.mkdir()
    Image.fromarray(np.random.RandomState(3).randint(0, 256, (256, 256, 3)).astype(np.uint8)).save(str(inp / "b.png"))
    outs = {}
    for mode in ("host", "device"):
        outs[mode] = tmp_path / ("out_" + mode)
        r = _run([os.path.join(ROOT, "run_infer_tile.py"), "--synthetic", "--input_dir=%s" % inp, "--output_dir=%s" % outs[mode], "--batch_size=8",
                  "--patch_input_shape=256", "--patch_output_shape=256", "--overlay=device", "--overlay_encode=%s" % mode])
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = (np.array(Image.open(str(outs[m] / "overlay" / "b.jpg"))) for m in ("host", "device"))
    assert a.shape == (512, 512, 3) and np.array_equal(a, b)
    assert b"\xff\xdd" in (outs["device"] / "overlay" / "b.jpg").read_bytes()[:700]  # (the device's file: it carries a DRI segment)
    n = 0
    for t in ("gland", "lumen", "nuclei", "pclass"):
        fa, fb = (outs[m] / ("%s_mat" % t) / "b.mat" for m in ("host", "device"))
        # (savemat stamps its header with the time of writing: the first 128 bytes are text, the data follow)
        assert fa.read_bytes()[128:] == fb.read_bytes()[128:], t
        n += 1
    assert n == 4


def test_run_infer_wsi_encodes_the_saved_overlay_on_the_device_to_the_same_pixels(tmp_path):
    from PIL import Image

    from cerberus_amd.wsi import synth_slide

    slides = tmp_path / "slides"
    slides.mkdir()
    Image.fromarray(synth_slide(530, 610, seed=5).cpu().numpy()).save(str(slides / "s1.png"))
    outs = {}
    for mode in ("host", "device"):
        outs[mode] = tmp_path / ("out_" + mode)
        r = _run([os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % slides, "--wsi_file_ext=.png", "--output_dir=%s" % outs[mode],
                  "--logging_dir=%s" % (tmp_path / ("log_" + mode)), "--batch_size=6", "--patch_input_shape=256", "--patch_output_shape=256", "--save_overlay",
                  "--overlay_ds=4", "--overlay_encode=%s" % mode])
        assert r.returncode == 0, r.stderr[-2000:]
    a, b = (np.array(Image.open(str(outs[m] / "overlay" / "s1.jpg"))) for m in ("host", "device"))
    assert a.ndim == 3 and a.shape[2] == 3 and min(a.shape[:2]) > 100 and np.array_equal(a, b)
    import joblib

    da, db = (joblib.load(str(outs[m] / "dat" / "s1.dat")) for m in ("host", "device"))
    assert sorted(da) == sorted(db)

    def canon(insts):  # (the dictionary's keys are fresh uuids in every run: the instances themselves are compared, in a fixed order)
        return sorted(tuple((f, v.tobytes() if isinstance(v, np.ndarray) else repr(v)) for f, v in sorted(d.items())) for d in insts.values())

    n = 0
    for t in ("Nuclei", "Gland", "Lumen"):
        assert canon(da[t]) == canon(db[t]), t
        n += len(da[t])
    print("instances:", n)


def test_the_option_is_refused_by_name_where_no_picture_is_on_the_device(tmp_path):
    (tmp_path / "in").mkdir()
    r = _run([os.path.join(ROOT, "run_infer_tile.py"), "--synthetic", "--input_dir=%s" % (tmp_path / "in"), "--output_dir=%s" % (tmp_path / "o"),
              "--overlay=host", "--overlay_encode=device"])
    assert r.returncode != 0 and "ValueError" in r.stderr and "--overlay_encode=device" in r.stderr and "--overlay=device" in r.stderr
    r = _run([os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % (tmp_path / "in"), "--output_dir=%s" % (tmp_path / "o"),
              "--overlay_encode=device"])
    assert r.returncode != 0 and "ValueError" in r.stderr and "--overlay_encode=device" in r.stderr and "--save_overlay" in r.stderr
    r = _run([os.path.join(ROOT, "run_infer_tile.py"), "--synthetic", "--input_dir=%s" % (tmp_path / "in"), "--overlay_encode=gpu"])
    assert r.returncode != 0 and "--overlay_encode takes host or device" in r.stderr
    assert not (tmp_path / "o").exists()
