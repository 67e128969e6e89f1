"""cerberus_amd.targets: what needs no device -- the structuring element, argument validation, the fixture generator, and that targets.hip
builds for gfx950 without a GPU and defines every cerb_target_* entry the header declares."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT


def test_structuring_element_equals_the_documented_opencv_elements():
    """3 x 3 and 5 x 5 against the pins that do not come from this repository (tests/golden/cv2_documented.json); 11 x 11 follows the same
    documented row-span formula (OpenCV is not installed to pin it): 89 pixels, symmetric, and equal to the fixture generator's stand-in."""
    from cerberus_amd.targets import structuring_element
    from oracle import cv2_standin

    doc = json.load(open(os.path.join(GOLDEN, "cv2_documented.json")))
    assert np.array_equal(structuring_element(3), np.array(doc["getStructuringElement_MORPH_ELLIPSE_3x3"]["value"]))
    assert np.array_equal(structuring_element(5), np.array(doc["getStructuringElement_MORPH_ELLIPSE_5x5"]["value"]))
    assert int(structuring_element(3).sum()) == 5
    e11 = structuring_element(11)
    assert e11.shape == (11, 11) and e11.dtype == np.uint8 and int(e11.sum()) == 89
    assert np.array_equal(e11, e11[::-1]) and np.array_equal(e11, e11[:, ::-1]) and np.array_equal(e11, e11.T[::-1].T)
    for k in (3, 5, 7, 9, 11):
        assert np.array_equal(structuring_element(k), cv2_standin.getStructuringElement(cv2_standin.MORPH_ELLIPSE, (k, k))), k


def test_argument_validation_raises_by_name():
    from cerberus_amd.targets import TARGET_CODES, gen_targets, gen_targets_batch

    assert sorted(TARGET_CODES) == sorted(["IP", "IP-ERODED-3", "IP-ERODED-11", "IP-ERODED-CONTOUR-3", "IP-ERODED-CONTOUR-11", "NP", "TP", "PC"])
    ann = np.zeros((32, 40, 1), np.int32)
    with pytest.raises(KeyError, match="IP-ERODED-5"):
        gen_targets(ann, ["N"], {"N": "IP-ERODED-5"}, (16, 16), "seg")
    with pytest.raises(ValueError, match="crop_shape"):
        gen_targets(ann, ["N"], {"N": "IP"}, (33, 16), "seg")
    with pytest.raises(ValueError, match="crop_shape"):
        gen_targets_batch(ann[None], ["N"], {"N": "IP"}, (16, 41))
    with pytest.raises(TypeError, match="integers"):
        gen_targets(ann.astype(np.float32), ["N"], {"N": "IP"}, (16, 16), "seg")
    import torch

    with pytest.raises(TypeError, match="integers"):
        gen_targets_batch(torch.zeros((1, 32, 40, 1), dtype=torch.float64), ["N"], {"N": "IP"}, (16, 16))
    with pytest.raises(ValueError, match="dimensions"):
        gen_targets_batch(ann, ["N"], {"N": "IP"}, (16, 16))
    with pytest.raises(TypeError, match="CUDA tensor or a numpy array"):
        gen_targets([[0]], ["N"], {"N": "IP"}, (1, 1), "seg")


def test_reference_names_are_exported():
    import cerberus_amd

    assert "cerberus_amd.targets.gen_targets" in cerberus_amd.__doc__ and "loader/targets.py" in cerberus_amd.__doc__


def test_fixture_generator_reproduces_the_committed_fixture(tmp_path):
    """tests/tools/gen_golden_targets.py rerun against the reference checkout gives tests/golden/targets.npz again, array for array and bit for
    bit.  (The generator itself refuses to write unless its recomputed distance sums reproduce the reference's weight maps bit for bit.)"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    try:
        import gen_golden_targets as gen
    finally:
        sys.path.pop(0)
    if not os.path.exists(os.path.join(gen.REF, "loader", "targets.py")):
        pytest.skip("no reference checkout here (CERBERUS_REFERENCE)")
    out = str(tmp_path / "targets.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "gen_golden_targets.py"), "--out", out], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    a, b = np.load(out), np.load(os.path.join(GOLDEN, "targets.npz"))
    assert sorted(a.files) == sorted(b.files)
    for k in a.files:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k
    assert os.path.getsize(os.path.join(GOLDEN, "targets.npz")) < (1 << 20)


def test_fixture_holds_the_cases_the_feature_is_specified_on():
    g = np.load(os.path.join(GOLDEN, "targets.npz"))
    cases = [str(c) for c in g["cases"]]
    codes = {str(c) for n in cases for c in g[n + "/c2t_codes"]}
    assert codes == {"IP", "IP-ERODED-3", "IP-ERODED-11", "IP-ERODED-CONTOUR-3", "IP-ERODED-CONTOUR-11", "NP", "TP", "PC"}
    assert tuple(g["paramset_448/ann"].shape) == (448, 448, 6) and len(g["paramset_448/c2t_heads"]) == 6
    assert not g["empty/ann"].any() and len(np.unique(g["one_instance/ann"])) == 2
    assert float(g["one_instance/out/N#WEIGHT-MAP"].min()) == 1.0 == float(g["one_instance/out/N#WEIGHT-MAP"].max())
    assert int(g["sparse_ids/ann"].max()) == 1 << 20
    assert "" in [str(v) for v in g["multi_channel/has_flag"]]  # None flags of the absent head
    assert not bool(g["no_weight_map/gen_unet_weight_map"])
    t = g["touches_all_borders/ann"][..., 0]
    assert t[0].any() and t[-1].any() and t[:, 0].any() and t[:, -1].any()
    assert any(tuple(g[n + "/crop"]) != tuple(g[n + "/ann"].shape[:2]) for n in cases) and any(g[n + "/ann"].shape[0] % 2 for n in cases)


def test_targets_hip_builds_for_gfx950_and_defines_the_declared_entry_points(tmp_path):
    from cerberus_amd import build as b

    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc here")
    assert "targets.hip" in b.SOURCES
    obj = str(tmp_path / "targets.o")
    r = subprocess.run([hipcc] + b.FLAGS + b.EXTRA_FLAGS.get("targets.hip", []) + ["-c", os.path.join(b.CSRC, "targets.hip"), "-o", obj], capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "warning" not in r.stderr, r.stderr[-3000:]
    nm = subprocess.run(["nm", "--defined-only", obj], capture_output=True, text=True, check=True).stdout
    defined = set(re.findall(r"\b[TtWw]\s+(cerb_target_[a-z0-9_]+)\b", nm))
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cerberus_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(cerb_target_[a-z0-9_]+)\s*\(", txt))
    assert len(declared) == 6 and declared == defined, (sorted(declared), sorted(defined))
