"""IP-ERODED-3 / -11 (two-class INST heads, PostProcInstErodedMap) without a GPU: the test-side restatement against the reference's own label maps
(tests/golden/pp_eroded.npz, written by tests/tools/gen_golden_eroded.py), the new export's declaration and binding, the tile driver's codes, the
mirror class's assertions and the slide driver's refusal."""
import os
import re
import types

import numpy as np
import pytest

import eroded_ref
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "pp_eroded.npz"))


def test_restatement_equals_every_reference_label_map(gold):
    names = [str(x) for x in gold["names"]]
    assert len(names) >= 22 and {str(gold["tissue/" + n]) for n in names} == {"Nuclei", "Gland", "Lumen"}
    for name, tissue, m, want in eroded_ref.cases(gold):
        got = eroded_ref.proc(m, tissue)
        assert got.dtype == np.float64 and got.shape == want.shape, name
        assert np.array_equal(got, want), (name, int((got != want).sum()))
    # what the hand-made cases are there for
    out = {n: gold["out/" + n] for n in names}
    assert out["nuc_7_and_8"].max() == 5 and out["gland_1499_1500"].max() == 1 and out["lumen_149_150"].max() == 1   # min_size keeps area >= min_size
    assert out["nuc_all_fg"].max() == 0                                                                              # no background pixel: the reference's id list is empty
    # the pad rule: at 21 px from the edges no side of the box is padded and the dilation stops at the box; at 23 px all four are
    d21, d23 = out["gland_pad21"], out["gland_pad23"]
    assert not d21[20].any() and not d21[:, 20].any() and d23[22 - 4:23].any() and d23[:, 22 - 4:23].any()


def test_export_is_declared_and_bound():
    from cerberus_amd import _lib

    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cerberus_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+cerb_postproc_eroded\s*\(([^;]*?)\)\s*;", txt, flags=re.S)
    assert m, "include/cerberus_hip.h does not declare cerb_postproc_eroded"
    assert m.group(1).count(",") + 1 == 11
    assert "cerb_postproc_eroded" in _lib.EXPORTS
    at = _lib.lib().cerb_postproc_eroded.argtypes
    assert at is not None and len(at) == 11


def test_tile_driver_knows_the_four_codes():
    from cerberus_amd import tile

    assert set(tile.POSTPROC_CODES) == {"IP-ERODED-CONTOUR-3", "IP-ERODED-CONTOUR-11", "IP-ERODED-3", "IP-ERODED-11"}


def test_mirror_class_assertions_fire_before_any_device_work():
    from cerberus_amd.postproc import PostProcInstErodedMap

    raw = np.zeros((8, 8, 1), np.float32)
    with pytest.raises(AssertionError):
        PostProcInstErodedMap.post_process(raw, {"Nuclei-INST": [0, 1]}, "Stroma")
    with pytest.raises(AssertionError):
        PostProcInstErodedMap.post_process(raw, {"Gland-INST": [0, 1]}, "Nuclei")  # no Nuclei-INST key


def test_slide_driver_refuses_the_eroded_codes_by_name():
    from cerberus_amd import wsi

    with pytest.raises(NotImplementedError, match="IP-ERODED-3"):
        wsi.refuse_eroded_codes({"Gland-INST": "IP-ERODED-CONTOUR-11", "Nuclei-INST": "IP-ERODED-3"})
    with pytest.raises(NotImplementedError, match="IP-ERODED-11"):
        wsi.refuse_eroded_codes({"Gland-INST": "IP-ERODED-11"})
    wsi.refuse_eroded_codes({"Gland-INST": "IP-ERODED-CONTOUR-11", "Nuclei-INST": "IP-ERODED-CONTOUR-3", "Nuclei-TYPE": "TP"})
    # WSIRunner: a two-class INST head is refused before a canvas (or anything else on the device) is made
    net = types.SimpleNamespace(_decoders=[("Gland", "INST", 3, "Gland-INST"), ("Nuclei", "INST", 2, "Nuclei-INST")])
    with pytest.raises(NotImplementedError, match="Nuclei-INST.*IP-ERODED-3"):
        wsi.WSIRunner(net, (512, 512))
    # the command line says it before it loads a model: settings.yml's req_target_code is checked first
    src = open(os.path.join(ROOT, "run_infer_wsi.py")).read()
    assert src.index("refuse_eroded_codes(decoders)") < src.index("manager = InferManager(")
