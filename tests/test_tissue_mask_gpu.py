"""The tissue-mask generator on the device (cerberus_amd/tissue.py: stain_entropy_otsu, morphology, get_tissue_mask; csrc/tissue_mask.hip and the
morphology entry at its end) against the reference's own values (misc/utils.py:195-244 through tests/tools/gen_golden_tissue_mask.py ->
tests/golden/tissue_mask.npz), and `run_infer_wsi.py --auto_mask` against the `--msk_dir` run on the mask it saved.

Entropy bound: a value is the sum of at most 49 table terms of magnitude <= 0.531 (max of -p log2 p), each added with about one ulp (1.1e-16) of
rounding, three such sums combined: below 1e-14.  1e-12 leaves two decades for a libm whose log differs from the fixture machine's in the last
bits (the table is filled on the host)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "tissue_mask.npz"))


@pytest.fixture(scope="module")
def device_parts(gold):
    """get_tissue_mask(img, return_parts=True) of every fixture image, computed once: name -> (mask numpy, parts)"""
    import torch

    from cerberus_amd import tissue

    out = {}
    for nm in gold["images"]:
        mask, parts = tissue.get_tissue_mask(torch.from_numpy(gold[nm + "/img"]).cuda(), return_parts=True)
        out[str(nm)] = (mask.cpu().numpy(), parts)
    return out


def test_stain_bytes_equal_the_reference_on_every_image(gold, device_parts):
    for nm, (_, parts) in device_parts.items():
        got = parts["planes"].permute(1, 2, 0).cpu().numpy()
        assert got.dtype == np.uint8 and np.array_equal(got, gold[nm + "/hed"]), nm


def test_stain_bytes_of_all_2_24_colours_match_the_reference_digest(gold):
    import torch

    from cerberus_amd import tissue

    i = torch.arange(1 << 24, device="cuda", dtype=torch.int32)
    img = torch.stack([(i >> 16) & 255, (i >> 8) & 255, i & 255], -1).to(torch.uint8).reshape(4096, 4096, 3)
    got = tissue.stain_planes(img).permute(1, 2, 0).contiguous().cpu().numpy()
    pick = np.random.RandomState(int(gold["seed"]) + 7).randint(0, 1 << 24, 4096)
    assert np.array_equal(img.reshape(-1, 3).cpu().numpy()[pick], gold["all_colours/sample_rgb"])
    bad = np.nonzero((got.reshape(-1, 3)[pick] != gold["all_colours/sample_hed"]).any(axis=1))[0]
    assert bad.size == 0, (gold["all_colours/sample_rgb"][bad[:5]], got.reshape(-1, 3)[pick][bad[:5]], gold["all_colours/sample_hed"][bad[:5]])
    assert hashlib.sha256(got.tobytes()).hexdigest() == str(gold["all_colours/sha256"])


def test_entropy_within_1e_12_of_the_reference_on_every_pixel(gold, device_parts):
    for nm, (_, parts) in device_parts.items():
        got = parts["entropy"].cpu().numpy()
        ref = gold[nm + "/entropy"]
        assert got.dtype == np.float64 and got.shape == ref.shape
        err = float(np.abs(got - ref).max())
        print(nm, "max |entropy - reference| = %.3e" % err)
        assert err <= 1e-12, (nm, err)
        assert parts["range"] == (float(got.min()), float(got.max())), nm  # the device's own minimum / maximum


def test_histogram_counts_and_otsu_threshold(gold, device_parts):
    for nm, (_, parts) in device_parts.items():
        ent = parts["entropy"].cpu().numpy()
        lo, hi = parts["range"]
        want = np.histogram(ent.ravel(), bins=256, range=(lo, hi))[0]
        assert parts["counts"].dtype == np.int64 and np.array_equal(parts["counts"], want), nm
        assert int(parts["counts"].sum()) == ent.size
        assert abs(parts["threshold"] - float(gold[nm + "/threshold"])) <= 1e-9, (nm, parts["threshold"], float(gold[nm + "/threshold"]))


def test_masks_equal_the_reference_exactly(gold, device_parts):
    import torch

    from cerberus_amd import tissue

    for nm, (mask, parts) in device_parts.items():
        assert np.array_equal(parts["otsu_mask"].cpu().numpy(), gold[nm + "/stain_entropy_otsu"]), nm
        assert mask.dtype == np.uint8 and np.array_equal(mask, gold[nm + "/get_tissue_mask"]), nm
    nm = str(gold["images"][0])
    m1 = tissue.stain_entropy_otsu(torch.from_numpy(gold[nm + "/img"]).cuda())
    assert m1.dtype == torch.bool and np.array_equal(m1.cpu().numpy(), gold[nm + "/stain_entropy_otsu"])


def test_morphology_equals_the_reference_on_every_hand_made_mask(gold):
    import torch

    from cerberus_amd import tissue

    for nm in gold["masks"]:
        got = tissue.morphology(torch.from_numpy(gold["mask/%s/in" % nm]).cuda())
        assert got.dtype == torch.bool
        want = gold["mask/%s/out" % nm]
        diff = got.cpu().numpy() != want
        assert not diff.any(), (str(nm), int(diff.sum()), np.argwhere(diff)[:5].tolist())


def test_row_strided_view_and_repeated_calls_give_the_same_bytes(gold):
    import torch

    from cerberus_amd import tissue

    img = gold["img131x197/img"]
    h, w = img.shape[:2]
    packed = torch.from_numpy(img).cuda()
    big = torch.full((h + 3, w + 7, 3), 77, dtype=torch.uint8, device="cuda")
    big[1:h + 1, 5:w + 5] = packed
    view = big[1:h + 1, 5:w + 5]
    assert view.stride(0) == (w + 7) * 3 and not view.is_contiguous()
    a, pa = tissue.get_tissue_mask(packed, return_parts=True)
    b, pb = tissue.get_tissue_mask(view, return_parts=True)
    c, pc = tissue.get_tissue_mask(packed, return_parts=True)
    for x, px in ((b, pb), (c, pc)):
        assert torch.equal(a, x) and torch.equal(pa["planes"], px["planes"]) and torch.equal(pa["otsu_mask"], px["otsu_mask"])
        assert pa["entropy"].cpu().numpy().tobytes() == px["entropy"].cpu().numpy().tobytes()
        assert pa["threshold"] == px["threshold"] and np.array_equal(pa["counts"], px["counts"])


def test_constant_image_raises_value_error():
    import torch

    from cerberus_amd import tissue

    with pytest.raises(ValueError, match="single entropy value"):
        tissue.get_tissue_mask(torch.full((64, 80, 3), 255, dtype=torch.uint8, device="cuda"))


def _slide(seed=11):
    """2048 x 3072: glass (238 with faint noise) and two elliptical tissue regions textured in 8 x 8-pixel cells of a 24-colour palette, so that the
    texture survives the x8 box means of the thumbnail; patch columns 10 and 11 (x >= 2560) hold glass only."""
    rs = np.random.RandomState(seed)
    img = (238 + rs.randint(-1, 2, (2048, 3072, 3))).astype(np.uint8)
    palette = np.stack([rs.randint(150, 231, 24), rs.randint(80, 181, 24), rs.randint(120, 221, 24)], -1).astype(np.uint8)
    tex = np.repeat(np.repeat(palette[rs.randint(0, 24, (256, 384))], 8, axis=0), 8, axis=1)
    yy, xx = np.mgrid[0:2048, 0:3072]
    for cy, cx, a, b in ((640, 800, 400, 560), (1520, 2000, 320, 480)):
        inside = ((yy - cy) / float(a)) ** 2 + ((xx - cx) / float(b)) ** 2 <= 1.0
        img[inside] = tex[inside]
    return img


def test_run_infer_wsi_auto_mask_equals_the_msk_dir_run_on_the_saved_mask(tmp_path):
    """Run A: --auto_mask --auto_mask_ds=8 --save_mask --save_label_maps.  Run B: --msk_dir = run A's mask/ output.  The saved mask is
    get_tissue_mask of the reader's thumbnail, patches without tissue did not run, and B's label maps and dictionary equal A's.  (The .dat keys are
    fresh uuid4 values in every run and an .npz carries zip time stamps, so the files are compared entry by entry and array by array: every value's
    bytes, in order.)"""
    import joblib
    import torch
    from PIL import Image

    from cerberus_amd import tissue
    from cerberus_amd.reader import WSIReader
    from cerberus_amd.wsi import SlideGeometry

    slides = tmp_path / "slides"
    slides.mkdir()
    np.save(str(slides / "s1.npy"), _slide())
    base = [sys.executable, os.path.join(ROOT, "run_infer_wsi.py"), "--synthetic", "--input_dir=%s" % slides, "--wsi_file_ext=.npy", "--batch_size=8",
            "--patch_input_shape=256", "--patch_output_shape=256", "--save_label_maps", "--save_mask"]
    out_a, out_b = tmp_path / "a", tmp_path / "b"
    r = subprocess.run(base + ["--output_dir=%s" % out_a, "--logging_dir=%s" % (tmp_path / "la"), "--auto_mask", "--auto_mask_ds=8"], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    saved = np.array(Image.open(str(out_a / "mask" / "s1.png")))
    thumb = tissue.thumbnail(WSIReader.open(input_img=str(slides / "s1.npy")), 0.5, "mpp", 8)
    assert thumb.shape == (256, 384, 3)
    mask = tissue.get_tissue_mask(torch.from_numpy(thumb).cuda()).cpu().numpy()
    assert np.array_equal(saved > 0, mask > 0) and 4000 < int(mask.sum()) < mask.size // 2
    sel = tissue.select_patches(mask, SlideGeometry((2048, 3072), 256, 256).out_boxes(), (2048, 3072)).reshape(8, 12)
    assert sel.any() and not sel[:, 10:].any()  # two patch columns were skipped
    za = np.load(str(out_a / "s1.npz"))
    assert za["Nuclei"].shape == (2048, 3072) and za["Nuclei"][:, 2560:].max() == 0 and za["type_Nuclei-TYPE"][:, 2560:].max() == 0 and za["pclass"][:, 640:].max() == 0
    assert "Gland_region0" in za.files and "Gland_region1" in za.files  # the two tissue regions
    r = subprocess.run(base + ["--output_dir=%s" % out_b, "--logging_dir=%s" % (tmp_path / "lb"), "--msk_dir=%s" % (out_a / "mask")], capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    zb = np.load(str(out_b / "s1.npz"))
    assert sorted(za.files) == sorted(zb.files)
    for k in za.files:
        assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), k
    da, db = joblib.load(str(out_a / "dat" / "s1.dat")), joblib.load(str(out_b / "dat" / "s1.dat"))
    assert list(da.keys()) == list(db.keys())
    for k in da:
        if k in ("proc_resolution", "base_resolution"):
            assert da[k] == db[k], k
        elif not isinstance(da[k], dict):
            assert np.array_equal(np.asarray(da[k]), np.asarray(db[k])), k
        else:  # uuid -> instance entry
            ea, eb = list(da[k].values()), list(db[k].values())
            assert len(ea) == len(eb), k
            for x, y in zip(ea, eb):
                assert sorted(x.keys()) == sorted(y.keys())
                for f in x:
                    assert np.asarray(x[f]).dtype == np.asarray(y[f]).dtype and np.asarray(x[f]).tobytes() == np.asarray(y[f]).tobytes(), (k, f)
    assert np.array_equal(np.array(Image.open(str(out_b / "mask" / "s1.png"))), saved)
