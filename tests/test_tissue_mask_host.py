"""Host side of the tissue-mask generator (cerberus_amd/tissue.py; reference misc/utils.py:195-244): the two tables the kernels are fed and Otsu's
arithmetic on 256 counts, against tests/golden/tissue_mask.npz (the reference's own values, tests/tools/gen_golden_tissue_mask.py); the driver's
refusals of --auto_mask; the option table.  No GPU."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLDEN, "tissue_mask.npz"))


def test_stain_table_reproduces_the_reference_bytes(gold):
    from cerberus_amd import tissue

    t = tissue.stain_table()
    assert t.shape == (3, 256, 3) and t.dtype == np.float64
    assert np.array_equal(tissue.stain_bytes_host(gold["all_colours/sample_rgb"], t), gold["all_colours/sample_hed"])
    for nm in gold["images"]:
        assert np.array_equal(tissue.stain_bytes_host(gold[nm + "/img"], t), gold[nm + "/hed"]), nm
    # negative values and values of 256 and more are both among the sample: the wrap-around is exercised
    x = ((t[0][gold["all_colours/sample_rgb"][:, 0]] + t[1][gold["all_colours/sample_rgb"][:, 1]]) + t[2][gold["all_colours/sample_rgb"][:, 2]]) * 255.0
    assert (x < 0).any() and (x >= 256).any()


def test_otsu_on_the_stored_histograms_gives_the_stored_thresholds(gold):
    from cerberus_amd import tissue

    for nm in gold["images"]:
        ent = gold[nm + "/entropy"]
        lo, hi = float(ent.min()), float(ent.max())
        counts = gold[nm + "/counts"]
        assert np.array_equal(counts, np.histogram(ent.ravel(), bins=256, range=(lo, hi))[0]), nm
        thr = tissue.otsu_threshold(counts, lo, hi)
        assert thr == float(gold[nm + "/threshold"]), (nm, thr)
        assert np.array_equal(ent > thr, gold[nm + "/stain_entropy_otsu"]), nm


def test_entropy_term_table_reproduces_the_reference_entropy_of_the_smallest_image(gold):
    """The [pop][count] table, summed over the bins in ascending order and combined as (H + E) - D, is the reference's entropy map bit for bit (9 x 11:
    all but three pixels' footprints are cut by a border)."""
    from cerberus_amd import tissue

    t = tissue.entropy_term_table()
    assert t.shape == (50, 50) and t[49, 49] == 0.0 and t[7, 0] == 0.0 and t[4, 2] == -0.5
    hed = gold["img9x11/hed"]
    h, w = hed.shape[:2]
    disk = [(dy, dx) for dy in range(-4, 5) for dx in range(-4, 5) if dy * dy + dx * dx <= 16]
    assert len(disk) == 49
    ent = np.zeros((3, h, w))
    for s in range(3):
        for y in range(h):
            for x in range(w):
                vals = [int(hed[y + dy, x + dx, s]) for dy, dx in disk if 0 <= y + dy < h and 0 <= x + dx < w]
                assert len(vals) < 49 or (y == 4 and 4 <= x <= 6)
                e = 0.0
                for v, c in zip(*np.unique(vals, return_counts=True)):  # ascending bins
                    e -= t[len(vals), c]
                ent[s, y, x] = e
    assert np.array_equal((ent[0] + ent[1]) - ent[2], gold["img9x11/entropy"])


def test_auto_mask_is_refused_beside_msk_dir_and_for_synthetic_specs(tmp_path):
    import run_infer_wsi

    slides, masks = tmp_path / "slides", tmp_path / "masks"
    slides.mkdir()
    masks.mkdir()
    (slides / "s1.txt").write_text("synthetic:700x900:5")
    common = ["--synthetic", "--input_dir=%s" % slides, "--wsi_file_ext=.txt", "--output_dir=%s" % (tmp_path / "out")]
    with pytest.raises(ValueError, match="--auto_mask and --msk_dir"):
        run_infer_wsi.main(common + ["--auto_mask", "--msk_dir=%s" % masks])
    with pytest.raises(ValueError, match=r"s1\.txt is a synthetic slide spec"):
        run_infer_wsi.main(common + ["--auto_mask"])
    with pytest.raises(ValueError, match="--auto_mask_ds"):
        run_infer_wsi.main(common + ["--auto_mask", "--auto_mask_ds=0"])
    assert not (tmp_path / "out").exists()  # refused before anything was opened or written


def test_option_table_keeps_the_reference_flags_and_adds_two():
    from cerberus_amd.cli import WSI_OPTIONS, parse

    got = [(f, v, d) for f, v, d, _ in WSI_OPTIONS]
    old = [("--gpu", True, "0"), ("--model", True, None), ("--synthetic", False, False), ("--nr_inference_workers", True, "0"), ("--nr_post_proc_workers", True, "0"),
           ("--batch_size", True, "30"), ("--tile_shape", True, "2048"), ("--chunk_shape", True, "15000"), ("--ambiguous_size", True, "64"), ("--wsi_proc_mag", True, "0.5"),
           ("--wsi_file_ext", True, ".svs"), ("--cache_path", True, "cache/"), ("--logging_dir", True, "logging/"), ("--input_dir", True, None), ("--msk_dir", True, None),
           ("--output_dir", True, "output/"), ("--patch_input_shape", True, "448"), ("--patch_output_shape", True, "144"), ("--wsi_bulk_idx", True, "1"),
           ("--wsi_proc_step", True, "10"), ("--save_thumb", False, False), ("--save_mask", False, False), ("--save_label_maps", False, False),
           ("--reference_tiling", False, False), ("--jpeg_decode", True, "host")]
    assert got[:len(old)] == old
    assert got[len(old):] == [("--auto_mask", False, False), ("--auto_mask_ds", True, "16")]
    a = parse("run_infer_wsi.py", WSI_OPTIONS, ["--synthetic"])
    assert a["--auto_mask"] is False and a["--auto_mask_ds"] == "16" and a["--msk_dir"] is None
    b = parse("run_infer_wsi.py", WSI_OPTIONS, ["--auto_mask", "--auto_mask_ds=8"])
    assert b["--auto_mask"] is True and b["--auto_mask_ds"] == "8"
