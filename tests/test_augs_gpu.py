"""cerberus_amd.augs on the GPU against the independent restatement tests/augs_ref.py (written from include/cerberus_hip.h): every comparison is exact
equality, except Gaussian noise, whose ln / cos / sin come from two math libraries -- there equality is demanded wherever the restatement's pre-floor
value lies at least 1e-6 from an integer, |difference| <= 1 elsewhere, and the excluded share (computed from the restatement alone) is capped at 0.1 %."""
import os
from collections import OrderedDict

import numpy as np
import pytest
import torch

import augs_cases
import augs_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


def _np(t):
    return t.cpu().numpy()


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _arrays(seed, n, H, W, c, id_max=1000):
    rng = np.random.RandomState(seed)
    return rng.randint(0, 256, (n, H, W, 3)).astype(np.uint8), rng.randint(0, id_max, (n, H, W, c)).astype(np.int32)


def _check_warp(img, ann, maps, out_hw, numpy_input=False):
    from cerberus_amd import augs

    gi, ga = augs.warp_crop(img if numpy_input else _cuda(img), ann if numpy_input else _cuda(ann), maps, out_hw)
    assert gi.is_cuda and gi.dtype == torch.uint8 and gi.is_contiguous() and tuple(gi.shape) == (img.shape[0],) + tuple(out_hw) + (3,)
    assert ga.is_cuda and ga.dtype == torch.int32 and ga.is_contiguous() and tuple(ga.shape) == (ann.shape[0],) + tuple(out_hw) + (ann.shape[3],)
    assert np.array_equal(_np(gi), R.warp(img, maps, out_hw)) and np.array_equal(_np(ga), R.warp(ann, maps, out_hw))
    return _np(gi), _np(ga)


# ---- warp -------------------------------------------------------------------------------------------------------------------------------------------
def test_warp_identity_is_the_centre_crop_and_flips_are_np_flip():
    src, out = (37, 45), (24, 28)
    img, ann = _arrays(1, 3, 37, 45, 2)
    maps = [R.compose_map(src, out), R.compose_map(src, out, fliplr=True), R.compose_map(src, out, flipud=True)]
    gi, ga = _check_warp(img, ann, maps, out)
    oy, ox = (37 - 24) // 2, (45 - 28) // 2
    for got, a in ((gi, img), (ga, ann)):
        crop = a[:, oy:oy + 24, ox:ox + 28]
        assert np.array_equal(got[0], crop[0]) and np.array_equal(got[1], np.flip(crop[1], 1)) and np.array_equal(got[2], np.flip(crop[2], 0))


def test_warp_tiles_cross_64_pixel_boundaries():
    src, out = (130, 70), (100, 66)
    img, ann = _arrays(2, 2, 130, 70, 3)
    maps = [R.compose_map(src, out, (1.1, 0.9), 3.0, (0.6, -1.2), 31.0, True, False), R.compose_map(src, out, (0.85, 1.15), -4.0, (-1.0, 0.4), -140.0, False, True)]
    _check_warp(img, ann, maps, out, numpy_input=True)


def test_warp_eight_channels_and_one_channel():
    for c in (8, 1):
        img, ann = _arrays(3 + c, 2, 20, 22, c)
        _check_warp(img, ann, [R.compose_map((20, 22), (16, 16), rotate_deg=17.0), R.compose_map((20, 22), (16, 16), (1.2, 0.8), fliplr=True)], (16, 16))


def test_warp_rot90_of_a_square_source_is_np_rot90():
    img, ann = _arrays(4, 2, 33, 33, 2)
    gi, ga = _check_warp(img, ann, [R.compose_map((33, 33), (33, 33), rotate_deg=90.0), R.compose_map((33, 33), (33, 33), rotate_deg=-90.0)], (33, 33))
    for got, a in ((gi, img), (ga, ann)):
        assert np.array_equal(got[0], np.rot90(a[0], 3)) and np.array_equal(got[1], np.rot90(a[1], 1))


def test_warp_eight_random_affine_draws():
    from cerberus_amd import augs

    src, out = (37, 45), (24, 28)
    p = augs.sample_params(8, src, out, np.random.RandomState(17))
    maps = [R.compose_map(src, out, p["scale"][i], p["shear"][i], p["translate"][i], p["rotate"][i], p["fliplr"][i], p["flipud"][i]) for i in range(8)]
    assert p["map"].tolist() == maps
    img, ann = _arrays(5, 8, 37, 45, 2)
    _check_warp(img, ann, maps, out)


def test_warp_outside_the_source_is_zero():
    src, out = (37, 45), (24, 28)
    img, ann = _arrays(6, 1, 37, 45, 2, id_max=50)
    img, ann = np.maximum(img, 1), np.maximum(ann, 1)  # no zero inside the source
    gi, ga = _check_warp(img, ann, [R.compose_map(src, out, translate=(20.0, -9.0))], out)
    # out[v][u] = src[v + oy + 9][u + ox - 20]: columns u < 20 - ox and rows v >= 37 - 9 - oy lie outside
    oy, ox = (37 - 24) // 2, (45 - 28) // 2
    outside = np.zeros(out, bool)
    outside[:, :20 - ox] = True
    outside[37 - 9 - oy:, :] = True
    assert outside.any() and not outside.all()
    assert not gi[0][outside].any() and not ga[0][outside].any() and gi[0][~outside].all() and ga[0][~outside].all()
    assert np.array_equal(gi[0, :37 - 9 - oy, 20 - ox:], img[0, oy + 9:, :ox + 28 - 20])  # the rest is the source, shifted


def test_warp_keeps_ids_up_to_int32_max():
    img, ann = _arrays(7, 1, 12, 14, 2)
    ann[0, ::2] = 2 ** 31 - 1
    ann[0, 1::2, ::3] = 2 ** 31 - 2
    _, ga = _check_warp(img, ann, [R.compose_map((12, 14), (12, 14), fliplr=True)], (12, 14))
    assert int(ga.max()) == 2 ** 31 - 1 and np.array_equal(ga[0], ann[0, :, ::-1])


def test_refusals_side_above_16384_and_equal_pointers():
    """An error and no launch: the destination keeps its bytes."""
    from cerberus_amd import _lib, augs

    L = _lib.lib()
    with pytest.raises(_lib.CerberusHipError):
        augs.warp_crop(torch.zeros((1, 16385, 1, 3), dtype=torch.uint8, device="cuda"), None, [R.compose_map((16385, 1), (4, 1))], (4, 1))
    with pytest.raises(_lib.CerberusHipError):
        augs.gaussian_blur(torch.zeros((1, 1, 16385, 3), dtype=torch.uint8, device="cuda"), 3, 3)
    img = _cuda(_arrays(8, 2, 9, 11, 1)[0])
    keep = img.clone()
    maps = _cuda(np.array([R.compose_map((9, 11), (9, 11), fliplr=True)] * 2, np.int64))
    k = _cuda(np.array([3, 3], np.int32))
    one = torch.zeros((1, 16385, 1, 3), dtype=torch.uint8, device="cuda")
    dst = torch.full((1, 4, 1, 3), 7, dtype=torch.uint8, device="cuda")
    assert L.cerb_aug_warp(one.data_ptr(), None, 1, 16385, 1, 0, maps.data_ptr(), dst.data_ptr(), None, 4, 1, None) != 0
    assert b"16384" in L.cerb_last_error()
    assert L.cerb_aug_warp(img.data_ptr(), None, 2, 9, 11, 0, maps.data_ptr(), img.data_ptr(), None, 9, 11, None) != 0
    assert b"overlap" in L.cerb_last_error()
    assert L.cerb_aug_gaussian_blur(img.data_ptr(), img.data_ptr(), 2, 9, 11, k.data_ptr(), k.data_ptr(), None) != 0
    assert L.cerb_aug_median_blur(img.data_ptr(), img.data_ptr(), 2, 9, 11, k.data_ptr(), None) != 0
    assert L.cerb_aug_median_blur(one.data_ptr(), dst.data_ptr(), 1, 16385, 1, k.data_ptr(), None) != 0
    torch.cuda.synchronize()
    assert torch.equal(img, keep) and bool((dst == 7).all())


# ---- blurs ------------------------------------------------------------------------------------------------------------------------------------------
PAIRS = [(kx, ky) for kx in (1, 3, 5) for ky in (1, 3, 5)]


@pytest.mark.parametrize("hw", [(19, 23), (1, 2), (2, 1)])
def test_gaussian_blur_all_nine_size_pairs_in_one_batch(hw):
    """Mixed per-sample sizes in one launch; 1 x 2 and 2 x 1 are smaller than the radius (every tap is a replicated border)."""
    from cerberus_amd import augs

    img = np.random.RandomState(31).randint(0, 256, (9,) + hw + (3,)).astype(np.uint8)
    kx, ky = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    got = _np(augs.gaussian_blur(_cuda(img), kx, ky))
    assert np.array_equal(got, R.gaussian_blur(img, kx, ky))
    assert np.array_equal(got[0], img[0])  # (1, 1) is a copy


@pytest.mark.parametrize("hw", [(19, 23), (1, 2), (2, 1)])
def test_median_blur_all_sizes_in_one_batch(hw):
    from cerberus_amd import augs

    img = np.random.RandomState(32).randint(0, 256, (3,) + hw + (3,)).astype(np.uint8)
    got = _np(augs.median_blur(_cuda(img), [1, 3, 5]))
    assert np.array_equal(got, R.median_blur(img, [1, 3, 5]))
    assert np.array_equal(got[0], img[0])  # k = 1 is a copy


def test_blurs_keep_a_constant_image_constant():
    from cerberus_amd import augs

    img = np.empty((9, 7, 6, 3), np.uint8)
    img[...] = np.array([255, 1, 128], np.uint8)
    assert np.array_equal(_np(augs.gaussian_blur(_cuda(img), [p[0] for p in PAIRS], [p[1] for p in PAIRS])), img)
    assert np.array_equal(_np(augs.median_blur(_cuda(img[:3]), [1, 3, 5])), img[:3])


def test_blur_sizes_outside_1_3_5_are_refused_on_the_host():
    from cerberus_amd import augs

    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device="cuda")
    for bad in (0, 2, 7):
        with pytest.raises(ValueError):
            augs.gaussian_blur(img, bad, 3)
        with pytest.raises(ValueError):
            augs.median_blur(img, bad)


# ---- noise ------------------------------------------------------------------------------------------------------------------------------------------
def _check_noise(img, sigma, pc, key):
    from cerberus_amd import augs

    got = _np(augs.gaussian_noise(_cuda(img), sigma, pc, key)).astype(np.int64)
    want, pre = R.gaussian_noise(img, sigma, pc, key)
    loose = augs_cases.noise_excluded(pre)
    share = float(loose.mean())
    diff = np.abs(got - want.astype(np.int64))
    print("noise: excluded share %.3e, pixels differing inside it %d" % (share, int((diff[loose] != 0).sum())))
    assert share <= 1e-3
    assert not diff[~loose].any() and (diff[loose] <= 1).all()
    return got


def test_noise_against_the_restatement():
    img, sigma, pc, key = augs_cases.noise_case()  # 33 x 31, N = 4 (an odd pixel count: the byte path)
    got = _check_noise(img, sigma, pc, key)
    assert (got != img).mean() > 0.3
    # shared mode: equal offsets on the three channels wherever nothing clips (the integer offset floor(p + s z + 0.5) - p does not depend on p)
    for i in np.flatnonzero(pc == 0):
        off = got[i] - img[i].astype(np.int64)
        free = ((got[i] > 0) & (got[i] < 255)).all(-1)
        assert free.sum() > 500 and (off[free] == off[free][:, :1]).all()
    for i in np.flatnonzero(pc != 0):
        off = got[i] - img[i].astype(np.int64)
        assert (off[..., 0] != off[..., 1]).mean() > 0.3


def test_noise_on_the_dword_path():
    img = np.random.RandomState(41).randint(0, 256, (2, 32, 32, 3)).astype(np.uint8)  # 1024 pixels per sample: 4-byte aligned samples
    _check_noise(img, np.array([8.0, 2.5]), np.array([1, 0], np.int32), np.array([99, 2 ** 40 + 5], np.uint64))


def test_noise_sigma_zero_copies_same_key_repeats_other_key_differs():
    from cerberus_amd import augs

    img, sigma, pc, key = augs_cases.noise_case()
    dev = _cuda(img)
    assert torch.equal(augs.gaussian_noise(dev, 0.0, pc, key), dev)
    assert torch.equal(augs.gaussian_noise(dev, [np.nan, 0.0, np.nan, 0.0], pc, key), dev)  # NaN: the sample is copied
    a, b = augs.gaussian_noise(dev, sigma, pc, key), augs.gaussian_noise(dev, sigma, pc, key)
    assert torch.equal(a, b)
    c = augs.gaussian_noise(dev, sigma, pc, key + np.uint64(1))
    for i in range(4):
        assert float((a[i] != c[i]).float().mean()) > 0.3
    # the same key on two samples gives the same noise field
    same = np.array([5, 5, 5, 5], np.uint64)
    flat = np.full_like(img, 128)
    d = _np(augs.gaussian_noise(_cuda(flat), 6.0, 1, same))
    assert np.array_equal(d[0], d[1]) and np.array_equal(d[0], d[3])


# ---- colour -----------------------------------------------------------------------------------------------------------------------------------------
def _strips():
    """the 4695 test pixels as one row (an odd count: the byte path, with a tail) and, one pixel added, as 8 x 587 (the dword path)"""
    px = augs_cases.colour_pixels()
    assert px.shape == (1, 1, 343 + 256 + 4096, 3)
    more = np.concatenate([px, px[:, :, :1]], 2).reshape(1, 8, 587, 3)
    return [px, more]


def _values(lo, hi, seed):
    return np.concatenate([[lo, hi, 0.0], np.random.RandomState(seed).uniform(lo, hi, 3), [np.nan]])


@pytest.mark.parametrize("name,lo,hi", [("brightness", -26.0, 26.0), ("saturation", -0.2, 0.2), ("hue", -8.0, 8.0), ("contrast", 0.75, 1.25)])
def test_colour_operation_against_the_restatement(name, lo, hi):
    """Both range ends, 0, three random values and a NaN (that sample is skipped) in one batch of seven, on both memory paths."""
    from cerberus_amd import augs

    vals = _values(lo, hi, 50 + len(name))
    for strip in _strips():
        img = np.repeat(strip, len(vals), 0)
        if name == "contrast":
            assert torch.equal(augs.add_to_contrast(_cuda(img), vals), _cuda(img))  # the default: the reference's function returns its input
            got = _np(augs.add_to_contrast(_cuda(img), vals, apply_contrast=True))
        else:
            got = _np(getattr(augs, "add_to_" + name)(_cuda(img), vals))
        want = getattr(R, name)(img, vals)
        assert np.array_equal(got, want), name
        assert np.array_equal(got[-1], img[-1])  # NaN skips the sample
        assert (got[0] != img[0]).any()


def test_hue_greys_shift_180_and_negative_wrap():
    from cerberus_amd import augs

    px = augs_cases.colour_pixels()
    greys = np.ascontiguousarray(px[:, :, 343:343 + 256])
    assert np.array_equal(_np(augs.add_to_hue(_cuda(greys), 5.5)), greys)
    img = np.repeat(px, 4, 0)
    got = _np(augs.add_to_hue(_cuda(img), [0.0, 180.0, -8.0, 172.0]))
    assert np.array_equal(got[0], got[1])  # a shift of 180 is a shift of 0
    assert np.array_equal(got[2], got[3]) and not np.array_equal(got[2], got[0])  # a negative shift wraps
    assert np.array_equal(got, R.hue(img, [0.0, 180.0, -8.0, 172.0]))
    # fractional negative shifts and shifts beyond one turn, against the restatement
    vals = [-0.5, -179.75, 359.5, -361.25]
    assert np.array_equal(_np(augs.add_to_hue(_cuda(img), vals)), R.hue(img, vals))


@pytest.mark.parametrize("hw", [(61, 67), (64, 66)])
def test_channel_sums_and_contrast_on_an_image_batch(hw):
    from cerberus_amd import augs

    rng = np.random.RandomState(61)
    img = rng.randint(0, 256, (5,) + hw + (3,)).astype(np.uint8)
    img[1] = 255  # the largest sums
    img[2] = 0
    img[3, :, :, 1] //= 4  # unequal channel means
    sums = augs.channel_sums(_cuda(img))
    assert sums.dtype == torch.int64 and np.array_equal(_np(sums), img.astype(np.int64).sum((1, 2)))
    vals = [0.75, 1.25, 0.9, 1.2499, np.nan]
    assert np.array_equal(_np(augs.add_to_contrast(_cuda(img), vals, apply_contrast=True)), R.contrast(img, vals))


# ---- pipeline ---------------------------------------------------------------------------------------------------------------------------------------
def _sequence(img, ann, p, out_hw, apply_contrast):
    """the single operations, sample by sample, in augment_batch's documented order"""
    from cerberus_amd import augs

    imgs, anns = [], []
    for i in range(img.shape[0]):
        x, a = augs.warp_crop(img[i:i + 1], ann[i:i + 1], p["map"][i:i + 1], out_hw)
        if p["gauss_k"][i].any():
            x = augs.gaussian_blur(x, int(p["gauss_k"][i, 0]), int(p["gauss_k"][i, 1]))
        elif p["median_k"][i]:
            x = augs.median_blur(x, int(p["median_k"][i]))
        elif np.isfinite(p["noise_sigma"][i]):
            x = augs.gaussian_noise(x, p["noise_sigma"][i], p["noise_per_channel"][i], p["noise_key"][i])
        for op in p["colour_order"][i]:
            name = augs.COLOUR_OPS[op]
            if name == "contrast":
                x = augs.add_to_contrast(x, p[name][i], apply_contrast=apply_contrast)
            else:
                x = getattr(augs, "add_to_" + name)(x, p[name][i])
        imgs.append(x)
        anns.append(a)
    return torch.cat(imgs), torch.cat(anns)


def _mixed_params(src, out):
    from cerberus_amd import augs

    nan = np.nan
    return augs.sample_params(
        6, src, out, None, policy=None, scale=[[1.1, 0.9]] * 6, rotate=[10.0, -75.0, 0.0, 179.0, 33.0, -120.0], shear=[0.0, 4.0, -5.0, 0.0, 2.0, 1.0],
        fliplr=[True, False, True, False, False, True], flipud=[False, False, True, True, False, False],
        gauss_k=[[3, 5], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0]], median_k=[0, 5, 0, 0, 0, 3], noise_sigma=[nan, nan, 9.5, nan, 4.0, nan],
        noise_per_channel=[0, 0, 1, 0, 0, 0], noise_key=[0, 0, 77, 0, 2 ** 50 + 3, 0],
        colour_order=[[0, 1, 2, 3], [3, 2, 1, 0], [1, 3, 0, 2], [2, 0, 3, 1], [0, 1, 2, 3], [3, 0, 1, 2]],
        hue=[7.5, -8.0, nan, 3.0, 0.0, -2.5], saturation=[0.2, nan, -0.2, 0.05, nan, 0.1], brightness=[-26.0, 26.0, 5.5, nan, nan, -3.0],
        contrast=[0.75, 1.25, 1.1, 0.9, nan, 0.8])


@pytest.mark.parametrize("apply_contrast", [False, True])
@pytest.mark.parametrize("src,out", [((40, 44), (32, 36)), ((37, 45), (23, 29))])
def test_augment_batch_equals_the_single_operations_in_sequence(src, out, apply_contrast):
    """Bit for bit, with mixed per-sample choices (Gaussian / median / noise / none, different colour orders, skipped operations), on a geometry whose
    samples are 4-byte aligned and on one whose samples are not; then with eight draws of the default policy."""
    from cerberus_amd import augs

    img, ann = _arrays(71, 6, src[0], src[1], 5)
    p = _mixed_params(src, out)
    gi, ga = augs.augment_batch(_cuda(img), _cuda(ann), p, out, apply_contrast=apply_contrast)
    assert gi.is_cuda and gi.is_contiguous() and gi.dtype == torch.uint8 and tuple(gi.shape) == (6,) + out + (3,)
    assert ga.is_cuda and ga.is_contiguous() and ga.dtype == torch.int32 and tuple(ga.shape) == (6,) + out + (5,)
    si, sa = _sequence(_cuda(img), _cuda(ann), p, out, apply_contrast)
    assert torch.equal(gi, si) and torch.equal(ga, sa)
    ni, na = augs.augment_batch(img, ann, p, out, apply_contrast=apply_contrast)  # numpy inputs are uploaded
    assert torch.equal(ni, gi) and torch.equal(na, ga)
    assert np.array_equal(_np(ga), R.warp(ann, p["map"], out))
    if not apply_contrast:  # the default leaves the contrast step out: the same as NaN contrast values
        q = dict(p, contrast=np.full(6, np.nan))
        assert torch.equal(augs.augment_batch(_cuda(img), _cuda(ann), q, out, apply_contrast=True)[0], gi)
    img8, ann8 = _arrays(72, 8, src[0], src[1], 2)
    p8 = augs.sample_params(8, src, out, np.random.RandomState(4))
    gi8, ga8 = augs.augment_batch(_cuda(img8), _cuda(ann8), p8, out, apply_contrast=apply_contrast)
    si8, sa8 = _sequence(_cuda(img8), _cuda(ann8), p8, out, apply_contrast)
    assert torch.equal(gi8, si8) and torch.equal(ga8, sa8)


CHANNEL = ["Lumen-INST", "Gland-INST", "Nuclei-INST", "Nuclei-TYPE", "Gland-TYPE"]
C2T = OrderedDict([("Lumen-INST", "IP-ERODED-CONTOUR-3"), ("Gland-INST", "IP-ERODED-CONTOUR-11"), ("Nuclei-INST", "IP-ERODED-CONTOUR-3"),
                   ("Nuclei-TYPE", "TP"), ("Gland-TYPE", "TP")])


def _annotated_batch(seed, n, side):
    """n tiles with a few discs per instance channel and a class per instance in the matching type channel"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[:side, :side]
    ann = np.zeros((n, side, side, 5), np.int32)
    for i in range(n):
        for ch, count, rad, tch in ((0, 3, 9, None), (1, 4, 12, 4), (2, 12, 4, 3)):
            for k in range(count):
                cy, cx = rng.randint(0, side, 2)
                disc = (yy - cy) ** 2 + (xx - cx) ** 2 <= rad * rad
                ann[i, :, :, ch][disc] = k + 1
                if tch is not None:
                    ann[i, :, :, tch][disc] = 1 + k % 2
    img = rng.randint(0, 256, (n, side, side, 3)).astype(np.uint8)
    return img, ann


def test_targets_of_the_device_output_equal_targets_of_its_host_copy():
    from cerberus_amd import augs
    from cerberus_amd.targets import gen_targets_batch

    img, ann = _annotated_batch(81, 3, 80)
    p = augs.sample_params(3, (80, 80), (64, 64), np.random.RandomState(8))
    _, ann_aug = augs.augment_batch(img, ann, p, (64, 64))
    a = gen_targets_batch(ann_aug, CHANNEL, C2T, (64, 64))
    b = gen_targets_batch(_np(ann_aug), CHANNEL, C2T, (64, 64))
    assert list(a) == list(b)
    for k in a:
        if k == "dummy_target":
            assert np.array_equal(a[k], b[k])
        else:
            assert torch.equal(a[k], b[k]), k
    assert int(a["Nuclei-INST"].max()) > 0


def test_train_batch_feeds_train_step():
    """train_batch returns what train_step takes ('img', 'dummy_target', every head and weight map, CUDA tensors) and one step on the smallest
    geometry of the training tests (64 x 64, N = 3) returns finite losses."""
    from cerberus_amd import augs
    from cerberus_amd.losses import PARAMSET_LOSS
    from cerberus_amd.net_desc import create_model
    from cerberus_amd.train import Adam, train_step
    from cerberus_amd.weights import default_model_kwargs, make_state_dict

    img, ann = _annotated_batch(82, 3, 80)
    batch = augs.train_batch(img, ann, CHANNEL, C2T, (64, 64), (64, 64), np.random.RandomState(12))
    want = {"img", "dummy_target"} | set(C2T) | {h + "#WEIGHT-MAP" for h, c in C2T.items() if c.startswith("IP-ERODED")}
    assert set(batch) == want
    assert batch["img"].is_cuda and batch["img"].dtype == torch.uint8 and tuple(batch["img"].shape) == (3, 64, 64, 3) and batch["img"].is_contiguous()
    assert all(v.is_cuda and tuple(v.shape) == (3, 64, 64, 1) for k, v in batch.items() if k not in ("img", "dummy_target"))
    again = augs.train_batch(img, ann, CHANNEL, C2T, (64, 64), (64, 64), np.random.RandomState(12))
    assert all(torch.equal(batch[k], again[k]) for k in batch if k != "dummy_target")  # same seed, same batch
    tasks = ["Lumen", "Gland", "Nuclei", "Nuclei#TYPE", "Gland#TYPE"]
    seed = int(np.load(os.path.join(GOLDEN, "train_loss.npz"))["weight_seed"])
    m = create_model(**default_model_kwargs(considered_tasks=tasks))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in make_state_dict(seed, considered_tasks=tasks).items()}, strict=True)
    res = train_step(batch, ({"net": {"desc": m, "optimizer": Adam(lr=1.0e-3), "extra_info": {"loss": PARAMSET_LOSS}}}, None))
    losses = res["EMA"]
    assert {h + "_loss" for h in C2T} | {"overall_loss"} <= set(losses)
    assert all(np.isfinite(v) for v in losses.values()) and losses["overall_loss"] > 0, losses
    assert res["raw"]["img"].dtype == np.uint8 and res["raw"]["img"].shape == (2, 64, 64, 3)
