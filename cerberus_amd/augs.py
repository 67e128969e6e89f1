"""Training augmentations on the device: the shape and input augmentations that sit in front of gen_targets in the model family's training pipeline
(the lambdas of the reference's loader/augs.py and the affine / flip / crop steps around them).

    sample_params(n, src_hw, out_hw, rng, policy=TRAIN_POLICY)              the host draws every random number: a dict of small numpy arrays
    augment_batch(img, ann, params, out_hw, apply_contrast=False)           -> (img_aug uint8 [N, h, w, 3], ann_aug int32 [N, h, w, C]), CUDA
    train_batch(img, ann, channel, channel_to_target, out_hw, crop_shape, rng, ...)   augment_batch + gen_targets_batch -> the dict train_step takes
    warp_crop / gaussian_blur / median_blur / gaussian_noise / add_to_hue / add_to_saturation / add_to_brightness / add_to_contrast / channel_sums
                                                                            the single operations over CUDA tensors

The host draws numbers, the device moves pixels: every kernel (csrc/augs.hip, cerb_aug_* of include/cerberus_hip.h) is a pure function of its input
and a few per-sample parameters, defined in integers and float64 in the header.  The definitions are this project's own; bit parity with OpenCV or
imgaug is not claimed.  There is no CPU path.

Contrast: the reference's add_to_contrast computes its result and then returns clip(img), i.e. its INPUT (loader/augs.py:71-78).  The default
mirrors that -- the operation draws its random number and changes nothing; apply_contrast=True applies the evident intent instead.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

# Configuration data of the training policy (ranges are closed below, open above, as numpy's uniform draws them).
TRAIN_POLICY = {
    "scale": (0.8, 1.2),             # per axis
    "shear": (-5.0, 5.0),            # degrees
    "translate": (-0.01, 0.01),      # fraction of the source side, per axis
    "rotate": (-179.0, 179.0),       # degrees
    "fliplr": 0.5,                   # probability
    "flipud": 0.5,
    "blur_max_ksize": 3,             # sizes are randint(0, 3) * 2 + 1 (loader/augs.py:27-28, 39-40)
    "noise_sigma": (0.0, 12.75),     # 0.05 * 255
    "noise_per_channel": 0.5,        # probability
    "hue": (-8.0, 8.0),
    "saturation": (-0.2, 0.2),
    "brightness": (-26.0, 26.0),
    "contrast": (0.75, 1.25),
}
COLOUR_OPS = ("hue", "saturation", "brightness", "contrast")  # colour_order holds indices into this tuple
MAX_SIDE = 16384


# ---- host: the warp's integer map -------------------------------------------------------------------------------------------------------------------
def compose_map(src_hw, out_hw, scale=(1.0, 1.0), shear=0.0, translate=(0.0, 0.0), rotate=0.0, fliplr=False, flipud=False):
    """The six Q16 integers (A, B, C, D, E, F) of cerb_aug_warp for one sample (include/cerberus_hip.h): the inverse of
    M = T(c + t) R(rotate) Shear_x(shear) S(scale) T(-c) in float64, each entry quantised with int(rint(m * 65536)), then the centre crop to out_hw and
    the two flips of the output folded into the integers exactly.  Angles in degrees, translate in pixels (x, y), scale (sx, sy)."""
    H, W = int(src_hw[0]), int(src_hw[1])
    h, w = int(out_hw[0]), int(out_hw[1])
    cx, cy = (W - 1) / 2.0, (H - 1) / 2.0
    th, ph = np.deg2rad(float(rotate)), np.deg2rad(float(shear))

    def T(tx, ty):
        return np.array([[1.0, 0.0, tx], [0.0, 1.0, ty], [0.0, 0.0, 1.0]], np.float64)

    R = np.array([[np.cos(th), -np.sin(th), 0.0], [np.sin(th), np.cos(th), 0.0], [0.0, 0.0, 1.0]], np.float64)
    Sh = np.array([[1.0, np.tan(ph), 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], np.float64)
    S = np.diag([float(scale[0]), float(scale[1]), 1.0])
    M = T(cx + float(translate[0]), cy + float(translate[1])) @ R @ Sh @ S @ T(-cx, -cy)
    a, b, c, d, e, f = M[0, 0], M[0, 1], M[0, 2], M[1, 0], M[1, 1], M[1, 2]
    det = a * e - b * d
    inv = (e / det, -b / det, (b * f - c * e) / det, -d / det, a / det, (c * d - a * f) / det)
    A, B, Cc, D, E, F = (int(np.rint(m * 65536.0)) for m in inv)
    oy, ox = (H - h) // 2, (W - w) // 2
    Cc, F = Cc + A * ox + B * oy, F + D * ox + E * oy
    if fliplr:
        Cc, F = Cc + A * (w - 1), F + D * (w - 1)
        A, D = -A, -D
    if flipud:
        Cc, F = Cc + B * (h - 1), F + E * (h - 1)
        B, E = -B, -E
    return np.array([A, B, Cc, D, E, F], np.int64)


# ---- host: the random draws -------------------------------------------------------------------------------------------------------------------------
def sample_params(n, src_hw, out_hw, rng, policy=TRAIN_POLICY, **fixed):
    """Per-sample parameters of augment_batch for n samples of src_hw = (H, W) cropped to out_hw = (h, w): a plain dict of numpy arrays.

    rng is a numpy.random.RandomState.  The draw ORDER is part of the contract (same seed -> same parameters; tests/test_augs_host.py freezes a
    table).  For sample 0, then sample 1, ... each sample draws, in this order:
       1. scale x, scale y        uniform(policy['scale'])  twice
       2. shear                   uniform(policy['shear'])  degrees
       3. translate x, y          uniform(policy['translate']) * W, then uniform(policy['translate']) * H  (pixels)
       4. rotate                  uniform(policy['rotate'])  degrees
       5. fliplr, flipud          random_sample() < p, twice
       6. which = randint(0, 3)   0 Gaussian blur, 1 median blur, 2 Gaussian noise; then that operation's own draws:
            Gaussian blur   randint(0, blur_max_ksize, size=(2,)) * 2 + 1 -> (kx, ky)       (loader/augs.py:27-28; OpenCV's ksize is (width, height))
            median blur     randint(0, blur_max_ksize) * 2 + 1                              (loader/augs.py:39-40)
            noise           sigma = uniform(policy['noise_sigma']); per_channel = random_sample() < p;
                            key = randint(0, 2**32, size=2, dtype=uint32) -> low word | high word << 32
       7. colour_order = permutation(4) over COLOUR_OPS = (hue, saturation, brightness, contrast)
       8. in THAT order, each colour operation's value: uniform(policy[<name>])  (contrast draws whether or not it is applied)
    Returned keys: 'map' int64 [n, 6] (compose_map), 'scale' [n, 2], 'shear' [n], 'translate' [n, 2], 'rotate' [n] (float64), 'fliplr' / 'flipud'
    bool [n], 'gauss_k' int32 [n, 2] = (kx, ky) and 'median_k' int32 [n] (0 = not chosen), 'noise_sigma' float64 [n] (NaN = not chosen),
    'noise_per_channel' int32 [n], 'noise_key' uint64 [n], 'colour_order' int32 [n, 4], 'hue' / 'saturation' / 'brightness' / 'contrast' float64 [n]
    (NaN = skip the operation for that sample).

    policy=None draws NOTHING: every parameter is the identity (unit scale, no blur or noise, NaN colour values) unless given by keyword --
    any of the returned keys except 'map', which is always composed here from the (given or drawn) affine parameters, e.g.
    sample_params(2, (64, 64), (48, 48), None, policy=None, rotate=[0.0, 90.0], gauss_k=[[3, 5], [0, 0]], median_k=[0, 3])."""
    n = int(n)
    H, W = int(src_hw[0]), int(src_hw[1])
    h, w = int(out_hw[0]), int(out_hw[1])
    if n < 1 or h < 1 or w < 1 or h > H or w > W:
        raise ValueError("sample_params: out_hw %s does not fit src_hw %s (n = %d)" % ((h, w), (H, W), n))
    p = OrderedDict()
    p["scale"], p["shear"], p["translate"], p["rotate"] = np.ones((n, 2)), np.zeros(n), np.zeros((n, 2)), np.zeros(n)
    p["fliplr"], p["flipud"] = np.zeros(n, bool), np.zeros(n, bool)
    p["gauss_k"], p["median_k"] = np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    p["noise_sigma"], p["noise_per_channel"], p["noise_key"] = np.full(n, np.nan), np.zeros(n, np.int32), np.zeros(n, np.uint64)
    p["colour_order"] = np.tile(np.arange(4, dtype=np.int32), (n, 1))
    for name in COLOUR_OPS:
        p[name] = np.full(n, np.nan)
    if policy is not None:
        for i in range(n):
            p["scale"][i] = rng.uniform(*policy["scale"]), rng.uniform(*policy["scale"])
            p["shear"][i] = rng.uniform(*policy["shear"])
            p["translate"][i] = rng.uniform(*policy["translate"]) * W, rng.uniform(*policy["translate"]) * H
            p["rotate"][i] = rng.uniform(*policy["rotate"])
            p["fliplr"][i] = rng.random_sample() < policy["fliplr"]
            p["flipud"][i] = rng.random_sample() < policy["flipud"]
            which = int(rng.randint(0, 3))
            if which == 0:
                p["gauss_k"][i] = rng.randint(0, policy["blur_max_ksize"], size=(2,)) * 2 + 1
            elif which == 1:
                p["median_k"][i] = int(rng.randint(0, policy["blur_max_ksize"])) * 2 + 1
            else:
                p["noise_sigma"][i] = rng.uniform(*policy["noise_sigma"])
                p["noise_per_channel"][i] = rng.random_sample() < policy["noise_per_channel"]
                lo, hi = (int(v) for v in rng.randint(0, 2 ** 32, size=2, dtype=np.uint32))
                p["noise_key"][i] = lo | (hi << 32)
            p["colour_order"][i] = rng.permutation(4)
            for op in p["colour_order"][i]:
                p[COLOUR_OPS[op]][i] = rng.uniform(*policy[COLOUR_OPS[op]])
    for k, v in fixed.items():
        if k not in p:
            raise KeyError("sample_params: unknown parameter %r (known: %s)" % (k, ", ".join(p)))
        v = np.asarray(v, dtype=p[k].dtype)
        if v.shape != p[k].shape:
            raise ValueError("sample_params: %r must have shape %s, got %s" % (k, p[k].shape, v.shape))
        p[k] = v.copy()
    p["map"] = np.stack([compose_map((H, W), (h, w), p["scale"][i], p["shear"][i], p["translate"][i], p["rotate"][i], p["fliplr"][i], p["flipud"][i])
                         for i in range(n)])
    return dict(p)


# ---- device plumbing --------------------------------------------------------------------------------------------------------------------------------
def _need_gpu():
    if not torch.cuda.is_available():
        raise _lib.CerberusHipError("cerberus_amd needs a ROCm GPU; there is no CPU fallback")


def _device_of(*arrays):
    for a in arrays:
        if torch.is_tensor(a) and a.is_cuda:
            return a.device
    return torch.device("cuda", torch.cuda.current_device())


def _image(img, dev, who):
    """uint8 [N, H, W, 3], contiguous, on the device (a numpy array is uploaded once)"""
    if isinstance(img, np.ndarray):
        if img.dtype != np.uint8:
            raise TypeError("%s: img must be uint8, got %s" % (who, img.dtype))
        img = torch.from_numpy(np.ascontiguousarray(img))
    if not torch.is_tensor(img) or img.dtype != torch.uint8:
        raise TypeError("%s: img must be a uint8 CUDA tensor or numpy array" % who)
    if img.dim() != 4 or img.shape[-1] != 3:
        raise ValueError("%s: img must be [N, H, W, 3], got %s" % (who, tuple(img.shape)))
    return img.to(dev).contiguous()


def _annotation(ann, dev, who):
    if isinstance(ann, np.ndarray):
        if ann.dtype.kind not in "iub":
            raise TypeError("%s: ann must hold integers, got %s" % (who, ann.dtype))
        ann = torch.from_numpy(np.ascontiguousarray(ann).astype(np.int32, copy=False))
    if not torch.is_tensor(ann) or ann.is_floating_point() or ann.is_complex():
        raise TypeError("%s: ann must be an integer CUDA tensor or numpy array" % who)
    if ann.dim() != 4 or not 1 <= ann.shape[-1] <= 8:
        raise ValueError("%s: ann must be [N, H, W, C] with 1 <= C <= 8, got %s" % (who, tuple(ann.shape)))
    return ann.to(dev, torch.int32).contiguous()


def _upload(sections, dev):
    """One pinned buffer, one asynchronous copy: sections = [numpy array, ...] -> device tensors viewing one allocation (each 8-byte aligned)."""
    offs, total = [], 0
    for a in sections:
        offs.append(total)
        total += (a.nbytes + 7) // 8 * 8
    host = torch.empty(max(total, 8), dtype=torch.uint8, pin_memory=True)
    hv = host.numpy()
    for a, o in zip(sections, offs):
        hv[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = host.to(dev, non_blocking=True)
    return [buf[o:o + a.nbytes] for a, o in zip(sections, offs)], buf


def _values(v, n, dtype, who):
    a = np.asarray(v, dtype=dtype)
    if a.ndim == 0:
        a = np.full(n, a, dtype=dtype)
    if a.shape != (n,):
        raise ValueError("%s: expected one value per sample (%d), got shape %s" % (who, n, a.shape))
    return a


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _sizes(k, n, who):
    k = _values(k, n, np.int32, who)
    if not np.isin(k, (1, 3, 5)).all():
        raise ValueError("%s: sizes must be 1, 3 or 5, got %s" % (who, k.tolist()))
    return k


# ---- single operations ------------------------------------------------------------------------------------------------------------------------------
def warp_crop(img, ann, maps, out_hw):
    """cerb_aug_warp: img uint8 [N, H, W, 3] and / or ann integer [N, H, W, C <= 8] (either may be None) gathered through maps (int64 [N, 6],
    compose_map) into [N, h, w, .]: nearest neighbour, 0 outside the source.  -> (img_out or None, ann_out or None), CUDA."""
    _need_gpu()
    if img is None and ann is None:
        raise ValueError("warp_crop: neither img nor ann")
    dev = _device_of(img, ann)
    img = None if img is None else _image(img, dev, "warp_crop")
    ann = None if ann is None else _annotation(ann, dev, "warp_crop")
    first = img if img is not None else ann
    n, H, W = (int(v) for v in first.shape[:3])
    if img is not None and ann is not None and tuple(ann.shape[:3]) != (n, H, W):
        raise ValueError("warp_crop: img %s and ann %s differ in N, H or W" % (tuple(img.shape), tuple(ann.shape)))
    h, w = int(out_hw[0]), int(out_hw[1])
    maps = np.ascontiguousarray(np.asarray(maps, dtype=np.int64))
    if maps.shape != (n, 6):
        raise ValueError("warp_crop: maps must be [N, 6], got %s" % (maps.shape,))
    with torch.cuda.device(dev):
        (dmaps,), _keep = _upload([maps], dev)
        return _warp(img, ann, dmaps, h, w)


def _warp(img, ann, dmaps, h, w):
    first = img if img is not None else ann
    dev = first.device
    n, H, W = (int(v) for v in first.shape[:3])
    if h < 1 or w < 1:
        raise ValueError("warp_crop: empty output %s" % ((h, w),))
    c = int(ann.shape[3]) if ann is not None else 0
    if max(H, W, h, w) > MAX_SIDE:  # the native call refuses it too; here BEFORE an output of that size is allocated
        raise _lib.CerberusHipError("warp_crop: side above %d" % MAX_SIDE)
    img_out = None if img is None else torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    ann_out = None if ann is None else torch.empty((n, h, w, c), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().cerb_aug_warp(None if img is None else img.data_ptr(), None if ann is None else ann.data_ptr(), n, H, W, c, dmaps.data_ptr(),
                                        None if img_out is None else img_out.data_ptr(), None if ann_out is None else ann_out.data_ptr(), h, w, _stream(dev)))
    return img_out, ann_out


def gaussian_blur(img, kx, ky):
    """cerb_aug_gaussian_blur: per-sample sizes kx, ky in {1, 3, 5} (a number or one per sample); integer weights, replicated borders."""
    _need_gpu()
    img = _image(img, _device_of(img), "gaussian_blur")
    n, h, w = (int(v) for v in img.shape[:3])
    kx, ky = _sizes(kx, n, "gaussian_blur"), _sizes(ky, n, "gaussian_blur")
    with torch.cuda.device(img.device):
        (dkx, dky), _keep = _upload([kx, ky], img.device)
        out = torch.empty_like(img)
        _lib.check(_lib.lib().cerb_aug_gaussian_blur(img.data_ptr(), out.data_ptr(), n, h, w, dkx.data_ptr(), dky.data_ptr(), _stream(img.device)))
    return out


def median_blur(img, k):
    """cerb_aug_median_blur: per-sample size k in {1, 3, 5}; per-channel median of the k x k window, replicated borders."""
    _need_gpu()
    img = _image(img, _device_of(img), "median_blur")
    n, h, w = (int(v) for v in img.shape[:3])
    k = _sizes(k, n, "median_blur")
    with torch.cuda.device(img.device):
        (dk,), _keep = _upload([k], img.device)
        out = torch.empty_like(img)
        _lib.check(_lib.lib().cerb_aug_median_blur(img.data_ptr(), out.data_ptr(), n, h, w, dk.data_ptr(), _stream(img.device)))
    return out


def gaussian_noise(img, sigma, per_channel, key):
    """cerb_aug_gaussian_noise: out = clip(floor(p + sigma z + 0.5), 0, 255) with z from Philox4x32-10 keyed per sample (uint64) and counted per pixel;
    per_channel: three independent normals per pixel instead of one shared by the channels.  sigma = 0 (or NaN) copies the sample."""
    _need_gpu()
    img = _image(img, _device_of(img), "gaussian_noise")
    n, h, w = (int(v) for v in img.shape[:3])
    sigma = _values(sigma, n, np.float64, "gaussian_noise")
    pc, key = _values(per_channel, n, np.int32, "gaussian_noise"), _values(key, n, np.uint64, "gaussian_noise")
    with torch.cuda.device(img.device):
        (ds, dp, dk), _keep = _upload([sigma, pc, key], img.device)
        out = torch.empty_like(img) if np.isfinite(sigma).all() else img.clone()
        _lib.check(_lib.lib().cerb_aug_gaussian_noise(img.data_ptr(), out.data_ptr(), n, h, w, ds.data_ptr(), dp.data_ptr(), dk.data_ptr(), _stream(img.device)))
    return out


def channel_sums(img):
    """cerb_aug_channel_sums: int64 [N, 3], the exact sum of every channel of every sample."""
    _need_gpu()
    img = _image(img, _device_of(img), "channel_sums")
    n, h, w = (int(v) for v in img.shape[:3])
    sums = torch.empty((n, 3), dtype=torch.int64, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.lib().cerb_aug_channel_sums(img.data_ptr(), n, h, w, sums.data_ptr(), _stream(img.device)))
    return sums


def _colour(op, img, value):
    _need_gpu()
    img = _image(img, _device_of(img), "add_to_" + op)
    n, h, w = (int(v) for v in img.shape[:3])
    value = _values(value, n, np.float64, "add_to_" + op)
    with torch.cuda.device(img.device):
        (dv,), _keep = _upload([value], img.device)
        out = torch.empty_like(img)
        _colour_launch(op, img, out, dv, _stream(img.device))
    return out


def _colour_launch(op, src, dst, dvalue, stream):
    L = _lib.lib()
    n, h, w = (int(v) for v in src.shape[:3])
    if op == "contrast":
        sums = torch.empty((n, 3), dtype=torch.int64, device=src.device)
        _lib.check(L.cerb_aug_channel_sums(src.data_ptr(), n, h, w, sums.data_ptr(), stream))
        _lib.check(L.cerb_aug_contrast(src.data_ptr(), dst.data_ptr(), n, h, w, dvalue.data_ptr(), sums.data_ptr(), stream))
    else:
        _lib.check(getattr(L, "cerb_aug_" + op)(src.data_ptr(), dst.data_ptr(), n, h, w, dvalue.data_ptr(), stream))


def add_to_hue(img, value):
    """cerb_aug_hue: 8-bit HSV (H in 0..179) in integers, H' = trunc((H + value) mod 180), back to RGB in float64.  NaN skips a sample."""
    return _colour("hue", img, value)


def add_to_saturation(img, value):
    """cerb_aug_saturation: trunc(clip(p s + grey (1 - s), 0, 255)), s = 1 + value, grey in OpenCV's 8-bit fixed point.  NaN skips a sample."""
    return _colour("saturation", img, value)


def add_to_brightness(img, value):
    """cerb_aug_brightness: trunc(clip(p + value, 0, 255)).  NaN skips a sample."""
    return _colour("brightness", img, value)


def add_to_contrast(img, value, apply_contrast=False):
    """The default mirrors the reference, whose add_to_contrast returns its input (module docstring): a copy.  apply_contrast=True:
    cerb_aug_contrast, trunc(clip(p value + mean_c (1 - value), 0, 255)) with mean_c the sample's exact channel mean.  NaN skips a sample."""
    if not apply_contrast:
        _need_gpu()
        img = _image(img, _device_of(img), "add_to_contrast")
        _values(value, int(img.shape[0]), np.float64, "add_to_contrast")
        return img.clone()
    return _colour("contrast", img, value)


# ---- the pipeline -----------------------------------------------------------------------------------------------------------------------------------
def augment_batch(img, ann, params, out_hw, apply_contrast=False):
    """img uint8 [N, H, W, 3], ann integer [N, H, W, C <= 8] (numpy: uploaded once; or CUDA), params from sample_params -> (img_aug uint8 [N, h, w, 3],
    ann_aug int32 [N, h, w, C]), contiguous CUDA tensors.

    Order: warp (image and annotation, one gather) -> each sample's one of Gaussian blur / median blur / noise (a sample with none is copied) -> the
    four colour operations in each sample's own colour_order.  Equal bit for bit to the single operations applied in that sequence.
    The blur, median and noise kernels share one source and one destination and each writes only its own samples; a colour kernel runs in place, once
    per (position in the order, operation) that some sample uses, with NaN for the other samples.  All parameters go up in ONE pinned, asynchronous
    copy; nothing synchronises the host."""
    _need_gpu()
    dev = _device_of(img, ann)
    img, ann = _image(img, dev, "augment_batch"), _annotation(ann, dev, "augment_batch")
    n, H, W = (int(v) for v in img.shape[:3])
    if tuple(ann.shape[:3]) != (n, H, W):
        raise ValueError("augment_batch: img %s and ann %s differ in N, H or W" % (tuple(img.shape), tuple(ann.shape)))
    h, w = int(out_hw[0]), int(out_hw[1])
    maps = np.ascontiguousarray(np.asarray(params["map"], dtype=np.int64))
    if maps.shape != (n, 6):
        raise ValueError("augment_batch: params are for %d samples, the batch has %d" % (maps.shape[0], n))
    gk = np.asarray(params["gauss_k"], np.int32).reshape(n, 2).copy()
    mk = np.asarray(params["median_k"], np.int32).reshape(n).copy()
    sigma = np.asarray(params["noise_sigma"], np.float64).reshape(n)
    chosen = (gk != 0).any(1).astype(int) + (mk != 0) + np.isfinite(sigma)
    if (chosen > 1).any():
        raise ValueError("augment_batch: a sample takes at most one of Gaussian blur / median blur / noise")
    if not np.isin(gk[(gk != 0).any(1)], (1, 3, 5)).all() or not np.isin(mk, (0, 1, 3, 5)).all():
        raise ValueError("augment_batch: blur sizes must be 1, 3 or 5")
    gk[chosen == 0] = 1  # none chosen: the 1 x 1 Gaussian is the copy
    order = np.asarray(params["colour_order"], np.int64).reshape(n, 4)
    if not (np.sort(order, 1) == np.arange(4)).all():
        raise ValueError("augment_batch: every row of colour_order must be a permutation of 0..3")
    rounds = []  # (position, operation name, values with NaN where the sample's operation at that position is another one)
    for r in range(4):
        for o, name in enumerate(COLOUR_OPS):
            vals = np.where(order[:, r] == o, np.asarray(params[name], np.float64).reshape(n), np.nan)
            if np.isfinite(vals).any() and (name != "contrast" or apply_contrast):
                rounds.append((name, vals))
    sections = [maps, np.ascontiguousarray(gk[:, 0]), np.ascontiguousarray(gk[:, 1]), mk, sigma,
                np.asarray(params["noise_per_channel"], np.int32).reshape(n), np.asarray(params["noise_key"], np.uint64).reshape(n)] + [v for _, v in rounds]
    L = _lib.lib()
    with torch.cuda.device(dev):
        stream = _stream(dev)
        views, _keep = _upload(sections, dev)
        dmaps, dkx, dky, dmk, dsig, dpc, dkey = views[:7]
        warped, ann_aug = _warp(img, ann, dmaps, h, w)
        out = torch.empty_like(warped)
        if (gk != 0).any():
            _lib.check(L.cerb_aug_gaussian_blur(warped.data_ptr(), out.data_ptr(), n, h, w, dkx.data_ptr(), dky.data_ptr(), stream))
        if (mk != 0).any():
            _lib.check(L.cerb_aug_median_blur(warped.data_ptr(), out.data_ptr(), n, h, w, dmk.data_ptr(), stream))
        if np.isfinite(sigma).any():
            _lib.check(L.cerb_aug_gaussian_noise(warped.data_ptr(), out.data_ptr(), n, h, w, dsig.data_ptr(), dpc.data_ptr(), dkey.data_ptr(), stream))
        for (name, _), dv in zip(rounds, views[7:]):
            _colour_launch(name, out, out, dv, stream)
    return out, ann_aug


def train_batch(img, ann, channel, channel_to_target, out_hw, crop_shape, rng, policy=TRAIN_POLICY, apply_contrast=False, params=None, **gen_targets_kwargs):
    """One training batch on the device: sample_params (unless `params` is given) -> augment_batch -> gen_targets_batch on the augmented annotation
    (fix_mirror_padding runs inside it) -> the dict cerberus_amd.train.train_step takes: the targets, 'dummy_target' and 'img' (uint8 CUDA
    [N, h, w, 3]).  channel / channel_to_target / crop_shape and the keyword arguments are gen_targets_batch's."""
    from .targets import gen_targets_batch

    if params is None:
        params = sample_params(int(img.shape[0]), tuple(img.shape[1:3]), out_hw, rng, policy=policy)
    img_aug, ann_aug = augment_batch(img, ann, params, out_hw, apply_contrast=apply_contrast)
    batch = gen_targets_batch(ann_aug, channel, channel_to_target, crop_shape, **gen_targets_kwargs)
    batch["img"] = img_aug
    return batch
