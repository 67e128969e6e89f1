"""Training targets on the device: mirror of the reference's loader/targets.py::gen_targets (+ loader/augs.py::fix_mirror_padding).

    gen_targets(ann, channel, channel_to_target, crop_shape, task_mode, **kwargs) -> (OrderedDict, has_flag)      one sample, the reference's protocol
    gen_targets_batch(ann [N, H, W, C], channel, channel_to_target, crop_shape, ...) -> dict                      what train_step takes beside 'img'

Target codes: IP, NP (binarise), TP, PC (pass through), IP-ERODED-3 / -11 (inner map 0 / 1), IP-ERODED-CONTOUR-3 / -11 (inner + 2 * contour);
the ERODED codes also give "<head>#WEIGHT-MAP" (the U-Net weight map + 1, or ones with gen_unet_weight_map=False).  As in the reference the
ERODED getters list three sub-channels ["", "", "#WEIGHT-MAP"] of which the first two share a key: the dict keeps the second (the class map) and
has_flag names the head twice (loader/targets.py:68,102,237-242).

Everything is computed by the cerb_target_* kernels of libcerberus_hip.so (csrc/targets.hip); there is no CPU path.  Returned maps are CUDA
tensors: class / pixel maps int32, weight maps float32, the fill of a head whose channel is absent float32 zeros (the reference: int32 /
float64 / float64 numpy arrays; train_step casts to float either way).

Host synchronisation: ONE per call that makes weight maps -- after the inner maps are labelled the host reads the number of labels per map and
their summed window area (a few integers) to size the distance-transform workspace.  A call without weight maps (no ERODED code, or
gen_unet_weight_map=False) synchronises nothing.  The workspaces are cached per device and shared by all calls: calls on one device run one after
the other (one stream at a time), as everywhere in this package.
"""
import ctypes as C
from collections import OrderedDict

import numpy as np
import torch

from . import _lib

# code -> (kind, element size, flag): flag = binarise for pixel codes, contour for eroded codes
TARGET_CODES = {
    "IP": ("pixel", 0, 1),
    "NP": ("pixel", 0, 1),
    "TP": ("pixel", 0, 0),
    "PC": ("pixel", 0, 0),
    "IP-ERODED-3": ("eroded", 3, 0),
    "IP-ERODED-11": ("eroded", 11, 0),
    "IP-ERODED-CONTOUR-3": ("eroded", 3, 1),
    "IP-ERODED-CONTOUR-11": ("eroded", 11, 1),
}
_SUB = {"pixel": [""], "eroded": ["", "", "#WEIGHT-MAP"]}
MAX_HEADS = 8  # CERB_TARGET_MAX_HEADS: heads per native call

_ws_cache = {}


def structuring_element(ksize):
    """cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (ksize, ksize)) by OpenCV's documented row-span formula, as the morphology kernel uses it
    (host only).  The 3 x 3 and 5 x 5 elements are pinned by tests/golden/cv2_documented.json; 11 x 11 follows the same formula (89 pixels) --
    OpenCV itself is not available to pin it."""
    ksize = int(ksize)
    out = np.zeros((ksize, ksize), np.uint8)
    _lib.check(_lib.lib().cerb_target_element(ksize, out.ctypes.data_as(C.c_void_p)))
    return out


def _scratch(dev, slot, nbytes):
    key = (dev.index if dev.index is not None else torch.cuda.current_device(), slot)
    t = _ws_cache.get(key)
    if t is None or t.numel() < nbytes:
        _ws_cache.pop(key, None)
        t = None
        _ws_cache[key] = t = torch.empty(int(nbytes), dtype=torch.uint8, device=dev)
    return t


def _check_args(ann, channel, channel_to_target, crop_shape, ndim):
    for ch_code, tg_code in channel_to_target.items():
        if tg_code not in TARGET_CODES:
            raise KeyError("gen_targets: unknown target code %r for %r (known: %s)" % (tg_code, ch_code, ", ".join(TARGET_CODES)))
    if isinstance(ann, np.ndarray):
        if ann.dtype.kind not in "iub":
            raise TypeError("gen_targets: ann must hold integers (instance / class ids), got %s" % ann.dtype)
        ann = torch.from_numpy(np.ascontiguousarray(ann).astype(np.int32, copy=False))
    if not torch.is_tensor(ann):
        raise TypeError("gen_targets: ann must be a CUDA tensor or a numpy array, got %s" % type(ann).__name__)
    if ann.is_floating_point() or ann.is_complex():
        raise TypeError("gen_targets: ann must hold integers (instance / class ids), got %s" % ann.dtype)
    if ann.dim() != ndim:
        raise ValueError("gen_targets: ann must have %d dimensions %s, got shape %s" % (ndim, "(N, H, W, C)" if ndim == 4 else "(H, W, C)", tuple(ann.shape)))
    h, w = int(ann.shape[-3]), int(ann.shape[-2])
    ch, cw = int(crop_shape[0]), int(crop_shape[1])
    if ch < 1 or cw < 1 or ch > h or cw > w:
        raise ValueError("gen_targets: crop_shape %s does not fit the %d x %d annotation" % ((ch, cw), h, w))
    return ann, (ch, cw)


def _heads_struct(heads):
    s = _lib.TargetHeads()
    s.n_heads = len(heads)
    for i, (_, chan, ksize, flag) in enumerate(heads):
        s.chan[i], s.ksize[i], s.flag[i] = chan, ksize, flag
    return s


def _pixel(ann, heads, crop):
    n, h, w, c = (int(v) for v in ann.shape)
    out = torch.empty((len(heads), n, crop[0], crop[1], 1), dtype=torch.int32, device=ann.device)
    stream = torch.cuda.current_stream(ann.device).cuda_stream
    hs = _heads_struct(heads)
    _lib.check(_lib.lib().cerb_target_pixel_maps(ann.data_ptr(), n, h, w, c, C.byref(hs), crop[0], crop[1], out.data_ptr(), C.c_void_p(stream)))
    return out


def _eroded(ann, heads, crop, weight_map, want_dsum):
    L = _lib.lib()
    n, h, w, c = (int(v) for v in ann.shape)
    dev = ann.device
    nh = len(heads)
    cls = torch.empty((nh, n, crop[0], crop[1], 1), dtype=torch.int32, device=dev)
    if not weight_map:
        wmap = torch.ones((nh, n, crop[0], crop[1], 1), dtype=torch.float32, device=dev)  # np.zeros(...) + 1 (loader/targets.py:95-97)
    else:
        wmap = torch.empty((nh, n, crop[0], crop[1], 1), dtype=torch.float32, device=dev)
    dsum = torch.empty_like(wmap) if (want_dsum and weight_map) else None
    ws = _scratch(dev, 0, L.cerb_target_workspace_bytes(nh * n, h, w))
    meta = torch.empty(2 + nh * n, dtype=torch.int32, device=dev) if weight_map else None
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    hs = _heads_struct(heads)
    _lib.check(L.cerb_target_eroded_maps(ann.data_ptr(), n, h, w, c, C.byref(hs), crop[0], crop[1], cls.data_ptr(), meta.data_ptr() if weight_map else None,
                                         ws.data_ptr(), ws.numel(), stream))
    if weight_map:
        m = meta.cpu().numpy()  # the call's one synchronisation: label counts and summed window area size the distance planes
        total = int(m[:2].view(np.uint64)[0])
        kmax = int(m[2:].max())
        wws = _scratch(dev, 1, L.cerb_target_window_workspace_bytes(nh * n, kmax, total))
        _lib.check(L.cerb_target_weight_maps(n, h, w, C.byref(hs), crop[0], crop[1], ws.data_ptr(), ws.numel(), kmax, total, wws.data_ptr(), wws.numel(),
                                             wmap.data_ptr(), dsum.data_ptr() if dsum is not None else None, stream))
    return cls, wmap, dsum


def _generate(ann, channel, channel_to_target, crop, gen_unet_weight_map, want_dsum, single_plane=False):
    """ann: CUDA int32 [N, H, W, C], contiguous.  Returns (OrderedDict key -> [N, h, w, 1], has_flag, {head: d1 + d2}).
    single_plane: every head whose name is in `channel` reads channel 0 (the whole-annotation modes)."""
    if not torch.cuda.is_available():
        raise _lib.CerberusHipError("cerberus_amd needs a ROCm GPU; there is no CPU fallback")
    channel = list(channel)
    n = int(ann.shape[0])
    pixel, eroded = [], []
    for ch_code, tg_code in channel_to_target.items():
        kind, ksize, flag = TARGET_CODES[tg_code]
        if ch_code in channel:
            (pixel if kind == "pixel" else eroded).append((ch_code, 0 if single_plane else channel.index(ch_code), ksize, flag))
    done, dsums = {}, {}
    with torch.cuda.device(ann.device):
        for i in range(0, len(pixel), MAX_HEADS):
            part = pixel[i:i + MAX_HEADS]
            out = _pixel(ann, part, crop)
            for j, hd in enumerate(part):
                done[hd[0]] = [out[j]]
        for i in range(0, len(eroded), MAX_HEADS):
            part = eroded[i:i + MAX_HEADS]
            cls, wmap, dsum = _eroded(ann, part, crop, gen_unet_weight_map, want_dsum)
            for j, hd in enumerate(part):
                done[hd[0]] = [cls[j], cls[j], wmap[j]]  # the reference's [bg_map, class map, weight map]: the first is overwritten by key
                if dsum is not None:
                    dsums[hd[0]] = dsum[j]
    target, has_flag = OrderedDict(), []
    for ch_code, tg_code in channel_to_target.items():
        sub = [ch_code + s for s in _SUB[TARGET_CODES[tg_code][0]]]
        if ch_code in done:
            maps = done[ch_code]
            has_flag.extend(sub)
        else:  # the channel is absent: dummy fill, None flags (loader/targets.py:219-221)
            maps = [torch.zeros((n, crop[0], crop[1], 1), dtype=torch.float32, device=ann.device)] * len(sub)
            has_flag.extend([None] * len(sub))
        for k, v in zip(sub, maps):
            target[k] = v
    return target, has_flag, dsums


def gen_targets(ann, channel, channel_to_target, crop_shape, task_mode="seg", gen_unet_weight_map=True, return_dsum=False, **kwargs):
    """The reference's gen_targets (loader/targets.py:185-244) for ONE sample on the device.

    ann: CUDA integer tensor (H, W, C) or numpy integer array (uploaded); channel: the names of ann's channels; channel_to_target: head name ->
    target code (TARGET_CODES); crop_shape: (h, w) of the centre crop.  Returns (OrderedDict name -> CUDA tensor (h, w, 1), has_flag): int32
    class / pixel maps, float32 "<head>#WEIGHT-MAP", float32 zeros (and None flags) for a head whose channel is absent.
    task_mode != 'seg' hands the whole `ann` to every getter as the reference does (loader/targets.py:226-227): a 2-D (H, W) annotation serves
    every code; with a 3-D one only the element-wise codes (IP / NP / TP / PC) are defined, per channel.
    return_dsum=True appends {head: d1 + d2 (h, w, 1) float32}, the distance sum before the weight map's exponential (tests).
    Synchronises the host once when it makes weight maps (module docstring)."""
    two_d = task_mode != "seg" and getattr(ann, "ndim", 3) == 2
    if two_d:
        ann = ann[..., None]
    ann, crop = _check_args(ann, channel, channel_to_target, crop_shape, 3)
    if task_mode != "seg":
        present = [c for c in channel_to_target if c in channel]
        if not two_d and any(TARGET_CODES[channel_to_target[c]][0] == "eroded" for c in present):
            raise ValueError("gen_targets: task_mode %r hands every getter the whole annotation; the ERODED codes need a 2-D (H, W) one" % (task_mode,))
        if not two_d:
            # the element-wise getters return (H, W, C) maps here, and the reference keeps only 2-D maps in its final list (loader/targets.py:238):
            # they drop out, and the codes pair up with what is left -- the dummy fills.  Reproduced literally; nothing is computed.
            dev = ann.device if ann.is_cuda else torch.device("cuda", torch.cuda.current_device())
            codes, maps, has_flag = [], [], []
            for ch_code, tg_code in channel_to_target.items():
                sub = [ch_code + c for c in _SUB[TARGET_CODES[tg_code][0]]]
                codes.extend(sub)
                if ch_code in channel:
                    has_flag.extend(sub)
                else:
                    maps.extend([torch.zeros(crop + (1,), dtype=torch.float32, device=dev)] * len(sub))
                    has_flag.extend([None] * len(sub))
            res = (OrderedDict(zip(codes, maps)), has_flag)
            return res + ({},) if return_dsum else res
    dev_ann = ann.to("cuda", torch.int32).contiguous()
    target, has_flag, dsums = _generate(dev_ann[None], channel, channel_to_target, crop, bool(gen_unet_weight_map), return_dsum, single_plane=two_d)
    target = OrderedDict((k, v[0]) for k, v in target.items())
    if return_dsum:
        return target, has_flag, {k: v[0] for k, v in dsums.items()}
    return target, has_flag


def gen_targets_batch(ann, channel, channel_to_target, crop_shape, task_mode="seg", gen_unet_weight_map=True, return_dsum=False, **kwargs):
    """gen_targets over a batch: ann CUDA integer tensor or numpy array [N, H, W, C] -> the dict cerberus_amd.train.train_step takes beside 'img':
    "<head>" -> [N, h, w, 1] (int32; float32 zeros for an absent channel), "<head>#WEIGHT-MAP" -> [N, h, w, 1] float32 and "dummy_target" ->
    object array [N, B] of head names / None built from has_flag.  Equal bit for bit to N gen_targets calls.

    All N samples and all heads of a kind go through the device together (one native call per group of up to 8 heads, every kernel launched once
    over N x heads maps); the values stay CUDA tensors.  One host synchronisation per group that makes weight maps (label counts and window area
    size the distance-transform workspace), none otherwise.  return_dsum=True returns (dict, {head: d1 + d2 [N, h, w, 1]})."""
    if task_mode != "seg":
        raise ValueError("gen_targets_batch: only task_mode='seg' is batched (gen_targets handles the whole-annotation modes)")
    ann, crop = _check_args(ann, channel, channel_to_target, crop_shape, 4)
    dev_ann = ann.to("cuda", torch.int32).contiguous()
    target, has_flag, dsums = _generate(dev_ann, channel, channel_to_target, crop, bool(gen_unet_weight_map), return_dsum)
    out = dict(target)
    dummy = np.empty((int(dev_ann.shape[0]), len(has_flag)), dtype=object)
    dummy[:] = [has_flag]
    out["dummy_target"] = dummy
    return (out, dsums) if return_dsum else out
