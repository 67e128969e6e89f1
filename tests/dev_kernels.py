"""ctypes bindings of the test-only entry layer of libcerberus_hip_dev.so (cerberus_amd/csrc/dev_entry.hip: cerb_dev_<kernel> wrappers over single
launchers of cerb_net.h for the training step, cerb_devfwd_<kernel> for the forward path: cerb_devfwd_conv drives any one forward convolution launcher,
cerb_devfwd_stem / _head / _patch_class take raw weights and pack them as the handle does)
and the helpers that lay tensors out as the kernels expect, the tile-planar layout included.  Developer code: it lives under tests/, and works only in the
child process of a `dev_switches` test (CERB_DEV_LIB=1), where cerberus_amd loads the developers' library.

Layouts: activations NHWC with a leading group axis [G][N][H][W][C]; weights [G][Cout][Cin][k][k].

Three protections every case uses:
  * outputs and workspaces are carved out of a larger buffer filled with SENTINEL (Guarded): after the call the sentinel around the payload must be intact;
  * outputs a launcher documents as ASSIGNED start as NaN (the schedule skips their zero fill: a kernel that accumulates by mistake returns NaN);
  * outputs documented as ACCUMULATED start from random values, and the reference adds to them."""
import ctypes as C
import os

import torch

SENTINEL = 12345.6789
PAD = 16384  # floats of sentinel on each side of a payload: more than one row of the largest map used (56 x 64 channels)

_P, _I, _LL, _F, _SZ = C.c_void_p, C.c_int, C.c_longlong, C.c_float, C.c_size_t
_SIGS = {
    "cerb_dev_wgrad_wino_supported": (_I, [_I] * 4),
    "cerb_dev_wgrad_wino_workspace_bytes": (_SZ, [_I] * 6),
    "cerb_dev_wgrad_wino": (_I, [_P] * 4 + [_I] * 6 + [_LL, _P, _P]),
    "cerb_dev_wgrad_workspace_bytes": (_SZ, [_I] * 7 + [C.POINTER(C.c_int)]),
    "cerb_dev_wgrad": (_I, [_P] * 4 + [_I] * 8 + [_LL, _P, _P]),
    "cerb_dev_stem_wgrad_mfma_workspace_bytes": (_SZ, []),
    "cerb_dev_stem_wgrad_mfma": (_I, [_P] * 3 + [_I] * 3 + [_P, _P]),
    "cerb_dev_stem_wgrad": (_I, [_P] * 3 + [_I] * 3 + [_P]),
    "cerb_dev_conv_bwd": (_I, [_P] * 6 + [_I] * 8 + [_LL, _P]),
    "cerb_dev_bn_workspace_bytes": (_SZ, [_I, _LL, _I]),
    "cerb_dev_bn_fold_workspace_bytes": (_SZ, [_I, _I]),
    "cerb_dev_bn_stats": (_I, [_P, _LL, _LL, _I, _I, _F] + [_P] * 5),
    "cerb_dev_bn_finalize": (_I, [_P, _I, _LL, _I, _F] + [_P] * 3 + [_I, _P, _P]),
    "cerb_dev_bn_bwd": (_I, [_P] * 5 + [_LL, _LL, _I, _I] + [_P] * 6 + [_I, _I, _I, C.c_ulonglong, _P, _P]),
    "cerb_dev_upadd_bwd_fused_ok": (_I, [_I] * 4),
    "cerb_dev_upadd_bwd": (_I, [_P] * 3 + [_I] * 5 + [_LL, _I, C.c_uint, _I, _I, _P]),
    "cerb_dev_maxpool_idx": (_I, [_P] * 3 + [_I] * 4 + [_P]),
    "cerb_dev_maxpool_bwd_idx": (_I, [_P] * 3 + [_I] * 4 + [_P]),
    "cerb_dev_maxpool_bwd": (_I, [_P] * 4 + [_I] * 4 + [_P]),
    "cerb_dev_pointwise_bwd": (_I, [_P] * 6 + [_LL, _I, _I, _P, _I, _P]),
    "cerb_dev_pw_bwd_small_workspace_bytes": (_SZ, [_LL, _I, _I]),
    "cerb_dev_pw_bwd_small": (_I, [_P] * 6 + [_LL, _I, _I, _I, _P, _P]),
    "cerb_dev_pw_wgrad_small_workspace_bytes": (_SZ, [_LL, _I, _I]),
    "cerb_dev_pw_wgrad_small": (_I, [_P] * 3 + [_LL, _I, _I, _P, _P]),
    "cerb_dev_colsum_workspace_bytes": (_SZ, [_I, _I]),
    "cerb_dev_colsum": (_I, [_P, _LL, _LL, _I, _I, _P, _P, _P]),
    "cerb_dev_crop_gap": (_I, [_P] + [_I] * 8 + [_P, _P]),
    "cerb_dev_crop_gap_bwd": (_I, [_P, _P] + [_I] * 8 + [_P]),
    "cerb_dev_dilate2": (_I, [_P, _P, _LL, _I, _I, _I, _P]),
    # the forward path, one launcher at a time (cerb_devfwd_*)
    "cerb_devfwd_planar_elems": (_LL, [_I] * 4),
    "cerb_devfwd_upsample2_add": (_I, [_P] * 3 + [_I] * 5 + [_LL, _P]),
    "cerb_devfwd_upsample2_add_planar": (_I, [_P] * 3 + [_I] * 5 + [_LL, _LL, _I, _P]),
    "cerb_devfwd_conv3x3": (_I, [_P] * 5 + [_I] * 7 + [_P]),
    "cerb_devfwd_conv_s2": (_I, [_P] * 4 + [_I] * 8 + [_P]),
    "cerb_devfwd_maxpool": (_I, [_P] * 2 + [_I] * 5 + [_P]),
    "cerb_devfwd_planar_to_nhwc": (_I, [_P] * 2 + [_I] * 4 + [_P]),
    "cerb_devfwd_conv": (_I, [_I] * 5 + [_P, _I, _I] + [_P] * 6 + [_I] * 7 + [_LL] * 5 + [C.POINTER(C.c_int)] + [_I] * 3 + [_P]),
    "cerb_devfwd_wino4b_packed": (_I, [_I] * 6),
    "cerb_devfwd_wino4b_bn_blocks": (_I, [_I] * 6),
    # stem, output heads, Patch-Class, the decoder entry with a region (tests/test_net_kernels_parity_gpu.py)
    "cerb_devfwd_stem": (_I, [_P] * 5 + [_I, _P] + [_I] * 4 + [_P]),
    "cerb_devfwd_head": (_I, [_I, _P, _I, _I, _I, _I, _P, _I, _P]),
    "cerb_devfwd_patch_class": (_I, [_P] * 9 + [_I] * 6 + [_P] * 3 + [_LL, _LL, _P]),
    "cerb_devfwd_upsample2_add_roi": (_I, [_P] * 3 + [_I] * 5 + [_LL, C.POINTER(C.c_int), _P]),
    "cerb_devfwd_upsample2_add_planar_roi": (_I, [_P] * 3 + [_I] * 5 + [_LL, _LL, C.POINTER(C.c_int), _I, _P]),
    # the training step's fused output-head passes and the separate passes beside them (tests/test_head_train_parity_gpu.py)
    "cerb_dev_head_train_supported": (_I, [_LL, _I, _I, _I]),
    "cerb_dev_head_fwd1": (_I, [_P] * 4 + [_LL, _P, C.POINTER(C.c_int)] + [_P] * 5),
    "cerb_dev_head_fwd2": (_I, [_P] * 8 + [_LL, _I, _P]),
    "cerb_dev_head_bwd_workspace_bytes": (_SZ, [_LL, _I]),
    "cerb_dev_head_bwd1": (_I, [_P] * 11 + [_LL, _I, _P, _P]),
    "cerb_dev_head_bwd2": (_I, [_P] * 14 + [_LL, _I, _I, _I] + [_P] * 6 + [C.POINTER(C.c_int), _P]),
    "cerb_dev_pointwise": (_I, [_P] * 4 + [_LL, _I, _I, _P, _P, C.POINTER(C.c_int), _P]),
    "cerb_dev_bn_apply": (_I, [_P] * 3 + [_LL, _LL, _I, _I] + [_P] * 4 + [_I, _P]),
}


class DevHead(C.Structure):
    """one head of cerb_devfwd_head (dev_entry.hip: struct DevHead); the first six are HOST float arrays, the pointers from `logits` on DEVICE ones"""
    _fields_ = [(n, _P) for n in ("w1", "b1", "scale", "shift", "w2", "b2")] + [
        (n, _I) for n in ("out_ch", "kind", "crop_y0", "crop_x0", "out_h", "out_w", "roi", "pad_")] + [
        ("logits", _P), ("out_inst", _P), ("out_type_u8", _P), ("out_type_i64", _P), ("tile_off", _P), ("tile_stride", _LL), ("row_stride", _LL),
        ("absmax_bits", _P)]


def hptr(t):
    """host pointer of a contiguous CPU tensor (the caller keeps the tensor alive across the call)"""
    assert not t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())
ENTRIES = sorted(_SIGS)
_lib = None


def lib():
    """The developers' library with argtypes on every cerb_dev_* entry."""
    global _lib
    if _lib is None:
        assert os.environ.get("CERB_DEV_LIB") == "1", "the cerb_dev_* entries exist only in libcerberus_hip_dev.so: run under conftest.dev_switches"
        from cerberus_amd import _lib as binding

        L = binding.lib()
        for name, (res, args) in _SIGS.items():
            f = getattr(L, name)
            f.restype, f.argtypes = res, args
        L.cerb_conv_guard_bytes.restype, L.cerb_conv_guard_bytes.argtypes = _SZ, [_I]
        _lib = L
    return _lib


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """device pointer of a tensor / Guarded (None -> null)"""
    if t is None:
        return None
    if isinstance(t, Guarded):
        t = t.t
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


class Guarded(object):
    """An output (or workspace) carved out of a sentinel-filled device buffer.  init: None = NaN (an ASSIGNED output), or a float32 CPU tensor of start
    values (an ACCUMULATED output)."""

    def __init__(self, shape, init=None, dtype=torch.float32):
        shape = tuple(int(s) for s in shape)
        n = 1
        for s in shape:
            n *= s
        self.n = n
        self.big = torch.full((PAD + n + PAD,), SENTINEL, dtype=torch.float32, device="cuda")
        body = self.big[PAD:PAD + n]
        if init is None:
            body.fill_(float("nan"))
        else:
            assert init.dtype == torch.float32 and init.numel() == n
            body.copy_(init.reshape(-1))
        self.t = body.view(dtype).view(shape) if dtype != torch.float32 else body.view(shape)

    def intact(self):
        return bool((self.big[:PAD] == SENTINEL).all()) and bool((self.big[PAD + self.n:] == SENTINEL).all())

    def cpu(self):
        return self.t.detach().cpu()


def workspace(nbytes):
    """A NaN-poisoned, sentinel-guarded workspace of at least nbytes (a split-K workspace is ASSIGNED by its first kernel)."""
    return Guarded(((int(nbytes) + 3) // 4 + 4,))


def guard_bytes(W):
    return int(lib().cerb_conv_guard_bytes(int(W)))


def banded(t, W):
    """A kernel input the schedule keeps in a DevBuf with a guard band (DevBuf::ensure(bytes, cerb_conv_guard_bytes(W)) in cerb_train.hip): the tensor
    inside a larger zero-filled device buffer with the same band in front of and behind it."""
    g = guard_bytes(W)
    assert g % 16 == 0
    t = t.contiguous()
    raw = torch.zeros(2 * g + t.numel() * t.element_size(), dtype=torch.uint8, device="cuda")
    body = raw[g:g + t.numel() * t.element_size()].view(t.dtype).view(t.shape)
    body.copy_(t)
    return body


def ok(rc, what):
    assert rc == 0, "%s returned hipError %d" % (what, rc)
    torch.cuda.synchronize()


# ---- the tile-planar layout (cerb_common.h: cerb_planar_offset) --------------------------------------------------------------------------------------
def _planar_idx(n, h, w, c):
    """float index of every element of an [n][h][w][c] tensor in its tile-planar buffer (cerb_common.h: cerb_planar_offset), and the buffer's size"""
    byp, bxp, ncc = (h + 15) // 16 + 2, (w + 15) // 16 + 2, c // 16
    y, x = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
    off = (((y // 16 + 1) * bxp + x // 16 + 1) * ncc) * 4096 + (((y % 4) * 4 + x % 4) * 16 + ((y // 4) % 4) * 4 + (x // 4) % 4) * 16
    per_image = byp * bxp * ncc * 4096
    ch = torch.arange(c)
    idx = torch.arange(n).view(n, 1, 1, 1) * per_image + off.view(1, h, w, 1) + (ch // 16 * 4096 + ch % 16).view(1, 1, 1, c)
    return idx.cuda(), n * per_image


def _to_planar(t):
    n, h, w, c = t.shape
    idx, size = _planar_idx(n, h, w, c)
    buf = torch.zeros(size, device="cuda")
    buf[idx] = t
    return buf


def _check_planar(buf, ref, what):
    """every pixel of the tile-planar buffer equals the NHWC reference, whatever no pixel maps to (the guard ring) is zero"""
    n, h, w, c = ref.shape
    idx, size = _planar_idx(n, h, w, c)
    assert buf.numel() == size, what
    got = buf[idx]
    assert torch.equal(got, ref), (what, int((got != ref).sum()))
    written = torch.zeros(size, dtype=torch.bool, device="cuda")
    written[idx.reshape(-1)] = True
    assert bool((buf[~written] == 0).all()), (what, "guard ring")
