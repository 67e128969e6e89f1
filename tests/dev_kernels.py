"""ctypes bindings of the test-only entry layer of libcerberus_hip_dev.so (cerberus_amd/csrc/dev_entry.hip: cerb_dev_<kernel> wrappers over single
launchers of cerb_net.h) and the helpers that lay tensors out as the kernels expect.  Developer code: it lives under tests/, and works only in the
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
}
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
