"""Kernel-level parity of the training step: every backward launcher of cerb_net.h on its own, through the test-only entry layer of the developers'
library (tests/dev_kernels.py), against a float64 reference of the same operation (tests/kernel_refs.py) at the smallest shapes that reach the
kernel's edges.  Per output tensor err(a) = max|a - ref64| / max|ref64|, and a kernel passes when err(kernel) <= K * err(yardstick) + 1e-7; the
yardstick is the same reference evaluated in float32 (for the Winograd-domain weight gradient: a float32 evaluation of that algorithm).  K per family
is at least twice the worst err(kernel) / err(yardstick) measured on the MI355X and never below 4 (table: DESIGN.md, "kernel-level parity of the
training step").  One test function per kernel family (the dev_switches decorator starts one child pytest per function); each prints its ratios."""
import os

import pytest
import torch

import dev_kernels as D
import kernel_refs as R
from conftest import dev_switches

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32


class Report(object):
    """Collects every figure of a family, prints it, and fails at the end with all misses (so one run shows every ratio)."""

    def __init__(self, family, k):
        self.family, self.k, self.bad, self.worst = family, k, [], 0.0

    def bar(self, case, name, got, ref64, yard):
        eg, ey = R.err(got, ref64), R.err(yard, ref64)
        ratio = eg / ey if ey > 0 else (0.0 if eg == 0 else float("inf"))
        self.worst = max(self.worst, ratio if eg > 1e-7 else 0.0)  # (below the absolute floor of the bar the ratio says nothing)
        print("%s %s %s: err %.3e yardstick %.3e ratio %.2f" % (self.family, case, name, eg, ey, ratio))
        if not eg <= self.k * ey + 1e-7:
            self.bad.append((case, name, "err %.3e > %g * %.3e + 1e-7" % (eg, self.k, ey)))

    def equal(self, case, name, got, ref):
        same = torch.equal(got.cpu(), ref)
        print("%s %s %s: %s" % (self.family, case, name, "equal" if same else "DIFFERS"))
        if not same:
            self.bad.append((case, name, "not equal to the reference"))

    def within_ulps(self, case, name, got, ref64, largest, ulps=4):
        """|got - ref64| <= ulps float32 ulps of the largest contribution"""
        import math

        ulp = 2.0 ** (math.floor(math.log2(largest)) - 23)
        g = got.cpu().to(F64)
        d = float((g - ref64).abs().max()) if bool(torch.isfinite(g).all()) else float("inf")
        print("%s %s %s: max diff %.3e = %.2f ulp of %.3e" % (self.family, case, name, d, d / ulp, largest))
        if not d <= ulps * ulp:
            self.bad.append((case, name, "%.2f ulp > %d" % (d / ulp, ulps)))

    def intact(self, case, *bufs):
        for i, b in enumerate(bufs):
            if b is not None and not b.intact():
                self.bad.append((case, "buffer %d" % i, "wrote outside its output / workspace"))

    def check(self, cond, case, what):
        if not cond:
            self.bad.append((case, what, "failed"))

    def finish(self):
        print("%s: worst err / yardstick ratio %.2f (K = %g)" % (self.family, self.worst, self.k))
        assert not self.bad, "%s: %d misses: %s" % (self.family, len(self.bad), self.bad[:12])


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _acc_init(ref64, gen):
    """start values of an ACCUMULATED output: random, of the size of what is added (a large start value would hide the kernel's error in the scale)"""
    s = float(ref64.std()) if ref64.numel() > 1 else float(ref64.abs().max())
    return (torch.randn(ref64.shape, generator=gen) * (s if s > 0 else 1.0)).to(F32)


# =====================================================================================================================================================
K_WGRAD_WINO = 4
WGRAD_WINO_CASES = [  # (G, N, H, W, Cin, Cout, with db)
    (1, 1, 8, 8, 64, 64, False),      # 4 tiles: one partial chunk, one slice
    (1, 1, 12, 20, 64, 64, True),     # 15 tiles: the last chunk is partial; non-square
    (1, 3, 12, 20, 64, 128, False),   # chunks straddle image boundaries: the halo of a tile at the top of image n + 1 must not read image n
    (5, 2, 20, 28, 128, 128, True),   # 20 channel tiles -> 6 slices over 9 chunks (uneven split); grouped, per-group x_gs
    (3, 1, 8, 12, 192, 320, True),    # 45 pairs, not a multiple of 8: idle workgroups in the rounded grid
    (1, 2, 8, 8, 512, 512, False),    # 64 channel tiles: the slice count clamped to 1
    (1, 2, 28, 28, 64, 64, True),     # the maps of the real step at 448 px
    (1, 1, 56, 56, 64, 64, False),
]


@dev_switches
def test_wgrad_wino_vs_float64_conv2d():
    L, rep, gen = D.lib(), Report("wgrad_wino", K_WGRAD_WINO), _gen(11)
    for G, N, H, W, Ci, Co, with_db in WGRAD_WINO_CASES:
        case = (G, N, H, W, Ci, Co, "db" if with_db else "-")
        x = torch.relu(torch.randn(G, N, H, W, Ci, generator=gen))
        dy = 1e-3 * torch.randn(G, N, H, W, Co, generator=gen)
        dw64, db64, _ = R.conv_grads(x, dy, None, 3, 1, F64)
        _, db32, _ = R.conv_grads(x, dy, None, 3, 1, F32)
        yard = R.wgrad_wino_formula(x, dy, F32)
        assert L.cerb_dev_wgrad_wino_supported(H, W, Ci, Co) == 1
        xd, dyd = D.banded(x.cuda(), W), dy.cuda()
        dw, db = D.Guarded((G, Co, Ci, 3, 3)), (D.Guarded((G, Co)) if with_db else None)
        ws = D.workspace(L.cerb_dev_wgrad_wino_workspace_bytes(G, N, H, W, Ci, Co))
        D.ok(L.cerb_dev_wgrad_wino(D.ptr(xd), D.ptr(dyd), D.ptr(dw), D.ptr(db), G, N, H, W, Ci, Co, N * H * W * Ci, D.ptr(ws), D.stream()), case)
        rep.bar(case, "dw", dw.cpu(), dw64, yard)
        if with_db:
            rep.bar(case, "db", db.cpu(), db64, db32)
        rep.intact(case, dw, db, ws)
    # shapes the kernel does not serve: the predicate refuses them and the launcher returns an error instead of launching
    x1, o1, w1 = torch.zeros(1 << 16, device="cuda"), torch.zeros(1 << 16, device="cuda"), torch.zeros(1 << 20, device="cuda")
    for H, W, Ci, Co in ((10, 8, 64, 64), (8, 10, 64, 64), (4, 8, 64, 64), (8, 4, 64, 64), (8, 8, 96, 64), (8, 8, 64, 32), (8, 8, 64, 96)):
        rep.check(L.cerb_dev_wgrad_wino_supported(H, W, Ci, Co) == 0, (H, W, Ci, Co), "cerb_wgrad_wino_supported refuses")
        rc = L.cerb_dev_wgrad_wino(D.ptr(x1), D.ptr(o1), D.ptr(w1), None, 1, 1, H, W, Ci, Co, H * W * Ci, D.ptr(w1), D.stream())
        rep.check(rc != 0, (H, W, Ci, Co), "the launcher returns an error")
    torch.cuda.synchronize()
    rep.finish()


# =====================================================================================================================================================
K_WGRAD = 4
WGRAD_CASES = [  # (G, N, H, W, Cin, Cout, ks, stride, with db); H, W: the INPUT map
    (1, 2, 3, 5, 512, 512, 3, 1, True), (1, 2, 6, 10, 256, 256, 3, 1, False),   # odd and tiny maps
    (1, 1, 4, 4, 512, 512, 3, 1, False),                                         # 64 tiles x 4 segments: the slice count clamped by nseg
    (5, 2, 6, 10, 64, 64, 3, 1, True),
    (1, 2, 6, 10, 64, 128, 3, 2, True), (1, 2, 16, 16, 64, 128, 3, 2, False), (1, 2, 12, 20, 128, 256, 3, 2, True),   # rows 2 yo - 1 + ky
    (1, 2, 6, 10, 64, 128, 1, 2, False), (1, 2, 16, 16, 64, 128, 1, 2, True), (1, 2, 12, 20, 128, 256, 1, 2, False),  # the downsample branches
    # pointwise: N = H = 1, W = rows on both sides of the 32-pixel segment and not multiples of it
    (1, 1, 1, 64, 64, 96, 1, 1, True), (1, 1, 1, 1000, 64, 96, 1, 1, True), (1, 1, 1, 4097, 64, 96, 1, 1, True),      # 96: the padded channel block
    (1, 1, 1, 64, 512, 64, 1, 1, False), (1, 1, 1, 1000, 512, 64, 1, 1, True), (1, 1, 1, 4097, 512, 64, 1, 1, False),  # conv_map's shape
    (1, 2, 40, 40, 64, 64, 3, 1, True), (1, 1, 1, 33, 96, 64, 1, 1, False),     # a row of two segments, the second partial; 96 input channels
]


@dev_switches
def test_wgrad_direct_vs_float64_conv2d():
    import ctypes

    L, rep, gen = D.lib(), Report("wgrad", K_WGRAD), _gen(12)
    for G, N, H, W, Ci, Co, ks, stride, with_db in WGRAD_CASES:
        case = (G, N, H, W, Ci, Co, "k%d s%d" % (ks, stride), "db" if with_db else "-")
        Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
        x = torch.relu(torch.randn(G, N, H, W, Ci, generator=gen))
        dy = 1e-3 * torch.randn(G, N, Ho, Wo, Co, generator=gen)
        dw64, db64, _ = R.conv_grads(x, dy, None, ks, stride, F64)
        dw32, db32, _ = R.conv_grads(x, dy, None, ks, stride, F32)
        xd, dyd = D.banded(x.cuda(), W), dy.cuda()
        dw, db = D.Guarded((G, Co, Ci, ks, ks)), (D.Guarded((G, Co)) if with_db else None)
        slices = ctypes.c_int(0)
        ws = D.workspace(L.cerb_dev_wgrad_workspace_bytes(G, N, Ho, Wo, Ci, Co, ks, ctypes.byref(slices)))
        D.ok(L.cerb_dev_wgrad(D.ptr(xd), D.ptr(dyd), D.ptr(dw), D.ptr(db), G, N, H, W, Ci, Co, ks, stride, N * H * W * Ci, D.ptr(ws), D.stream()), case)
        rep.bar(case + ("%d slices" % slices.value,), "dw", dw.cpu(), dw64, dw32)
        if with_db:
            rep.bar(case, "db", db.cpu(), db64, db32)
        rep.intact(case, dw, db, ws)
    rep.finish()


# =====================================================================================================================================================
K_STEM = 4


@dev_switches
def test_stem_wgrad_vs_float64_conv2d():
    L, rep, gen = D.lib(), Report("stem_wgrad", K_STEM), _gen(13)
    ws_bytes = L.cerb_dev_stem_wgrad_mfma_workspace_bytes()
    for N, H, W in ((1, 16, 16), (2, 16, 48), (3, 32, 16)):   # edge pixels dominate at 16 x 16
        tiles = torch.randint(0, 256, (N, H, W, 3), generator=gen, dtype=torch.uint8)
        dy = 1e-3 * torch.randn(N, H, W, 64, generator=gen)
        dw64, dw32 = R.stem_wgrad(tiles, dy, F64), R.stem_wgrad(tiles, dy, F32)
        td, dyd = tiles.cuda(), dy.cuda()
        dw, ws = D.Guarded((64, 3, 7, 7)), D.workspace(ws_bytes)
        D.ok(L.cerb_dev_stem_wgrad_mfma(D.ptr(td), D.ptr(dyd), D.ptr(dw), N, H, W, D.ptr(ws), D.stream()), (N, H, W))
        rep.bar((N, H, W), "dw (mfma)", dw.cpu(), dw64, dw32)
        rep.intact((N, H, W), dw, ws)
        del ws
        dw = D.Guarded((64, 3, 7, 7))
        D.ok(L.cerb_dev_stem_wgrad(D.ptr(td), D.ptr(dyd), D.ptr(dw), N, H, W, D.stream()), (N, H, W))
        rep.bar((N, H, W), "dw (gather)", dw.cpu(), dw64, dw32)
        rep.intact((N, H, W), dw)
    rep.finish()


# =====================================================================================================================================================
K_CONV_BWD = 10  # dx of the 3x3 cases: one float32 fmaf chain over 9 * Cout = 576 .. 1152 terms per element (conv_dgrad_kernel), measured 4.64


@dev_switches
def test_conv_bwd_fallback_vs_float64_conv2d():
    L, rep, gen = D.lib(), Report("conv_bwd", K_CONV_BWD), _gen(14)
    for G, N, H, W, Ci, Co in ((1, 2, 6, 10, 64, 128), (2, 1, 8, 8, 64, 64)):
        for ks in (1, 3):
            for stride in (1, 2):
                case = (G, N, H, W, Ci, Co, "k%d s%d" % (ks, stride))
                Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
                x = torch.relu(torch.randn(G, N, H, W, Ci, generator=gen))
                dy = 1e-3 * torch.randn(G, N, Ho, Wo, Co, generator=gen)
                w = torch.randn(G, Co, Ci, ks, ks, generator=gen) / (Ci * ks * ks) ** 0.5
                dw64, db64, dx64 = R.conv_grads(x, dy, w, ks, stride, F64)
                dw32, db32, dx32 = R.conv_grads(x, dy, w, ks, stride, F32)
                dx0 = _acc_init(dx64, gen)   # dx is ACCUMULATED, dw / db are ASSIGNED
                xd, dyd, wd = D.banded(x.cuda(), W), dy.cuda(), w.cuda()
                dx, dw, db = D.Guarded(dx64.shape, dx0), D.Guarded(dw64.shape), D.Guarded(db64.shape)
                D.ok(L.cerb_dev_conv_bwd(D.ptr(xd), D.ptr(dyd), D.ptr(wd), D.ptr(dx), D.ptr(dw), D.ptr(db), G, N, H, W, Ci, Co, ks, stride, N * H * W * Ci, D.stream()), case)
                rep.bar(case, "dx", dx.cpu(), dx0.to(F64) + dx64, dx0 + dx32)
                rep.bar(case, "dw", dw.cpu(), dw64, dw32)
                rep.bar(case, "db", db.cpu(), db64, db32)
                rep.intact(case, dx, dw, db)
    rep.finish()


# =====================================================================================================================================================
K_BN = 4
BN_FOLD_ROWS = 8193  # the smallest row count with more than 256 partial rows per group: bn_rpb(8193, 1) = 32 rows per block -> 257 blocks (> 256: the fold kernel)


def _bn_input(G, rows, C, gen):
    """per-channel spread in [0.5, 2] and mean in [-1, 1]: the variance is well away from zero"""
    return torch.randn(G, rows, C, generator=gen) * (0.5 + 1.5 * torch.rand(G, 1, C, generator=gen)) + (2 * torch.rand(G, 1, C, generator=gen) - 1)


@dev_switches
def test_batchnorm_statistics_vs_float64():
    L, rep, gen = D.lib(), Report("bn_stats", K_BN), _gen(15)
    for G, rows, C in ((1, 30, 64), (5, 33, 96), (1, 30, 512), (5, 2049, 64), (1, 2049, 512), (1, BN_FOLD_ROWS, 64), (5, 4097, 96)):
        case = (G, rows, C)
        y = _bn_input(G, rows, C, gen)
        ref64, ref32 = R.bn_stats(y, F64), R.bn_stats(y, F32)
        yd = y.cuda()
        out = [D.Guarded((G, C)) for _ in range(3)]
        ws = D.workspace(L.cerb_dev_bn_workspace_bytes(G, rows, C))
        D.ok(L.cerb_dev_bn_stats(D.ptr(yd), rows * C, rows, C, G, 1e-5, D.ptr(out[0]), D.ptr(out[1]), D.ptr(out[2]), D.ptr(ws), D.stream()), case)
        for i, name in enumerate(("mean", "rstd", "var_unbiased")):
            rep.bar(case, name, out[i].cpu(), ref64[i], ref32[i])
        rep.intact(case, ws, *out)
    # cerb_launch_bn_finalize on partials a producer left: [G][blocks][C][(sum, sum of squares)] doubles, 300 blocks (> 256: folded first) and 7
    for G, rows, C, blocks in ((2, 3000, 96, 300), (1, 70, 64, 7)):
        case = (G, rows, C, "%d blocks" % blocks)
        y = _bn_input(G, rows, C, gen)
        ref64, ref32 = R.bn_stats(y, F64), R.bn_stats(y, F32)
        per = rows // blocks
        yb = y.to(F64).view(G, blocks, per, C)
        part = torch.stack([yb.sum(2), (yb * yb).sum(2)], -1).contiguous().cuda()
        out = [D.Guarded((G, C)) for _ in range(3)]
        fold = D.workspace(L.cerb_dev_bn_fold_workspace_bytes(G, C))
        D.ok(L.cerb_dev_bn_finalize(D.ptr(part), blocks, rows, C, 1e-5, D.ptr(out[0]), D.ptr(out[1]), D.ptr(out[2]), G, D.ptr(fold), D.stream()), case)
        for i, name in enumerate(("mean", "rstd", "var_unbiased")):
            rep.bar(case, name + " (finalize)", out[i].cpu(), ref64[i], ref32[i])
        rep.intact(case, fold, *out)
    rep.finish()


BN_BWD_CASES = [  # G, rows, C, relu, resid, dy_assign, dresid_assign, eval groups
    dict(G=1, rows=30, C=64, relu=1, resid=False, dy_assign=1, dresid_assign=0, ev=()),      # relu behind a BatchNorm without residual: the internal relu = 2 path
    dict(G=1, rows=30, C=64, relu=1, resid=True, dy_assign=0, dresid_assign=1, ev=()),
    dict(G=5, rows=33, C=96, relu=0, resid=False, dy_assign=0, dresid_assign=0, ev=()),
    dict(G=5, rows=33, C=96, relu=1, resid=True, dy_assign=1, dresid_assign=0, ev=(1, 3)),   # groups 1 and 3 in eval mode
    dict(G=1, rows=2049, C=512, relu=1, resid=True, dy_assign=1, dresid_assign=1, ev=()),
    dict(G=5, rows=2049, C=64, relu=1, resid=False, dy_assign=0, dresid_assign=0, ev=(0, 4)),
    dict(G=1, rows=4097, C=96, relu=0, resid=True, dy_assign=0, dresid_assign=0, ev=()),
    dict(G=1, rows=BN_FOLD_ROWS, C=64, relu=1, resid=False, dy_assign=1, dresid_assign=0, ev=()),   # the fold kernel of the backward sums
    dict(G=1, rows=BN_FOLD_ROWS, C=64, relu=0, resid=False, dy_assign=1, dresid_assign=0, ev=(0,)),
]


def _bn_case_inputs(c, gen):
    """Inputs whose ReLU decisions are the same in float32 and float64: elements whose pre-activation is within 1e-3 of zero are moved away from it
    (a flipped mask is a property of the input, not of the kernel; the kernels recompute the mask in float32)."""
    G, rows, C = c["G"], c["rows"], c["C"]
    y = _bn_input(G, rows, C, gen)
    gamma, beta = 0.5 + torch.rand(G, C, generator=gen), 0.5 * torch.randn(G, C, generator=gen)
    resid = torch.randn(G, rows, C, generator=gen) if c["resid"] else None
    run_mean, run_var = 0.3 * torch.randn(G, C, generator=gen), 0.5 + 1.5 * torch.rand(G, C, generator=gen)
    if c["relu"]:
        for _ in range(4):
            _, zs = R.bn_forward(y, gamma, beta, resid, False, c["ev"], run_mean, run_var, F64)
            near = torch.stack([z.detach() for z in zs]).abs() < 1e-3
            if not bool(near.any()):
                break
            if resid is not None:
                resid = resid + near.to(F32) * 0.01
            else:
                y = y + near.to(F32) * 0.02 * torch.sign(gamma).view(G, 1, C)
        else:
            raise AssertionError("could not move the pre-activations away from zero")
    dz = 1e-3 * torch.randn(G, rows, C, generator=gen)
    return y, gamma, beta, resid, run_mean, run_var, dz


@dev_switches
def test_batchnorm_backward_vs_float64_autograd():
    L, rep, gen = D.lib(), Report("bn_bwd", K_BN), _gen(16)
    for c in BN_BWD_CASES:
        G, rows, C = c["G"], c["rows"], c["C"]
        case = tuple(sorted(c.items()))
        y, gamma, beta, resid, run_mean, run_var, dz = _bn_case_inputs(c, gen)
        res = {}
        for dt in (F64, F32):
            leaves, zs = R.bn_forward(y, gamma, beta, resid, c["relu"], c["ev"], run_mean, run_var, dt)
            res[dt] = R.bn_backward(leaves, zs, dz, dt) + (torch.stack([z.detach() for z in zs]),)
        dy64, dres64, dga64, dbe64, z64 = res[F64]
        dy32, dres32, dga32, dbe32, _ = res[F32]
        # the statistics the kernel is handed: batch statistics, or the running ones for the groups in eval mode
        mean, rstd, _ = R.bn_stats(y, F64)
        eval_mask = 0
        for g in c["ev"]:
            mean[g], rstd[g] = run_mean[g].to(F64), 1.0 / torch.sqrt(run_var[g].to(F64) + 1e-5)
            eval_mask |= 1 << g
        dy0 = None if c["dy_assign"] else _acc_init(dy64, gen)
        dres0 = None if (resid is None or c["dresid_assign"]) else _acc_init(dres64, gen)
        dev = [t.cuda() for t in (dz, z64.to(F32), y, mean.to(F32).contiguous(), rstd.to(F32).contiguous(), gamma, beta)]
        dy, dga, dbe = D.Guarded((G, rows, C), dy0), D.Guarded((G, C)), D.Guarded((G, C))
        dres = D.Guarded((G, rows, C), dres0) if resid is not None else None
        ws = D.workspace(L.cerb_dev_bn_workspace_bytes(G, rows, C))
        D.ok(L.cerb_dev_bn_bwd(D.ptr(dev[0]), D.ptr(dev[1]), D.ptr(dev[2]), D.ptr(dy), D.ptr(dres), rows * C, rows, C, G, D.ptr(dev[3]), D.ptr(dev[4]), D.ptr(dev[5]),
                               D.ptr(dev[6]), D.ptr(dga), D.ptr(dbe), c["relu"], c["dy_assign"], c["dresid_assign"], eval_mask, D.ptr(ws), D.stream()), case)
        rep.bar(case, "dy", dy.cpu(), dy64 if dy0 is None else dy0.to(F64) + dy64, dy32 if dy0 is None else dy0 + dy32)
        if resid is not None:
            rep.bar(case, "dresid", dres.cpu(), dres64 if dres0 is None else dres0.to(F64) + dres64, dres32 if dres0 is None else dres0 + dres32)
        rep.bar(case, "dgamma", dga.cpu(), dga64, dga32)
        rep.bar(case, "dbeta", dbe.cpu(), dbe64, dbe32)
        rep.intact(case, dy, dres, dga, dbe, ws)
    rep.finish()


# =====================================================================================================================================================
K_UPADD = 5


@dev_switches
def test_upsample_add_backward_vs_float64_interpolate():
    L, rep, gen = D.lib(), Report("upadd_bwd", K_UPADD), _gen(17)
    cases = []
    i = 0
    for H, W in ((2, 2), (4, 6), (6, 10), (16, 16)):   # 2 x 2 and 4 x 6: the clamped bilinear taps at the border dominate
        for C in (64, 512):
            for G in (1, 5):
                for shared in (0, 1):
                    # the flags rotate so that every value of each meets every map size; masks leave groups out (fused kernel only)
                    mask = 0xffffffff if (G == 1 or i % 3 == 0) else (0b10110 if i % 3 == 1 else 0b01001)
                    cases.append((1 + i % 2, H, W, C, G, shared, mask, (i // 2) % 2, (i // 3) % 2, False))
                    i += 1
    for H, W, C, G, shared in ((2, 2, 64, 5, 0), (4, 6, 512, 5, 1), (6, 10, 64, 1, 0), (16, 16, 64, 5, 1), (16, 16, 512, 5, 0)):
        cases.append((2, H, W, C, G, shared, 0xffffffff, 0, 0, True))   # the two-pass kernels: all groups, accumulate only
    for N, H, W, C, G, shared, mask, skip_assign, prev_assign, two_pass in cases:
        case = (N, H, W, C, G, "shared" if shared else "own", "mask %x" % (mask & ((1 << G) - 1)), "skip=" if skip_assign else "skip+=", "prev=" if prev_assign else "prev+=",
                "two-pass" if two_pass else "fused")
        if two_pass:
            os.environ["CERB_UPADD_BWD_TWO_PASS"] = "1"
        else:
            os.environ.pop("CERB_UPADD_BWD_TWO_PASS", None)
        rep.check(L.cerb_dev_upadd_bwd_fused_ok(H, W, C, G) == (0 if two_pass else 1), case, "kernel selection")
        dout = 1e-3 * torch.randn(G, N, H, W, C, generator=gen)
        live = [bool((mask >> g) & 1) for g in range(G)]
        ds64, dp64 = R.upadd_grads(dout, shared, live, F64)
        ds32, dp32 = R.upadd_grads(dout, shared, live, F32)
        ds0 = None if skip_assign else _acc_init(ds64, gen)
        dp0 = None if prev_assign else _acc_init(dp64, gen)
        dd = dout.cuda()
        ds, dp = D.Guarded(ds64.shape, ds0), D.Guarded(dp64.shape, dp0)
        prev_gs = 0 if shared else N * (H // 2) * (W // 2) * C
        D.ok(L.cerb_dev_upadd_bwd(D.ptr(dd), D.ptr(ds), D.ptr(dp), G, N, H, W, C, prev_gs, shared, mask, skip_assign, prev_assign, D.stream()), case)
        rep.bar(case, "dskip", ds.cpu(), ds64 if ds0 is None else ds0.to(F64) + ds64, ds32 if ds0 is None else ds0 + ds32)
        rep.bar(case, "dprev", dp.cpu(), dp64 if dp0 is None else dp0.to(F64) + dp64, dp32 if dp0 is None else dp0 + dp32)
        rep.intact(case, ds, dp)
    os.environ.pop("CERB_UPADD_BWD_TWO_PASS", None)
    rep.finish()


# =====================================================================================================================================================
@dev_switches
def test_maxpool_routing_vs_torch_cpu():
    L, rep, gen = D.lib(), Report("maxpool", 0), _gen(18)
    for N in (1, 3):
        for H, W in ((2, 2), (4, 6), (16, 16), (32, 48)):
            case, C = (N, H, W), 64
            x = torch.round(torch.relu(torch.randn(N, H, W, C, generator=gen)) * 2) / 2   # a few levels after a ReLU: most windows hold ties
            dy = 1e-3 * torch.randn(N, H // 2, W // 2, C, generator=gen)
            pool64, dx64 = R.maxpool(x, dy, F64)
            dx0 = 1e-3 * torch.randn(N, H, W, C, generator=gen)   # dx is ACCUMULATED (the stem's output is also the decoders' first skip)
            largest = max(float(dy.abs().max()), float(dx0.abs().max()))
            xd, dyd = x.cuda(), dy.cuda()
            pool, idx = D.Guarded((N, H // 2, W // 2, C)), D.Guarded((N, H // 2, W // 2, C // 4), dtype=torch.int32)
            D.ok(L.cerb_dev_maxpool_idx(D.ptr(xd), D.ptr(pool), D.ptr(idx), N, H, W, C, D.stream()), case)
            rep.equal(case, "pooled map", pool.cpu(), pool64.to(F32))
            dx = D.Guarded((N, H, W, C), dx0)
            D.ok(L.cerb_dev_maxpool_bwd_idx(D.ptr(idx), D.ptr(dyd), D.ptr(dx), N, H, W, C, D.stream()), case)
            rep.within_ulps(case, "dx by recorded positions", dx.cpu(), dx0.to(F64) + dx64, largest)
            dx2 = D.Guarded((N, H, W, C), dx0)
            D.ok(L.cerb_dev_maxpool_bwd(D.ptr(xd), D.ptr(pool), D.ptr(dyd), D.ptr(dx2), N, H, W, C, D.stream()), case)
            rep.within_ulps(case, "dx by the scan", dx2.cpu(), dx0.to(F64) + dx64, largest)
            # routing: without the start values the gradient of an element is a sum of whole dy values -- where torch routes nothing the kernel adds nothing
            rep.check(torch.equal((dx.cpu() != dx0), (dx64 != 0)) and torch.equal((dx2.cpu() != dx0), (dx64 != 0)), case, "gradient reaches exactly torch's elements")
            rep.intact(case, pool, idx, dx, dx2)
    rep.finish()


# =====================================================================================================================================================
K_POINTWISE = 8
PW_ROWS = (64, 511, 512, 513, 4097)
PW_SHAPES = ((64, 96), (96, 3), (96, 7), (512, 256))


def _pw_inputs(rows, cin, cout, scaled, gen):
    x = torch.relu(torch.randn(rows, cin, generator=gen))
    dy = 1e-3 * torch.randn(rows, cout, generator=gen)
    w = torch.randn(cout, cin, generator=gen) / cin ** 0.5
    scale = (2.0 * (torch.rand(rows, cin, generator=gen) < 0.5).to(F32)) if scaled else None   # a dropout mask * 1 / (1 - p)
    return x, dy, w, scale


@dev_switches
def test_pointwise_backward_vs_float64_matmul():
    L, rep, gen = D.lib(), Report("pointwise", K_POINTWISE), _gen(19)
    for rows in PW_ROWS:
        for cin, cout in PW_SHAPES:
            for scaled in (0, 1):
                for assign in (0, 1):
                    case = (rows, cin, cout, "scale" if scaled else "-", "dx=" if assign else "dx+=")
                    x, dy, w, scale = _pw_inputs(rows, cin, cout, scaled, gen)
                    dx64, dw64, db64 = R.pointwise_grads(x, dy, w, scale, F64)
                    dx32, dw32, db32 = R.pointwise_grads(x, dy, w, scale, F32)
                    dx0 = None if assign else _acc_init(dx64, gen)
                    dev = [t.cuda() for t in (x, dy, w)]
                    sd = scale.cuda() if scaled else None
                    dx, dw, db = D.Guarded((rows, cin), dx0), D.Guarded((cout, cin)), D.Guarded((cout,))
                    D.ok(L.cerb_dev_pointwise_bwd(D.ptr(dev[0]), D.ptr(dev[1]), D.ptr(dev[2]), D.ptr(dx), D.ptr(dw), D.ptr(db), rows, cin, cout, D.ptr(sd), assign, D.stream()), case)
                    rep.bar(case, "dx", dx.cpu(), dx64 if assign else dx0.to(F64) + dx64, dx32 if assign else dx0 + dx32)
                    rep.bar(case, "dw", dw.cpu(), dw64, dw32)
                    rep.bar(case, "db", db.cpu(), db64, db32)
                    rep.intact(case, dx, dw, db)
    # the heads' last layers (<= 8 outputs): the one-pass backward and the weight gradient on its own
    for rows in PW_ROWS:
        for cin, cout in ((96, 3), (96, 7)):
            for assign in (0, 1):
                case = (rows, cin, cout, "small", "dx=" if assign else "dx+=")
                x, dy, w, _ = _pw_inputs(rows, cin, cout, 0, gen)
                dx64, dw64, db64 = R.pointwise_grads(x, dy, w, None, F64)
                dx32, dw32, db32 = R.pointwise_grads(x, dy, w, None, F32)
                dx0 = None if assign else _acc_init(dx64, gen)
                dev = [t.cuda() for t in (x, dy, w)]
                dx, dw, db = D.Guarded((rows, cin), dx0), D.Guarded((cout, cin)), D.Guarded((cout,))
                ws = D.workspace(L.cerb_dev_pw_bwd_small_workspace_bytes(rows, cin, cout))
                D.ok(L.cerb_dev_pw_bwd_small(D.ptr(dev[0]), D.ptr(dev[1]), D.ptr(dev[2]), D.ptr(dx), D.ptr(dw), D.ptr(db), rows, cin, cout, assign, D.ptr(ws), D.stream()), case)
                rep.bar(case, "dx", dx.cpu(), dx64 if assign else dx0.to(F64) + dx64, dx32 if assign else dx0 + dx32)
                rep.bar(case, "dw", dw.cpu(), dw64, dw32)
                rep.bar(case, "db", db.cpu(), db64, db32)
                rep.intact(case, dx, dw, db, ws)
                if assign:
                    dw2, ws2 = D.Guarded((cout, cin)), D.workspace(L.cerb_dev_pw_wgrad_small_workspace_bytes(rows, cin, cout))
                    D.ok(L.cerb_dev_pw_wgrad_small(D.ptr(dev[0]), D.ptr(dev[1]), D.ptr(dw2), rows, cin, cout, D.ptr(ws2), D.stream()), case)
                    rep.bar(case, "dw (pw_wgrad_small)", dw2.cpu(), dw64, dw32)
                    rep.intact(case, dw2, ws2)
    # more than 8 outputs are not theirs: an error, not a launch
    t = torch.zeros(1 << 16, device="cuda")
    rep.check(L.cerb_dev_pw_bwd_small(D.ptr(t), D.ptr(t), D.ptr(t), D.ptr(t), D.ptr(t), D.ptr(t), 64, 96, 9, 1, D.ptr(t), D.stream()) != 0, "cout 9", "pw_bwd_small refuses")
    rep.check(L.cerb_dev_pw_wgrad_small(D.ptr(t), D.ptr(t), D.ptr(t), 64, 96, 9, D.ptr(t), D.stream()) != 0, "cout 9", "pw_wgrad_small refuses")
    torch.cuda.synchronize()
    rep.finish()


# =====================================================================================================================================================
K_SMALL = 6


@dev_switches
def test_colsum_crop_gap_dilate2_vs_float64():
    L, rep, gen = D.lib(), Report("small", K_SMALL), _gen(20)
    # column sums (bias gradients): a small grouped case, a ragged one (8 slabs, the last one short, 96 channels) and one below the slab threshold
    for G, rows, C in ((5, 33, 64), (1, 4097, 96), (3, 2047, 512)):
        d = 1e-3 * torch.randn(G, rows, C, generator=gen)
        dd = d.cuda()
        out, ws = D.Guarded((G, C)), D.workspace(L.cerb_dev_colsum_workspace_bytes(C, G))
        D.ok(L.cerb_dev_colsum(D.ptr(dd), rows * C, rows, C, G, D.ptr(out), D.ptr(ws), D.stream()), (G, rows, C))
        rep.bar((G, rows, C), "colsum", out.cpu(), R.colsum(d, F64), R.colsum(d, F32))
        rep.intact((G, rows, C), out, ws)
    # centre crop + global average pool and its backward: 9 x 9 out of 10 x 12, and the uncropped 3 x 5 map
    for N, H, W, C, y0, ch, x0, cw in ((2, 10, 12, 512, 0, 9, 1, 9), (3, 3, 5, 64, 0, 3, 0, 5)):
        case = (N, H, W, C, "window %d:%d x %d:%d" % (y0, y0 + ch, x0, x0 + cw))
        x = torch.relu(torch.randn(N, H, W, C, generator=gen))
        dg = 1e-3 * torch.randn(N, C, generator=gen)
        o64, dx64 = R.crop_gap(x, dg, y0, ch, x0, cw, F64)
        o32, dx32 = R.crop_gap(x, dg, y0, ch, x0, cw, F32)
        dx0 = _acc_init(dx64, gen)   # dx is ACCUMULATED
        xd, dgd = x.cuda(), dg.cuda()
        out, dx = D.Guarded((N, C)), D.Guarded((N, H, W, C), dx0)
        D.ok(L.cerb_dev_crop_gap(D.ptr(xd), N, H, W, C, y0, ch, x0, cw, D.ptr(out), D.stream()), case)
        D.ok(L.cerb_dev_crop_gap_bwd(D.ptr(dgd), D.ptr(dx), N, H, W, C, y0, ch, x0, cw, D.stream()), case)
        rep.bar(case, "crop_gap", out.cpu(), o64, o32)
        rep.bar(case, "crop_gap_bwd", dx.cpu(), dx0.to(F64) + dx64, dx0 + dx32)
        rep.check(torch.equal(dx.cpu()[dx64 == 0], dx0[dx64 == 0]), case, "nothing added outside the window")
        rep.intact(case, out, dx)
    # stride-2 dilation (exact): grouped, and a ragged one (2 x 2 output, 96 channels)
    for n, H, W, C in ((5, 6, 10, 64), (3, 2, 2, 96), (2, 16, 12, 512)):
        dy = torch.randn(n, H // 2, W // 2, C, generator=gen)
        dyd = dy.cuda()
        d = D.Guarded((n, H, W, C))
        D.ok(L.cerb_dev_dilate2(D.ptr(dyd), D.ptr(d), n, H, W, C, D.stream()), (n, H, W, C))
        rep.equal((n, H, W, C), "dilate2", d.cpu(), R.dilate2(dy))
        rep.intact((n, H, W, C), d)
    rep.check(L.cerb_dev_dilate2(D.ptr(dyd), D.ptr(d), 1, 3, 4, 64, D.stream()) != 0, "odd H", "dilate2 refuses")
    rep.finish()
