"""Kernel-level parity of the forward convolutions: every launcher (cerb_launch_conv, cerb_launch_wino, cerb_launch_wino4, cerb_launch_wino4b,
cerb_launch_wino4p) on its own, through cerb_devfwd_conv of the developers' library (tests/dev_kernels.py), against F.conv2d in float64 on the same inputs
(tests/kernel_refs.py: conv_forward) at the smallest shapes that reach the kernel's edges -- and the data-gradient use of the same kernels exactly as
cerb_train.hip launches it (device packers with dgrad = 1, zero bias with bias_gs = 0, relu = 0, the residual aliased to the output, the dilate2 pre-pass).

Per output tensor err(a) = max|a - ref64| / max|ref64|, and a launch passes when err(kernel) <= K * err(yardstick) + 1e-7.  The yardstick of the direct
kernel is conv2d in float32; that of the Winograd launchers is a plain float32 evaluation of THEIR algorithm (kernel_refs.wino_forward_formula: F(4x4) in
float32 is 13 .. 40 times noisier than the direct sum, a direct yardstick would fail a correct kernel or need a K that hides defects).  K per family is at
least twice the worst err(kernel) / err(yardstick) measured on the MI355X and never below 4 (table: DESIGN.md, "kernel-level parity of the forward
convolutions").  The protections of tests/test_kernel_parity_gpu.py apply: outputs between sentinel bands, assigned outputs start as NaN, the in-place
residual starts from random values, NHWC inputs carry the schedule's zero guard band.  One function per family, every figure printed; each function ends
with its refusals and with sensitivity controls: references made wrong on purpose (16 input channels dropped, replicate padding on one border, the taps
rotated, the residual left out) must miss the bar of the very outputs that passed it."""
import ctypes as C

import pytest
import torch

import dev_kernels as D
import kernel_refs as R
from conftest import dev_switches
from test_kernel_parity_gpu import K_BN, Report, _acc_init, _gen

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
IGEMM, WINO, WINO4, WINO4B, WINO4P = 0, 1, 2, 3, 4
NAMES = {IGEMM: "conv_igemm", WINO: "conv_wino", WINO4: "conv_wino4", WINO4B: "conv_wino4b", WINO4P: "conv_wino4p"}


def _band(t, W, ch):
    """the schedule's guard band, sized for the rows of THIS tensor (cerb_conv_guard_bytes counts 64-channel rows of a tile-wide map; the stride-2 tiles of
    conv_igemm read up to 33 rows past a small map): twice 17 rows of W x ch floats"""
    return D.banded(t, 2 * W * max(ch, 64) // 64)


class Launch(object):
    """One call of cerb_devfwd_conv.  x [Gx][N][H][W][Cin] (Gx = 1 with G > 1: in_gs = 0), w raw [G][Cout][Cin][k][k] (dgrad: the forward layer's tensor,
    the launch's Cin = w.shape[1]), bias [Gb][Cout] (Gb = 1 with G > 1: bias_gs = 0), resid [G][N][Ho][Wo][Cout] out of place, inplace = start values of
    the output that is its own residual, prev [Gp][N][H/2][W/2][Cin] (mode 1).  launcher WINO4P: tensors travel tile-planar, .got comes back NHWC and
    .ring_ok says that every float no pixel maps to is still zero."""

    def __init__(self, L, launcher, x, w, bias, resid=None, inplace=None, prev=None, ks=3, stride=1, relu=1, tag=0, host_pack=0, dgrad=0, roi=None, pk_off=0,
                 bn_blocks=0, pl_adj=(0, 0), x_dev=None):
        G = w.shape[0]
        Gx, N, H, W, Ci = x.shape
        Co = w.shape[2] if dgrad else w.shape[1]
        assert Ci == (w.shape[1] if dgrad else w.shape[2]) and bias.shape[1] == Co and Gx in (1, G) and bias.shape[0] in (1, G)
        Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
        planar = launcher == WINO4P
        self.bufs, self.ring_ok, self.bn = [], True, None
        bd = bias.cuda().contiguous()
        wd = w.cuda().contiguous()
        pd, prev_gs = None, 0
        if planar:
            size_i = D._planar_idx(N, H, W, Ci)[1]
            idx_o, size_o = D._planar_idx(N, Ho, Wo, Co)
            assert size_o == L.cerb_devfwd_planar_elems(N, Ho, Wo, Co)
            xd = D.banded(torch.cat([D._to_planar(x[g].cuda()) for g in range(Gx)]), 64)
            in_gs, out_gs = size_i, size_o
            out = D.Guarded((G * size_o,), init=torch.zeros(G * size_o))   # the guard ring and the pixels beyond the image are DATA: zero, and they stay zero
            ov = out.t.view(G, size_o)
            for g in range(G):
                ov[g][idx_o] = float("nan") if inplace is None else inplace[g].cuda()
            rd = None if resid is None else torch.cat([D._to_planar(resid[g].cuda()) for g in range(G)])
            byp, bxp = (Ho + 15) // 16 + 2 + pl_adj[0], (Wo + 15) // 16 + 2 + pl_adj[1]
        else:
            xd = x_dev if x_dev is not None else _band(x.cuda(), W, Ci)
            in_gs, out_gs = N * H * W * Ci, N * Ho * Wo * Co
            out = D.Guarded((G, N, Ho, Wo, Co), init=inplace)
            rd = None if resid is None else resid.cuda().contiguous()
            byp, bxp = pl_adj   # (conv_igemm's planar epilogue is asked for by non-zero block counts)
            if prev is not None:
                pd, prev_gs = _band(prev.cuda(), W // 2, Ci), (0 if prev.shape[0] == 1 and G > 1 else N * (H // 2) * (W // 2) * Ci)
        if Gx == 1 and G > 1:
            in_gs = 0
        resid_gs = out_gs
        if dgrad and G == 1:
            resid_gs = out_gs = 0   # as cerb_train.hip passes them
        part = None
        if bn_blocks:
            part = D.Guarded((G * bn_blocks * Co * 4,))   # [G][blocks][Cout][(sum, sum of squares)] doubles, ASSIGNED
            self.bufs.append(part)
        self.bufs.append(out)
        roi_c = None if roi is None else (C.c_int * 4)(*roi)
        res_ptr = D.ptr(out) if inplace is not None else D.ptr(rd)
        self.rc = L.cerb_devfwd_conv(launcher, ks, stride, 1 if prev is not None else 0, tag, D.ptr(wd), host_pack, dgrad, D.ptr(xd), D.ptr(pd), D.ptr(bd), res_ptr, D.ptr(out),
                                     D.ptr(part), G, N, H, W, Ci, Co, relu, in_gs, prev_gs, 0 if bias.shape[0] == 1 and (G > 1 or dgrad) else Co, resid_gs, out_gs, roi_c, pk_off, byp, bxp,
                                     D.stream())
        torch.cuda.synchronize()
        self.out = out
        if planar:
            self.got = torch.stack([ov[g][idx_o] for g in range(G)]).cpu()
            written = torch.zeros(size_o, dtype=torch.bool, device="cuda")
            written[idx_o.reshape(-1)] = True
            self.ring_ok = bool((ov[:, ~written] == 0).all())
            if rd is not None:
                self.ring_ok = self.ring_ok and torch.equal(rd, torch.cat([D._to_planar(resid[g].cuda()) for g in range(G)]))   # the residual is only read
        else:
            self.got = out.cpu()
        if part is not None:
            self.bn = part.t.view(torch.float64).view(G, bn_blocks, Co, 2)

    def intact(self):
        return all(b.intact() for b in self.bufs)


def _inputs(gen, G, Gx, N, H, W, Ci, Co, ks=3, stride=1, resid=False, Gp=0, Gb=None):
    """x = relu(randn), w = randn / (k sqrt(Cin)), bias = 0.1 randn, resid = randn (prev of mode 1 as x)"""
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    x = torch.relu(torch.randn(Gx, N, H, W, Ci, generator=gen))
    w = torch.randn(G, Co, Ci, ks, ks, generator=gen) / (ks * Ci ** 0.5)
    bias = 0.1 * torch.randn(G if Gb is None else Gb, Co, generator=gen)
    r = torch.randn(G, N, Ho, Wo, Co, generator=gen) if resid else None
    prev = torch.relu(torch.randn(Gp, N, H // 2, W // 2, Ci, generator=gen)) if Gp else None
    return x, w, bias, r, prev


def _yard(launcher, x, w, bias, resid, prev, ks, stride, relu):
    if launcher == IGEMM:
        return R.conv_forward(x, w, bias, resid, prev, ks, stride, relu, F32)
    return R.conv_epilogue(R.wino_forward_formula(x, w, 2 if launcher == WINO else 4, F32), bias, resid, relu, F32)


def _altered(kind, x, w, bias, resid, prev, ks, stride, relu):
    """a float64 reference made wrong in a way a kernel could fail"""
    if kind == "last 16 input channels dropped":
        return R.conv_forward(x[..., :-16], w[:, :, :-16], bias, resid, None if prev is None else prev[..., :-16], ks, stride, relu, F64)
    if kind == "taps rotated by 180 degrees":
        return R.conv_forward(x, w.flip(-1, -2), bias, resid, prev, ks, stride, relu, F64)
    if kind == "residual left out":
        return R.conv_forward(x, w, bias, None, prev, ks, stride, relu, F64)
    assert kind == "replicate padding on the left border" and stride == 1 and prev is None
    y = R.conv_forward(torch.cat([x[:, :, :, :1], x], 3), w, None, None, None, ks, 1, 0, F64)[:, :, :, 1:]   # column 0 sees a copy of itself on its left
    return R.conv_epilogue(y, bias, resid, relu, F64)


def _controls(rep, case, got, ref64, yard, alts):
    """sensitivity: the kernel's output against each altered reference must MISS the bar the true reference set (K has not grown past such defects)"""
    thr = rep.k * R.err(yard, ref64) + 1e-7
    for kind, alt in alts:
        miss = R.err(got, alt)
        print("%s %s control, %s: err %.3e = %.0f x the bar %.3e" % (rep.family, case, kind, miss, miss / thr, thr))
        rep.check(miss > thr, case, "control must miss the bar: " + kind)


def _relu_cuts(rep, case, ref64):
    z = float((ref64 == 0).double().mean())
    rep.check(0.2 <= z <= 0.8, case, "the ReLU must cut between 20 %% and 80 %% of the reference (%.2f): change the seed" % z)


def _roi_bar(rep, case, got, ref64, yard, roi):
    """inside the region the output meets the bar; outside it every element is still NaN or meets the same bar (whole items are computed).
    Returns how many elements outside the region are still NaN: the caller asserts the exact count its region leaves (at least one, or the case does not
    test the region)"""
    y0, y1, x0, x1 = roi
    inside = torch.zeros(got.shape, dtype=torch.bool)
    inside[:, :, y0:y1, x0:x1, :] = True
    nan = torch.isnan(got)
    rep.check(not bool(nan[inside].any()), case, "every element inside the region is computed")
    rep.bar(case, "inside the region", got[:, :, y0:y1, x0:x1, :], ref64[:, :, y0:y1, x0:x1, :], yard[:, :, y0:y1, x0:x1, :])
    rep.bar(case, "whatever was computed", torch.where(nan, ref64.to(F32), got), ref64, yard)
    left = int(nan[~inside].sum())
    print("%s %s: %d of %d elements outside the region left untouched" % (rep.family, case, left, int((~inside).sum())))
    return left


def _conv_case(L, rep, gen, launcher, G, Gx, N, H, W, Ci, Co, ks=3, stride=1, relu=1, resid=False, inplace=False, Gp=0, Gb=None, tag=0, roi=None, pk_off=0, host_pack=0,
               note=""):
    """one launch against float64 conv2d; returns what the controls and the packer comparison need"""
    case = (NAMES[launcher] + (" tag %d" % tag if launcher == WINO4P else ""), "G%d%s N%d %dx%d %d->%d k%d s%d" % (G, "(shared in)" if Gx < G else "", N, H, W, Ci, Co, ks, stride),
            "relu %d" % relu + (" resid" if resid else "") + (" in place" if inplace else "") + (" prev x%d" % Gp if Gp else "") + (" roi" if roi else "") +
            (" pk_off" if pk_off else "") + (" host pack" if host_pack else "") + note)
    x, w, bias, r, prev = _inputs(gen, G, Gx, N, H, W, Ci, Co, ks, stride, resid or inplace, Gp, Gb)
    ref64 = R.conv_forward(x, w, bias, r, prev, ks, stride, relu, F64)
    yard = _yard(launcher, x, w, bias, r, prev, ks, stride, relu)
    if relu:
        _relu_cuts(rep, case, ref64)
    run = Launch(L, launcher, x, w, bias, resid=None if inplace else r, inplace=r if inplace else None, prev=prev, ks=ks, stride=stride, relu=relu, tag=tag, roi=roi,
                 pk_off=pk_off, host_pack=host_pack)
    rep.check(run.rc == 0, case, "hipError %d" % run.rc)
    left = None
    if roi is None:
        rep.bar(case, "out", run.got, ref64, yard)
    else:
        left = _roi_bar(rep, case, run.got, ref64, yard, roi)
    rep.check(run.intact(), case, "sentinel bands")
    rep.check(run.ring_ok, case, "guard ring and the floats no pixel maps to stay zero; the residual is only read")
    return dict(case=case, got=run.got, ref64=ref64, yard=yard, args=(x, w, bias, r, prev, ks, stride, relu), left=left)


def _refused(L, rep, what, launcher, x, w, bias, **kw):
    """the entry returns an error and launches nothing: the NaN output is untouched"""
    run = Launch(L, launcher, x, w, bias, **kw)
    rep.check(run.rc != 0, (NAMES[launcher], what), "must be refused")
    rep.check(bool(torch.isnan(run.got).all()) and run.intact(), (NAMES[launcher], what), "a refused launch writes nothing")
    print("%s refusal, %s %s: hipError %d" % (rep.family, NAMES[launcher], what, run.rc))


def _packers(L, rep, gen, launcher, G, N, H, W, Ci, Co, **kw):
    """the same case on host-packed and on device-packed weights: both meet the bar; the largest difference between the two outputs is printed"""
    state = gen.get_state()
    a = _conv_case(L, rep, gen, launcher, G, G, N, H, W, Ci, Co, host_pack=0, **kw)
    gen.set_state(state)
    b = _conv_case(L, rep, gen, launcher, G, G, N, H, W, Ci, Co, host_pack=1, **kw)
    d = (a["got"].double() - b["got"].double()).abs()
    print("%s %s packers: largest |device-packed - host-packed| = %.3e" % (rep.family, a["case"][:2], float(d[torch.isfinite(d)].max()) if bool(torch.isfinite(d).any()) else float("nan")))
    return a


def _finish_all(*reps):
    """every report prints its summary line before any of them fails: one run shows every family's ratios and the union of the misses"""
    failed = []
    for r in reps:
        try:
            r.finish()
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, " || ".join(failed)


ALL_CONTROLS = ("last 16 input channels dropped", "replicate padding on the left border", "taps rotated by 180 degrees", "residual left out")


def _run_controls(rep, c):
    x, w, bias, r, prev, ks, stride, relu = c["args"]
    assert r is not None and ks == 3 and stride == 1 and prev is None
    _controls(rep, c["case"], c["got"], c["ref64"], c["yard"], [(k, _altered(k, *c["args"])) for k in ALL_CONTROLS])


# =====================================================================================================================================================
K_IGEMM = 9   # measured 4.40 (3x3, Cin = 128; at most 1.18 at 1x1): an element's 9 x Cin = 1152 products are added in ONE float32 accumulator chain of the matrix
              # pipe, two per step in ascending channel order, where conv2d's float32 sums in blocks -- the longer rounding chain of K_CONV_BWD, not a defect


@dev_switches
def test_igemm_vs_float64_conv2d():
    """conv_igemm: 16 x 16 tiles when Wo < 32, else 8 x 32; chunks of 32 channels at stride 1, 16 at stride 2"""
    L, rep, gen = D.lib(), Report("conv_igemm", K_IGEMM), _gen(21)
    # stride 1, ks 3 and 1: odd and tiny maps, one exact tile, Wo on both sides of the tile switch with a tile hanging over
    for i, (H, W) in enumerate(((5, 7), (16, 16), (9, 33), (8, 32))):
        ca, cb = ((64, 128), (128, 64)) if i % 2 == 0 else ((128, 64), (64, 128))
        _conv_case(L, rep, gen, IGEMM, 1, 1, 2, H, W, ca[0], ca[1], ks=3)
        _conv_case(L, rep, gen, IGEMM, 1, 1, 2, H, W, cb[0], cb[1], ks=1)
    _conv_case(L, rep, gen, IGEMM, 3, 3, 2, 5, 7, 64, 64, ks=3)            # three groups, own inputs
    _conv_case(L, rep, gen, IGEMM, 3, 1, 2, 16, 16, 64, 64, ks=3)          # ... and one shared input (in_gs = 0)
    ctl = _conv_case(L, rep, gen, IGEMM, 1, 1, 2, 9, 33, 64, 64, ks=3, resid=True)
    _conv_case(L, rep, gen, IGEMM, 1, 1, 2, 8, 32, 64, 64, ks=3, relu=0)
    _conv_case(L, rep, gen, IGEMM, 2, 2, 1, 5, 7, 128, 64, ks=1, relu=0, resid=True)
    # stride 2 (rows 2 yo - 1 + ky at the top and left border), NHWC output; 80 input channels: five 16-channel chunks
    for H, W in ((10, 14), (32, 32), (64, 80)):
        _conv_case(L, rep, gen, IGEMM, 1, 1, 2, H, W, 64, 128, ks=3, stride=2)
        _conv_case(L, rep, gen, IGEMM, 1, 1, 2, H, W, 64, 128, ks=1, stride=2, relu=0)
    _conv_case(L, rep, gen, IGEMM, 1, 1, 2, 10, 14, 80, 64, ks=3, stride=2)
    # mode 1: input = skip + bilinear x2 of prev; skip shared, prev per group and shared; the clamped taps dominate at 4 x 6; 6 x 34: the 8 x 32 tiles
    for H, W, Gp in ((4, 6, 2), (16, 16, 1), (16, 16, 2), (4, 6, 1), (6, 34, 2)):
        _conv_case(L, rep, gen, IGEMM, 2, 1, 2, H, W, 64, 64, Gp=Gp)
    _packers(L, rep, gen, IGEMM, 1, 2, 9, 33, 64, 128, ks=3)
    _packers(L, rep, gen, IGEMM, 1, 2, 10, 14, 64, 64, ks=1, stride=2)
    # refusals
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 8, 8, 48, 64)
    _refused(L, rep, "Cin = 48 at stride 1 (chunks of 32)", IGEMM, x, w, bias)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 8, 8, 64, 96)
    _refused(L, rep, "Cout = 96", IGEMM, x, w, bias)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 8, 8, 72, 64, ks=1, stride=2)
    _refused(L, rep, "Cin = 72 at stride 2 (chunks of 16)", IGEMM, x, w, bias, ks=1, stride=2)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 16, 16, 64, 64)
    _refused(L, rep, "a region of interest", IGEMM, x, w, bias, roi=(0, 8, 0, 8))
    _refused(L, rep, "a tile-planar output at stride 1", IGEMM, x, w, bias, pl_adj=(3, 3))
    _run_controls(rep, ctl)
    rep.finish()


# =====================================================================================================================================================
K_WINO2 = 4   # measured 1.95 against the float32 F(2x2) formula (512 -> 512 on 7 x 7; below 1.3 at 64 and 96 input channels)


@dev_switches
def test_wino_f2x2_vs_float64_conv2d():
    """conv_wino: items of 8 x 16 output pixels, chunks of 32 input channels"""
    L, rep, gen = D.lib(), Report("conv_wino", K_WINO2), _gen(22)
    # odd maps, one partial item, an exact item, an item hanging over on both sides
    for i, (H, W) in enumerate(((3, 5), (7, 7), (8, 16), (14, 14), (9, 17))):
        _conv_case(L, rep, gen, WINO, 1, 1, 2, H, W, 64, 64, resid=bool(i % 2))
    _conv_case(L, rep, gen, WINO, 1, 1, 2, 3, 5, 512, 512, resid=True)
    _conv_case(L, rep, gen, WINO, 1, 1, 2, 7, 7, 512, 512)
    _conv_case(L, rep, gen, WINO, 1, 1, 2, 14, 14, 96, 64)
    ctl = _conv_case(L, rep, gen, WINO, 1, 1, 2, 9, 17, 96, 64, resid=True)
    _conv_case(L, rep, gen, WINO, 2, 2, 2, 7, 7, 64, 64, resid=True)
    _conv_case(L, rep, gen, WINO, 2, 1, 2, 9, 17, 64, 64)
    _conv_case(L, rep, gen, WINO, 1, 1, 2, 8, 16, 64, 128, relu=0, resid=True)
    # region of interest on 24 x 40.  [5, 19) x [9, 33) overlaps every 8 x 16 item of the map (item rows 0..2, columns 0..2): nothing stays NaN, the case
    # pins the item offsets only through the bar.  [9, 15) x [17, 31) lies inside item (1, 1): the eight items around it must stay untouched.
    c = _conv_case(L, rep, gen, WINO, 1, 1, 2, 24, 40, 64, 64, roi=(5, 19, 9, 33))
    rep.check(c["left"] == 0, c["case"], "this region overlaps every item of the map")
    c = _conv_case(L, rep, gen, WINO, 1, 1, 2, 24, 40, 64, 64, roi=(9, 15, 17, 31))
    rep.check(c["left"] == 2 * (24 * 40 - 8 * 16) * 64, c["case"], "exactly the items outside the region stay NaN")
    _packers(L, rep, gen, WINO, 2, 2, 9, 17, 64, 64)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 8, 8, 48, 64)
    _refused(L, rep, "Cin = 48", WINO, x, w, bias)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 8, 8, 64, 96)
    _refused(L, rep, "Cout = 96", WINO, x, w, bias)
    _run_controls(rep, ctl)
    rep.finish()


# =====================================================================================================================================================
K_WINO4 = 5   # measured 2.49 against the float32 F(4x4) formula (512 -> 512 on 16 x 16, conv_wino4; conv_wino4b 2.37; below 1.4 up to 128 input channels)


def _bn_case(L, rep, gen, launcher, G, N, H, W, Ci, Co, pk_off):
    """the BatchNorm partials the output stage leaves (bn_part), folded by cerb_dev_bn_finalize, against the float64 statistics of the kernel's own output"""
    case = (NAMES[launcher], "bn_part G%d N%d %dx%d %d->%d%s" % (G, N, H, W, Ci, Co, " pk_off" if pk_off else ""))
    x, w, bias, _, _ = _inputs(gen, G, G, N, H, W, Ci, Co)
    blocks = L.cerb_devfwd_wino4b_bn_blocks(N, H, W, Ci, Co, pk_off) if launcher == WINO4B else N * ((H + 15) // 16) * ((W + 15) // 16)
    run = Launch(L, launcher, x, w, bias, relu=0, pk_off=pk_off, bn_blocks=blocks)
    rep.check(run.rc == 0 and run.intact(), case, "hipError %d / sentinel bands" % run.rc)
    rows = N * H * W
    y = run.got.view(G, rows, Co)
    ref64, ref32 = R.bn_stats(y, F64), R.bn_stats(y, F32)
    out = [D.Guarded((G, Co)) for _ in range(3)]
    fold = D.workspace(L.cerb_dev_bn_fold_workspace_bytes(G, Co))
    D.ok(L.cerb_dev_bn_finalize(D.ptr(run.bn), blocks, rows, Co, 1e-5, D.ptr(out[0]), D.ptr(out[1]), D.ptr(out[2]), G, D.ptr(fold), D.stream()), case)
    for i, name in enumerate(("mean", "rstd", "var_unbiased")):
        rep.bar(case + ("%d partial rows" % blocks,), name, out[i].cpu(), ref64[i], ref32[i])
    rep.intact(case, fold, *out)


@dev_switches
def test_wino_f4x4_nhwc_vs_float64_conv2d():
    """conv_wino4 (items of two 16 x 16 blocks, chunks of 16 channels) and conv_wino4b (one block or 16 packed tiles per item, chunks of 32)"""
    L, rep, rep_bn, gen = D.lib(), Report("conv_wino4/4b", K_WINO4), Report("conv_wino4/4b bn_part", K_BN), _gen(23)
    ctl = []   # one control case per launcher: conv_wino4b chunks the input channels by 32, conv_wino4 by 16
    for launcher in (WINO4, WINO4B):
        # block form: one block, an odd block count (conv_wino4's last pair repeats a block), tiles and blocks hanging over the map
        _conv_case(L, rep, gen, launcher, 1, 1, 1, 16, 16, 64, 64, pk_off=1)
        _conv_case(L, rep, gen, launcher, 1, 1, 3, 16, 16, 64, 128, pk_off=1, resid=True)
        ctl.append(_conv_case(L, rep, gen, launcher, 1, 1, 2, 18, 22, 128, 64, pk_off=1, resid=True))
        _conv_case(L, rep, gen, launcher, 1, 1, 1, 32, 48, 64, 64, pk_off=1)
        _conv_case(L, rep, gen, launcher, 1, 1, 3, 16, 16, 512, 512, pk_off=1, inplace=True)
        _conv_case(L, rep, gen, launcher, 1, 1, 1, 16, 16, 128, 64, pk_off=1, relu=0)
        _conv_case(L, rep, gen, launcher, 5, 1, 1, 16, 16, 64, 64, pk_off=1)                 # five groups on one input (in_gs = 0)
        # maps that conv_wino4b serves with packed items (pk_off = 0): 15 tiles per image (items straddle images: the halo of a tile at the top of image
        # n + 1 must not read image n), 49 tiles (the last item is partial), two groups
        _conv_case(L, rep, gen, launcher, 1, 1, 3, 12, 20, 64, 64, resid=True)
        _conv_case(L, rep, gen, launcher, 1, 1, 3, 12, 20, 64, 64, inplace=True)
        _conv_case(L, rep, gen, launcher, 1, 1, 1, 28, 28, 64, 128)
        _conv_case(L, rep, gen, launcher, 2, 2, 1, 20, 16, 128, 64)
        c = _conv_case(L, rep, gen, launcher, 1, 1, 1, 48, 64, 64, 64, roi=(7, 41, 18, 50))
        rep.check(c["left"] == 48 * 16 * 64, c["case"], "exactly block column 0 stays NaN")
        _packers(L, rep, gen, launcher, 2, 2, 18, 22, 64, 64, resid=True)
    _packers(L, rep, gen, WINO4B, 1, 3, 12, 20, 64, 64)   # ... and the packed items
    for N, H, W, pk_off, want in ((3, 12, 20, 0, 1), (1, 28, 28, 0, 1), (1, 20, 16, 0, 1), (3, 12, 20, 1, 0), (1, 16, 16, 0, 0), (1, 32, 48, 0, 0), (2, 18, 22, 0, 0)):
        rep.check(L.cerb_devfwd_wino4b_packed(N, H, W, 64, 64, pk_off) == want, (N, H, W, pk_off), "cerb_wino4b_packed = %d" % want)
    # 16 input channels: the smallest count conv_wino4 accepts, conv_wino4b refuses
    _conv_case(L, rep, gen, WINO4, 1, 1, 2, 16, 16, 16, 64)
    _conv_case(L, rep, gen, WINO4, 1, 1, 1, 18, 22, 48, 64)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 16, 16, 16, 64)
    _refused(L, rep, "Cin = 16", WINO4B, x, w, bias)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 16, 16, 48, 64)
    _refused(L, rep, "Cin = 48", WINO4B, x, w, bias)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 16, 16, 64, 96)
    _refused(L, rep, "Cout = 96", WINO4, x, w, bias)
    _refused(L, rep, "Cout = 96", WINO4B, x, w, bias)
    x, w, bias, r, _ = _inputs(gen, 1, 1, 1, 16, 16, 64, 64, resid=True)
    run = Launch(L, WINO4B, x, w, bias, resid=r, bn_blocks=1)
    rep.check(run.rc != 0 and bool(torch.isnan(run.got).all()), "conv_wino4b", "bn_part with a residual must be refused")
    # BatchNorm partials: block and packed forms, an odd block count on conv_wino4, a map hanging over the block grid (pixels outside the image must not count)
    for launcher, G, N, H, W, Ci, Co, pk_off in ((WINO4B, 1, 3, 16, 16, 64, 64, 1), (WINO4B, 1, 3, 12, 20, 64, 64, 0), (WINO4B, 2, 1, 28, 28, 64, 128, 0),
                                                 (WINO4B, 1, 2, 18, 22, 64, 64, 0), (WINO4, 1, 3, 16, 16, 64, 64, 1), (WINO4, 2, 2, 18, 22, 64, 64, 1),
                                                 (WINO4B, 1, 3, 12, 20, 64, 64, 1)):
        _bn_case(L, rep_bn, gen, launcher, G, N, H, W, Ci, Co, pk_off)
    for c in ctl:
        _run_controls(rep, c)
    _finish_all(rep, rep_bn)


# =====================================================================================================================================================
K_WINO4P = 4   # measured 1.86 against the float32 F(4x4) formula (256 -> 128 on 16 x 16)


@dev_switches
def test_wino_f4x4_planar_vs_float64_conv2d():
    """conv_wino4p: tile-planar input and output (+ tile-planar residual, tag 4), items of two 16 x 16 blocks"""
    L, rep, gen = D.lib(), Report("conv_wino4p", K_WINO4P), _gen(24)
    _conv_case(L, rep, gen, WINO4P, 1, 1, 1, 16, 16, 64, 64, tag=0)
    _conv_case(L, rep, gen, WINO4P, 1, 1, 3, 16, 16, 256, 128, tag=1)            # three blocks: the last pair repeats one
    _conv_case(L, rep, gen, WINO4P, 1, 1, 1, 32, 48, 64, 64, tag=2)
    _conv_case(L, rep, gen, WINO4P, 1, 1, 2, 40, 40, 64, 64, tag=3)              # blocks hang over the map
    _conv_case(L, rep, gen, WINO4P, 5, 5, 1, 16, 16, 64, 64, tag=3)
    _conv_case(L, rep, gen, WINO4P, 5, 1, 1, 16, 16, 64, 64, tag=1, relu=0)      # five groups on one input
    ctl = _conv_case(L, rep, gen, WINO4P, 1, 1, 3, 16, 16, 64, 64, tag=4, resid=True)
    _conv_case(L, rep, gen, WINO4P, 1, 1, 3, 16, 16, 64, 64, tag=4, inplace=True)
    _conv_case(L, rep, gen, WINO4P, 1, 1, 1, 40, 40, 256, 128, tag=4, resid=True)
    _conv_case(L, rep, gen, WINO4P, 5, 5, 1, 40, 40, 64, 64, tag=4, inplace=True)
    _conv_case(L, rep, gen, WINO4P, 1, 1, 1, 32, 48, 64, 64, tag=4, inplace=True, relu=0)
    c = _conv_case(L, rep, gen, WINO4P, 1, 1, 1, 48, 64, 64, 64, tag=0, roi=(7, 41, 18, 50))
    rep.check(c["left"] == 48 * 16 * 64, c["case"], "exactly block column 0 stays NaN")
    _packers(L, rep, gen, WINO4P, 2, 2, 40, 40, 64, 64, tag=2)
    x, w, bias, r, _ = _inputs(gen, 1, 1, 1, 16, 16, 64, 64, resid=True)
    _refused(L, rep, "pl_byp off by one", WINO4P, x, w, bias, tag=3, pl_adj=(1, 0))
    _refused(L, rep, "pl_bxp off by one", WINO4P, x, w, bias, tag=3, pl_adj=(0, -1))
    _refused(L, rep, "a residual with tag 3", WINO4P, x, w, bias, tag=3, resid=r)
    _refused(L, rep, "tag 4 without a residual", WINO4P, x, w, bias, tag=4)
    x, w, bias, _, _ = _inputs(gen, 1, 1, 1, 16, 16, 64, 96)
    _refused(L, rep, "Cout = 96", WINO4P, x, w, bias, tag=3)
    _run_controls(rep, ctl)
    rep.finish()


# =====================================================================================================================================================
K_DGRAD = 4   # measured 1.25 against the float32 Winograd formula on the rotated, transposed filter


def _dgrad_case(L, rep, gen, launcher, G, N, H, W, Ci, Co, stride=1, pk_off=0):
    """dx of the forward layer x [G][N][H][W][Ci] -> y [..][Co] (3x3, stride 1 or 2) as cerb_train.hip computes it: the forward Winograd kernel on in = dy (after
    the dilate2 pre-pass at stride 2) with Cin / Cout swapped, weights from the device packer with dgrad = 1, zero bias with bias_gs = 0, relu = 0; once into
    a fresh output, once with resid == out (accumulate in place, resid_gs = out_gs)."""
    case0 = (NAMES[launcher], "dgrad G%d N%d %dx%d %d->%d s%d" % (G, N, H, W, Ci, Co, stride))
    Ho, Wo = (H // 2, W // 2) if stride == 2 else (H, W)
    x = torch.relu(torch.randn(G, N, H, W, Ci, generator=gen))
    dy = 1e-3 * torch.randn(G, N, Ho, Wo, Co, generator=gen)
    w = torch.randn(G, Co, Ci, 3, 3, generator=gen) / (3 * Ci ** 0.5)
    dx64 = R.conv_grads(x, dy, w, 3, stride, F64)[2]
    wd_ = R.dgrad_filter(w)
    m = 2 if launcher == WINO else 4
    zero = torch.zeros(1, Ci)
    if stride == 2:   # the pre-pass on the device, into a guard-banded buffer as net->t_dil is
        dil = _band(torch.full((G, N, H, W, Co), float("nan"), device="cuda"), W, Co)
        dyd = dy.cuda()
        D.ok(L.cerb_dev_dilate2(D.ptr(dyd), D.ptr(dil), G * N, H, W, Co, D.stream()), case0)
        din = torch.stack([R.dilate2(dy[g]) for g in range(G)])
        rep.equal(case0, "dilate2", dil, din)
    else:
        dil, din = None, dy
    yard = R.wino_forward_formula(din, wd_, m, F32)
    res = None
    for inplace in (False, True):
        case = case0 + ("resid == out" if inplace else "fresh",)
        dx0 = _acc_init(dx64, gen) if inplace else None
        run = Launch(L, launcher, din, w, zero, inplace=dx0, relu=0, dgrad=1, pk_off=pk_off, x_dev=dil)
        rep.check(run.rc == 0 and run.intact(), case, "hipError %d / sentinel bands" % run.rc)
        if inplace:
            rep.bar(case, "dx", run.got, dx0.to(F64) + dx64, dx0 + yard)
            res = dict(case=case, got=run.got, ref64=dx0.to(F64) + dx64, yard=dx0 + yard, dx0=dx0, din=din, w=w, dx64=dx64)
        else:
            rep.bar(case, "dx", run.got, dx64, yard)
    return res


@dev_switches
def test_data_gradient_on_the_forward_winograd_kernels_vs_float64_autograd():
    L, rep, gen = D.lib(), Report("dgrad", K_DGRAD), _gen(25)
    ctl = None
    for G in (1, 2):
        _dgrad_case(L, rep, gen, WINO, G, 2, 6, 10, 64, 128)
        _dgrad_case(L, rep, gen, WINO, G, 2, 8, 8, 64, 128)
        c = _dgrad_case(L, rep, gen, WINO4B, G, 2, 16, 16, 64, 128)
        ctl = ctl or c
        _dgrad_case(L, rep, gen, WINO4B, G, 2, 12, 20, 64, 128)          # packed items
        _dgrad_case(L, rep, gen, WINO4, G, 2, 32, 32, 64, 128)
    rep.check(L.cerb_devfwd_wino4b_packed(2, 12, 20, 128, 64, 0) == 1 and L.cerb_devfwd_wino4b_packed(2, 16, 16, 128, 64, 0) == 0, "conv_wino4b", "item forms of the dgrad cases")
    # the stride-2 composite: dilate2, then the stride-1 kernel, is dx of a 3x3 stride-2 convolution
    _dgrad_case(L, rep, gen, WINO4B, 1, 2, 16, 16, 64, 128, stride=2)
    _dgrad_case(L, rep, gen, WINO4B, 2, 2, 12, 20, 64, 128, stride=2)
    _dgrad_case(L, rep, gen, WINO, 1, 2, 12, 20, 64, 128, stride=2)
    _dgrad_case(L, rep, gen, WINO4, 2, 1, 16, 16, 64, 128, stride=2)
    # controls on the in-place 16 x 16 case
    din, w, dx0 = ctl["din"], ctl["w"], ctl["dx0"].to(F64)
    wd_ = R.dgrad_filter(w)
    fwd = lambda a, b: R.conv_forward(a, b, None, None, None, 3, 1, 0, F64)  # noqa: E731
    _controls(rep, ctl["case"], ctl["got"], ctl["ref64"], ctl["yard"], [
        ("last 16 input channels dropped", dx0 + fwd(din[..., :-16], wd_[:, :, :-16])),
        ("replicate padding on the left border", dx0 + fwd(torch.cat([din[:, :, :, :1], din], 3), wd_)[:, :, :, 1:]),
        ("taps not rotated", dx0 + fwd(din, w.transpose(1, 2).contiguous())),
        ("residual left out", ctl["dx64"])])
    rep.finish()
