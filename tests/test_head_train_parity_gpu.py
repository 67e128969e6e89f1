"""Kernel-level parity of the training step's output heads: cerb_launch_head_fwd1 / _fwd2 / _bwd1 / _bwd2 (head_train.hip), each on its own through the
cerb_dev_head_* entries of the developers' library, and the separate passes beside them (cerb_launch_pointwise, cerb_launch_bn_apply), against autograd in
float64 over the same chain (tests/kernel_refs.py: head_train_forward / head_train_backward, tied to the torch.nn modules by tests/test_kernel_refs.py):

    p = relu(bn_in(prev)) when the BatchNorm in front is handed in;  hid = p W1^T + b1;  z = relu(batch_norm(hid));  logits = z W2^T + b2

The `hid`, `mean`, `rstd`, `dgamma`, `dbeta` a kernel takes as inputs are float32 roundings of float64 values and the reference starts from the same rounded
numbers: every kernel is measured on its own, not behind its predecessor.  Bar per tensor: err(kernel) <= K * err(ref32) + 1e-7 with err(a) = max|a - ref64| /
max|ref64| (K: DESIGN.md par. 5.3); BatchNorm statistics folded by cerb_launch_bn_finalize are compared with the float64 statistics of the tensor the launch
stored, with K_BN.  db1 behind batch statistics is zero by construction (the sum of dhid over the rows vanishes): there the error of kernel and yardstick
is taken relative to the largest per-channel sum |dhid|, the size of the terms that cancel.  in_part is summed over its rows on the host in double.
Outputs sit between sentinel bands; assigned ones start as NaN, the accumulated dprev from random values; workspaces are NaN-poisoned."""
import ctypes as C

import pytest
import torch

import dev_kernels as D
import kernel_refs as R
from conftest import dev_switches
from test_conv_forward_parity_gpu import _controls, _finish_all
from test_kernel_parity_gpu import K_BN, Report, _acc_init, _gen

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
K_HEAD_FWD = 6    # worst ratio 2.53 (fwd2, 7 outputs: 96 products in one matrix-pipe accumulator chain behind a float32 BatchNorm)
K_HEAD_BWD1 = 12  # worst ratio 5.55, db2: a thread adds the signed dlogits of up to 256 rows in ONE float32 chain (then 8 row slots, then the slabs) where torch
                  # sums in blocks, and the sum cancels to ~ 1 / sqrt(rows) of its terms; dW2 stays below its yardstick, dgamma / dbeta (the same chain) below 3.3
K_HEAD_BWD2 = 4   # worst ratio 1.59
K_PW = 8        # worst ratio 3.04 (512 -> 256): pointwise_kernel is one thread's chain of cin sequential fmaf per output, torch sums in blocks
K_BN_APPLY = 4
OUTS = (2, 3, 7)


def _zeros(rep, case, t, what):
    z = float((t <= 0).double().mean())
    rep.check(0.2 <= z <= 0.8, case, "the ReLU must cut between 20 %% and 80 %% of %s (%.2f): change the seed" % (what, z))


def _weights(gen, out):
    return dict(w1=torch.randn(96, 64, generator=gen) / 8, b1=0.1 * torch.randn(96, generator=gen), gamma=0.5 + torch.rand(96, generator=gen),
                beta=0.1 * torch.randn(96, generator=gen), w2=torch.randn(out, 96, generator=gen) / 96 ** 0.5, b2=0.1 * torch.randn(out, generator=gen))


def _prev(gen, rows, with_in):
    """-> prev, in_bn.  Without the BatchNorm in front: features relu(randn).  With it: the raw output of a convolution and (mean, rstd) = the float32 roundings
    of its float64 batch statistics, gamma in [0.5, 1.5], beta 0.1 randn"""
    if not with_in:
        return torch.relu(torch.randn(rows, 64, generator=gen)), None
    prev = torch.randn(rows, 64, generator=gen) * (0.5 + torch.rand(64, generator=gen)) + 0.3 * torch.randn(64, generator=gen)
    m, rs, _ = R.bn_stats(prev.view(1, rows, 64), F64)
    return prev, (m[0].to(F32), rs[0].to(F32), 0.5 + torch.rand(64, generator=gen), 0.1 * torch.randn(64, generator=gen))


def _chain(wt, prev, dt, **kw):
    return R.head_train_forward(prev, wt["w1"], wt["b1"], wt["gamma"], wt["beta"], wt["w2"], wt["b2"], dt, **kw)


def _hid_and_stats(wt, prev, in_bn):
    """what the backward kernels are handed: hid = the float32 rounding of the float64 hidden map, (mean, rstd) = the roundings of ITS float64 statistics"""
    hid = _chain(wt, prev, F64, in_bn=in_bn)["hid"].detach().to(F32)
    m, rs, _ = R.bn_stats(hid.view(1, -1, 96), F64)
    return hid, (m[0].to(F32), rs[0].to(F32))


def _dev(*ts):
    return [None if t is None else t.cuda().contiguous() for t in ts]


def _in_ptrs(in_bn):
    d = _dev(*in_bn) if in_bn is not None else [None] * 4
    return d, [D.ptr(t) for t in d]


def _fold(L, part, blocks, rows, Cc):
    """cerb_launch_bn_finalize over [blocks][C][2] double partials -> mean, rstd, var_unbiased [1][C]"""
    out = [D.Guarded((1, Cc)) for _ in range(3)]
    ws = D.workspace(L.cerb_dev_bn_fold_workspace_bytes(1, Cc))
    D.ok(L.cerb_dev_bn_finalize(D.ptr(part), blocks, rows, Cc, 1e-5, D.ptr(out[0]), D.ptr(out[1]), D.ptr(out[2]), 1, D.ptr(ws), D.stream()), "bn_finalize")
    return out, ws


def _stats_bar(L, rep, case, part, blocks, stored, rows, Cc):
    """the statistics partials a producer left, folded, against the float64 statistics of the tensor it stored"""
    out, ws = _fold(L, part, blocks, rows, Cc)
    r64, r32 = R.bn_stats(stored.view(1, rows, Cc), F64), R.bn_stats(stored.view(1, rows, Cc), F32)
    for i, name in enumerate(("mean", "rstd", "var_unbiased")):
        rep.bar(case, "bn " + name, out[i].cpu(), r64[i], r32[i])
    rep.intact(case, ws, *out)


@dev_switches
def test_head_forward_passes_vs_float64():
    L, gen = D.lib(), _gen(41)
    rep, bnrep = Report("head_fwd", K_HEAD_FWD), Report("head_fwd1 bn_part", K_BN)
    # ---- fwd1: 131152 rows = 8197 sixteen-row tiles > 4 x 2048 workgroups: the tile loop of a wave runs twice
    for rows in (16, 48, 64, 2112, 131152):
        for with_in in (False, True):
            case = ("fwd1", rows, "in_bn" if with_in else "-")
            wt = _weights(gen, 3)
            prev, in_bn = _prev(gen, rows, with_in)
            t64, t32 = _chain(wt, prev, F64, in_bn=in_bn), _chain(wt, prev, F32, in_bn=in_bn)
            if with_in:
                _zeros(rep, case, t64["p"].detach(), "relu(bn_in(prev))")
            hid = D.Guarded((rows, 96))
            part = D.Guarded((2048 * 96 * 2 * 2,))
            nb = C.c_int(-1)
            pd, w1d, b1d = _dev(prev, wt["w1"], wt["b1"])
            keep, ip = _in_ptrs(in_bn)
            rc = L.cerb_dev_head_fwd1(D.ptr(pd), D.ptr(w1d), D.ptr(b1d), D.ptr(hid), rows, D.ptr(part), C.byref(nb), ip[0], ip[1], ip[2], ip[3], D.stream())
            D.ok(rc, case)
            rep.bar(case, "hid", hid.cpu(), t64["hid"].detach(), t32["hid"].detach())
            rep.check(nb.value == min((rows // 16 + 3) // 4, 2048), case, "bn_blocks %d" % nb.value)
            _stats_bar(L, bnrep, case, part, nb.value, hid.cpu(), rows, 96)
            rep.intact(case, hid, part)
            rep.check(bool(torch.isnan(part.t[nb.value * 96 * 4:]).all()), case, "bn_part rows past bn_blocks untouched")   # (two NaN floats per double)
    # ---- fwd2
    kept = None
    for rows in (16, 80, 2112):
        for out in OUTS:
            case = ("fwd2", rows, "out %d" % out)
            wt = _weights(gen, out)
            prev, _ = _prev(gen, rows, False)
            hid, stats = _hid_and_stats(wt, prev, None)
            t64, t32 = _chain(wt, prev, F64, hid=hid, stats=stats), _chain(wt, prev, F32, hid=hid, stats=stats)
            _zeros(rep, case, t64["z"].detach(), "relu(bn(hid))")
            lg = D.Guarded((rows, out))
            d = _dev(hid, stats[0], stats[1], wt["gamma"], wt["beta"], wt["w2"], wt["b2"])
            D.ok(L.cerb_dev_head_fwd2(*[D.ptr(t) for t in d], D.ptr(lg), rows, out, D.stream()), case)
            rep.bar(case, "logits", lg.cpu(), t64["logits"].detach(), t32["logits"].detach())
            rep.intact(case, lg)
            if rows == 2112 and out == 7:
                kept = (case, wt, hid, stats, lg.cpu(), t64["logits"].detach(), t32["logits"].detach())
    # refusals: 24 rows (no multiple of 16); cerb_head_train_supported per case
    for name in ("fwd1", "fwd2"):
        wt = _weights(gen, 3)
        prev, _ = _prev(gen, 32, False)
        hid, stats = _hid_and_stats(wt, prev, None)
        o = D.Guarded((24, 96 if name == "fwd1" else 3))
        if name == "fwd1":
            d = _dev(prev, wt["w1"], wt["b1"])
            rc = L.cerb_dev_head_fwd1(D.ptr(d[0]), D.ptr(d[1]), D.ptr(d[2]), D.ptr(o), 24, None, None, None, None, None, None, D.stream())
        else:
            d = _dev(hid, stats[0], stats[1], wt["gamma"], wt["beta"], wt["w2"], wt["b2"])
            rc = L.cerb_dev_head_fwd2(*[D.ptr(t) for t in d], D.ptr(o), 24, 3, D.stream())
        torch.cuda.synchronize()
        rep.check(rc != 0 and bool(torch.isnan(o.cpu()).all()) and o.intact(), (name, "24 rows"), "must be refused and write nothing")
    for rows, cin, chid, out, want in ((64, 64, 96, 2, 1), (64, 64, 96, 3, 1), (32960, 64, 96, 7, 1), (64, 64, 96, 4, 0), (80, 64, 96, 3, 0), (24, 64, 96, 3, 0), (64, 128, 96, 3, 0),
                                       (64, 64, 64, 3, 0), (0, 64, 96, 3, 0)):
        rep.check(L.cerb_dev_head_train_supported(rows, cin, chid, out) == want, ("supported", rows, cin, chid, out), "cerb_head_train_supported")
    # sensitivity: the ReLU mask taken from hid instead of bn(hid)
    case, wt, hid, stats, got, r64, r32 = kept
    h64 = hid.to(F64)
    bn = R.bn_const(h64, stats[0], stats[1], wt["gamma"], wt["beta"], F64)
    wrong = (bn * (h64 > 0)) @ wt["w2"].to(F64).t() + wt["b2"].to(F64)
    _controls(rep, case, got, r64, r32, [("the ReLU mask taken from hid instead of bn(hid)", wrong), ("no ReLU", bn @ wt["w2"].to(F64).t() + wt["b2"].to(F64))])
    _finish_all(rep, bnrep)


def _db1_bar(rep, case, got, g64, g32):
    """db1 behind batch statistics: the reference is zero up to rounding, so kernel and yardstick are measured against the size of the terms that cancel"""
    scale = float(g64["dhid"].abs().sum(0).max())
    eg = float((got.to(F64) - g64["db1"]).abs().max()) / scale if bool(torch.isfinite(got).all()) else float("inf")
    ey = float((g32["db1"].to(F64) - g64["db1"]).abs().max()) / scale
    print("%s %s db1 (relative to sum |dhid|): err %.3e yardstick %.3e ratio %.2f" % (rep.family, case, eg, ey, eg / ey if ey > 0 else float("inf")))
    if eg > 1e-7:
        rep.worst = max(rep.worst, eg / ey if ey > 0 else float("inf"))
    rep.check(eg <= rep.k * ey + 1e-7, case, "db1: err %.3e > %g * %.3e + 1e-7" % (eg, rep.k, ey))


def _wrong_backward(wt, prev, hid, stats, dlog, mask_from_hid):
    """the head's backward by hand in float64 with one mistake: the ReLU mask taken from hid (else the right mask), batch-statistics terms as they should be"""
    h, dl = hid.to(F64), dlog.to(F64)
    mean, rstd, gamma = stats[0].to(F64), stats[1].to(F64), wt["gamma"].to(F64)
    xhat = (h - mean) * rstd
    mask = (h > 0) if mask_from_hid else (xhat * gamma + wt["beta"].to(F64) > 0)
    dz = (dl @ wt["w2"].to(F64)) * mask
    dbeta, dgamma = dz.sum(0), (dz * xhat).sum(0)
    dhid = gamma * rstd * (dz - dbeta / h.shape[0] - xhat * dgamma / h.shape[0])
    return dict(dgamma=dgamma, dbeta=dbeta, dprev=dhid @ wt["w1"].to(F64), dw1=dhid.t() @ prev.to(F64))


@dev_switches
def test_head_backward_passes_vs_float64():
    L, gen = D.lib(), _gen(42)
    rep1, rep2 = Report("head_bwd1", K_HEAD_BWD1), Report("head_bwd2", K_HEAD_BWD2)
    kept1 = kept2 = None
    # ---- bwd1: 2112 rows = two slabs, the second of 64 rows; 32960 = 17 slabs, 256 rows per thread in a full one
    for rows in (64, 2112, 4160, 32960):
        for out in OUTS:
            case = ("bwd1", rows, "out %d" % out)
            wt = _weights(gen, out)
            prev, _ = _prev(gen, rows, False)
            hid, stats = _hid_and_stats(wt, prev, None)
            dlog = torch.randn(rows, out, generator=gen) / rows
            g = []
            for dt in (F64, F32):
                t = _chain(wt, prev, dt, hid=hid, stats=stats)
                g.append(R.head_train_backward(t, dlog, dt))
            _zeros(rep1, case, t["z"].detach(), "relu(bn(hid))")
            outs = dict(dw2=D.Guarded((out, 96)), db2=D.Guarded((out,)), dgamma=D.Guarded((96,)), dbeta=D.Guarded((96,)))
            ws = D.workspace(L.cerb_dev_head_bwd_workspace_bytes(rows, out))
            d = _dev(hid, dlog, stats[0], stats[1], wt["gamma"], wt["beta"], wt["w2"])
            D.ok(L.cerb_dev_head_bwd1(*[D.ptr(t) for t in d], D.ptr(outs["dw2"]), D.ptr(outs["db2"]), D.ptr(outs["dgamma"]), D.ptr(outs["dbeta"]), rows, out, D.ptr(ws), D.stream()), case)
            for k, o in outs.items():
                rep1.bar(case, k, o.cpu(), g[0][k], g[1][k])
            rep1.intact(case, ws, *outs.values())
            if rows == 2112 and out == 7:
                kept1 = (case, wt, prev, hid, stats, dlog, {k: o.cpu() for k, o in outs.items()}, g)
    # ---- bwd2: 32960 rows = 515 tiles for 512 workgroups (three workgroups take a second tile)
    for rows in (64, 192, 32960):
        for out in OUTS:
            for eval_mode, assign, with_in, with_part in ((0, 1, False, False), (1, 0, False, False), (0, 1, True, True), (0, 0, True, False), (1, 1, True, True)):
                case = ("bwd2", rows, "out %d" % out, "eval" if eval_mode else "train", "assign" if assign else "accumulate", ("in_bn + in_part" if with_part else "in_bn") if with_in else "-")
                wt = _weights(gen, out)
                prev, in_bn = _prev(gen, rows, with_in)
                hid, stats = _hid_and_stats(wt, prev, in_bn)
                dlog = torch.randn(rows, out, generator=gen) / rows
                g = []
                for dt in (F64, F32):
                    t = _chain(wt, prev, dt, in_bn=in_bn, hid=hid, stats=stats if eval_mode else None)
                    g.append(R.head_train_backward(t, dlog, dt, prev=prev, in_bn=in_bn))
                init = None if assign else _acc_init(g[0]["dprev"], gen)
                dprev = D.Guarded((rows, 64), init=init)
                dw1, db1 = D.Guarded((96, 64)), D.Guarded((96,))
                ws = D.workspace(L.cerb_dev_head_bwd_workspace_bytes(rows, out))
                nblk = min(rows // 64, 512)
                part = D.Guarded((nblk * 64 * 2 * 2,)) if with_part else None
                d = _dev(hid, dlog, prev, stats[0], stats[1], wt["gamma"], wt["beta"], g[0]["dgamma"].to(F32), g[0]["dbeta"].to(F32), wt["w1"], wt["w2"])
                keep, ip = _in_ptrs(in_bn)
                nb = C.c_int(-1)
                rc = L.cerb_dev_head_bwd2(*[D.ptr(t) for t in d], D.ptr(dprev), D.ptr(dw1), D.ptr(db1), rows, out, eval_mode, assign, D.ptr(ws), ip[0], ip[1], ip[2], ip[3], D.ptr(part),
                                          C.byref(nb), D.stream())
                D.ok(rc, case)
                add = 0 if assign else init
                rep2.bar(case, "dprev", dprev.cpu(), g[0]["dprev"] + (0 if assign else init.to(F64)), g[1]["dprev"] + add)
                rep2.bar(case, "dw1", dw1.cpu(), g[0]["dw1"], g[1]["dw1"])
                if eval_mode:
                    rep2.bar(case, "db1", db1.cpu(), g[0]["db1"], g[1]["db1"])
                else:
                    _db1_bar(rep2, case, db1.cpu(), g[0], g[1])
                if with_part:
                    rep2.check(nb.value == nblk, case, "in_part rows %d" % nb.value)
                    got = part.t.view(F64).view(nblk, 64, 2).sum(0)   # summed on the host in double
                    rep2.bar(case, "in_part sum dz", got[:, 0].cpu(), g[0]["in_part"][:, 0], g[1]["in_part"][:, 0])
                    rep2.bar(case, "in_part sum dz xhat", got[:, 1].cpu(), g[0]["in_part"][:, 1], g[1]["in_part"][:, 1])
                rep2.intact(case, ws, dprev, dw1, db1, part)
                if rows == 192 and out == 7 and not eval_mode and assign and not with_in:
                    kept2 = (case, wt, prev, hid, stats, dlog, dict(dprev=dprev.cpu(), dw1=dw1.cpu()), g)
    # ---- refusals: out 4; 80 rows for bwd2; in_part without assign
    wt = _weights(gen, 3)
    prev, in_bn = _prev(gen, 128, True)
    hid, stats = _hid_and_stats(wt, prev, in_bn)
    dlog = torch.randn(128, 4, generator=gen)
    w24 = torch.randn(4, 96, generator=gen)
    zero = torch.zeros(96)

    def bwd2(rows, out, assign, with_part, what):
        dprev, dw1, db1, part = D.Guarded((128, 64)), D.Guarded((96, 64)), D.Guarded((96,)), D.Guarded((2 * 64 * 2 * 2,))
        ws = D.workspace(L.cerb_dev_head_bwd_workspace_bytes(128, 7))
        d = _dev(hid, dlog, prev, stats[0], stats[1], wt["gamma"], wt["beta"], zero, zero, wt["w1"], w24)
        keep, ip = _in_ptrs(in_bn)
        rc = L.cerb_dev_head_bwd2(*[D.ptr(t) for t in d], D.ptr(dprev), D.ptr(dw1), D.ptr(db1), rows, out, 0, assign, D.ptr(ws), ip[0], ip[1], ip[2], ip[3], D.ptr(part) if with_part else None,
                                  None, D.stream())
        torch.cuda.synchronize()
        clean = all(bool(torch.isnan(o.cpu()).all()) and o.intact() for o in (dprev, dw1, db1, part))
        rep2.check(rc != 0 and clean, ("refusal", what), "must be refused and write nothing")

    bwd2(128, 4, 1, False, "out 4")
    bwd2(80, 3, 1, False, "80 rows")
    bwd2(128, 3, 0, True, "in_part without assign")
    outs = [D.Guarded((4, 96)), D.Guarded((4,)), D.Guarded((96,)), D.Guarded((96,))]
    ws = D.workspace(L.cerb_dev_head_bwd_workspace_bytes(128, 7))
    d = _dev(hid, dlog, stats[0], stats[1], wt["gamma"], wt["beta"], w24)
    rc = L.cerb_dev_head_bwd1(*[D.ptr(t) for t in d], *[D.ptr(o) for o in outs], 128, 4, D.ptr(ws), D.stream())
    torch.cuda.synchronize()
    rep1.check(rc != 0 and all(bool(torch.isnan(o.cpu()).all()) and o.intact() for o in outs), ("refusal", "out 4"), "must be refused and write nothing")
    # ---- sensitivity
    case, wt, prev, hid, stats, dlog, got, g = kept1
    wrong = _wrong_backward(wt, prev, hid, stats, dlog, True)
    for k in ("dgamma", "dbeta"):
        _controls(rep1, case + (k,), got[k], g[0][k], g[1][k], [("the ReLU mask taken from hid instead of bn(hid)", wrong[k])])
    case, wt, prev, hid, stats, dlog, got, g = kept2
    wrong = _wrong_backward(wt, prev, hid, stats, dlog, True)
    t = _chain(wt, prev, F64, hid=hid, stats=stats)   # statistics as constants: no batch-statistics terms
    no_batch = R.head_train_backward(t, dlog, F64)
    for k in ("dprev", "dw1"):
        _controls(rep2, case + (k,), got[k], g[0][k], g[1][k], [("the batch-statistics terms of dhid dropped", no_batch[k]), ("the ReLU mask taken from hid instead of bn(hid)", wrong[k])])
    _finish_all(rep1, rep2)


@dev_switches
def test_pointwise_and_bn_apply_vs_float64():
    L, gen = D.lib(), _gen(43)
    rep, bnrep, app = Report("pointwise", K_PW), Report("pointwise bn_part", K_BN), Report("bn_apply", K_BN_APPLY)
    kept = None
    for rows in (64, 511, 4097):
        for cin, cout in ((64, 96), (96, 7), (512, 256)):
            for scaled in (False, True):
                case = (rows, "%d->%d" % (cin, cout), "in_scale" if scaled else "-")
                x = torch.relu(torch.randn(rows, cin, generator=gen))
                w, b = torch.randn(cout, cin, generator=gen) / cin ** 0.5, 0.1 * torch.randn(cout, generator=gen)
                sc = (torch.rand(rows, cin, generator=gen) > 0.3).to(F32) / 0.7 if scaled else None   # a dropout mask x 1 / (1 - p), per (row, channel)
                r64, r32 = R.pointwise_forward(x, w, b, sc, F64), R.pointwise_forward(x, w, b, sc, F32)
                out = D.Guarded((rows, cout))
                part = D.Guarded((2048 * cout * 2 * 2,))
                nb = C.c_int(-1)
                d = _dev(x, w, b)
                scd = None if sc is None else sc.cuda()
                D.ok(L.cerb_dev_pointwise(D.ptr(d[0]), D.ptr(d[1]), D.ptr(d[2]), D.ptr(out), rows, cin, cout, D.ptr(scd), D.ptr(part), C.byref(nb), D.stream()), case)
                rep.bar(case, "out", out.cpu(), r64, r32)
                print("pointwise %s: bn_blocks %d" % (case, nb.value))
                rep.check(nb.value >= 0, case, "bn_blocks reported")
                if nb.value > 0:
                    _stats_bar(L, bnrep, case, part, nb.value, out.cpu(), rows, cout)
                rep.check(bool(torch.isnan(part.t[max(nb.value, 0) * cout * 4:]).all()), case, "bn_part rows past bn_blocks untouched")   # (two NaN floats per double)
                rep.intact(case, out, part)
                if rows == 511 and cin == 64 and scaled:
                    kept = (case, out.cpu(), r64, r32, R.pointwise_forward(x, w, b, None, F64))
    rep.check(kept is not None, "control", "case kept")
    _controls(rep, kept[0], kept[1], kept[2], kept[3], [("in_scale dropped", kept[4])])
    keptb = None
    for G, rows, Cc in ((1, 33, 64), (5, 130, 96), (1, 70, 512), (5, 33, 512)):
        for in_place, with_res, relu in ((True, False, 1), (False, True, 1), (False, False, 0), (True, True, 0)):
            case = (G, rows, Cc, "in place" if in_place else "from src", "resid" if with_res else "-", "relu %d" % relu)
            src = torch.randn(G, rows, Cc, generator=gen) * (0.5 + torch.rand(G, 1, Cc, generator=gen)) + 0.3 * torch.randn(G, 1, Cc, generator=gen)
            res = torch.randn(G, rows, Cc, generator=gen) if with_res else None
            m, rs, _ = R.bn_stats(src, F64)
            m, rs = m.to(F32), rs.to(F32)
            ga, be = 0.5 + torch.rand(G, Cc, generator=gen), 0.1 * torch.randn(G, Cc, generator=gen)
            r64, r32 = R.bn_apply(src, res, m, rs, ga, be, relu, F64), R.bn_apply(src, res, m, rs, ga, be, relu, F32)
            if relu:
                _zeros(app, case, r64, "the reference")
            x = D.Guarded((G, rows, Cc), init=src if in_place else None)
            d = _dev(src, res, m, rs, ga, be)
            D.ok(L.cerb_dev_bn_apply(D.ptr(x), None if in_place else D.ptr(d[0]), D.ptr(d[1]), rows * Cc, rows, Cc, G, D.ptr(d[2]), D.ptr(d[3]), D.ptr(d[4]), D.ptr(d[5]), relu, D.stream()), case)
            app.bar(case, "out", x.cpu(), r64, r32)
            app.intact(case, x)
            if with_res and relu:
                keptb = (case, x.cpu(), r64, r32, R.bn_apply(src, None, m, rs, ga, be, relu, F64))
    _controls(app, keptb[0], keptb[1], keptb[2], keptb[3], [("the residual left out", keptb[4])])
    _finish_all(rep, bnrep, app)
