"""Kernel-level parity of what lies between the convolutions and the user: the 7x7 stem, the output heads (cerb_launch_head, cerb_launch_head_group with both
second GEMMs and every body), Patch-Class, the forward decoder entry, the inference max-pool and the tile-planar exit -- each launcher on its own through the
cerb_devfwd_* entries of the developers' library (tests/dev_kernels.py) against a float64 reference of the same operation (tests/kernel_refs.py; tied to the
torch.nn module chains by tests/test_kernel_refs.py).  The entries pack raw weights with the functions cerb_net_finalize packs with (cerb_host_pack_stem /
_head / _patch_class), so a wrong permutation shared by every kernel body -- invisible to the bit-identity A/Bs -- shows here.

Float outputs: per tensor err(a) = max|a - ref64| / max|ref64| and err(kernel) <= K * err(ref32) + 1e-7, K per family at least twice the worst ratio measured
on the MI355X and never below 4 (table: DESIGN.md par. 5.3).  Class ids (TYPE heads, Patch-Class): equal to the float64 argmax wherever the float64 top-2
logit margin exceeds 2 (K err32 + 1e-7) max|logit|, one of the float64 top two elsewhere, and at most 0.1 % of a case's pixels may lie under that margin.
The protections of tests/test_kernel_parity_gpu.py apply: outputs between sentinel bands, assigned outputs start as NaN, canvases start as a sentinel that
must survive outside the windows, tile-planar outputs start as zero with NaN at the pixels.  Every function ends with refusals and sensitivity controls."""
import ctypes as C
import struct

import pytest
import torch
import torch.nn.functional as F

import dev_kernels as D
import kernel_refs as R
from conftest import dev_switches
from test_conv_forward_parity_gpu import _controls, _finish_all, _roi_bar
from test_kernel_parity_gpu import Report, _gen

pytestmark = pytest.mark.gpu
F64, F32 = torch.float64, torch.float32
K_STEM = 4
K_HEAD = 4
K_PATCH_CLASS = 8   # worst ratio 3.75: each hidden unit is ONE thread's chain of 512 sequential fmaf (then 256), torch sums in blocks; the errors stay below 6e-7
K_ENTRY = 4
HEAD_LAUNCHERS = {0: "head_kernel", 1: "head_group 16x16x4", 2: "head_group 4x4x1"}
INST, TYPE = 0, 1


def _zeros(rep, case, t, what="the reference"):
    z = float((t <= 0).double().mean())
    rep.check(0.2 <= z <= 0.8, case, "the ReLU must cut between 20 %% and 80 %% of %s (%.2f): change the seed" % (what, z))


# =====================================================================================================================================================
# stem
# =====================================================================================================================================================
def _stem_run(L, tiles, w, scale, shift, relu, host_pack):
    N, H, W, _ = tiles.shape
    out = D.Guarded((N, H, W, 64))
    td, wd = tiles.cuda().contiguous(), w.cuda().contiguous()
    u8 = tiles.dtype == torch.uint8
    rc = L.cerb_devfwd_stem(D.ptr(td) if u8 else None, None if u8 else D.ptr(td), D.ptr(wd), D.hptr(scale), D.hptr(shift), host_pack, D.ptr(out), N, H, W, relu, D.stream())
    torch.cuda.synchronize()
    return rc, out


def _stem_weights(gen, folded):
    w = torch.randn(64, 3, 7, 7, generator=gen) / 147 ** 0.5
    scale = 0.5 + torch.rand(64, generator=gen) if folded else torch.ones(64)
    return w, scale, 0.1 * torch.randn(64, generator=gen)


@dev_switches
def test_stem_vs_float64_conv2d():
    L, rep, gen = D.lib(), Report("stem", K_STEM), _gen(31)
    u8 = lambda n, h, w: torch.randint(0, 256, (n, h, w, 3), generator=gen, dtype=torch.uint8)
    cases = [  # (tiles, relu, folded BatchNorm + host packer)
        (u8(1, 8, 32), 1, True),      # one whole 8 x 32 tile
        (u8(2, 5, 7), 1, True),       # smaller than a tile
        (u8(3, 13, 45), 1, True),     # partial tiles on both axes, three images
        (u8(3, 13, 45), 0, False),    # the training handle's form: raw convolution, device packer
        (u8(1, 16, 64), 0, True),
        (u8(385, 9, 33), 1, True),    # 385 x 2 x 2 = 1540 tiles > the grid of 1536: the grid-stride loop runs
        (300 * torch.rand(3, 13, 45, 3, generator=gen) - 20, 1, True),   # float pixel values, negative and non-integer
        (300 * torch.rand(3, 13, 45, 3, generator=gen) - 20, 0, False),
    ]
    keep = None
    for tiles, relu, folded in cases:
        case = (tuple(tiles.shape[:3]), str(tiles.dtype).split(".")[1], "relu %d" % relu, "host pack" if folded else "device pack")
        w, scale, shift = _stem_weights(gen, folded)
        ref64, ref32 = R.stem_forward(tiles, w, scale, shift, relu, F64), R.stem_forward(tiles, w, scale, shift, relu, F32)
        if relu:
            _zeros(rep, case, ref64)
        rc, out = _stem_run(L, tiles, w, scale, shift, relu, 1 if folded else 0)
        rep.check(rc == 0, case, "hipError %d" % rc)
        rep.bar(case, "out", out.cpu(), ref64, ref32)
        print("stem %s: %.1f %% of the elements differ from the float32 conv2d" % (case, 100 * float((out.cpu() != ref32).double().mean())))
        rep.intact(case, out)
        if tiles.dtype == torch.uint8 and tuple(tiles.shape[:3]) == (3, 13, 45) and relu:
            keep = (case, tiles, w, scale, shift, out.cpu(), ref64, ref32)
    # one case on both packers (scale 1): both meet the bar, and the two streams are the same numbers in the same places
    tiles = u8(3, 13, 45)
    w, scale, shift = _stem_weights(gen, False)
    ref64, ref32 = R.stem_forward(tiles, w, scale, shift, 1, F64), R.stem_forward(tiles, w, scale, shift, 1, F32)
    outs = []
    for host_pack in (0, 1):
        rc, out = _stem_run(L, tiles, w, scale, shift, 1, host_pack)
        rep.check(rc == 0, ("packers", host_pack), "hipError %d" % rc)
        rep.bar(("packers", "host" if host_pack else "device"), "out", out.cpu(), ref64, ref32)
        rep.intact(("packers", host_pack), out)
        outs.append(out.cpu())
    rep.equal("packers", "device-packed == host-packed", outs[0], outs[1])
    # refusals: the device packer folds no scale; both inputs at once
    rc, out = _stem_run(L, tiles, w, 0.5 + torch.rand(64, generator=gen), shift, 1, 0)
    rep.check(rc != 0 and bool(torch.isnan(out.cpu()).all()) and out.intact(), "refusal", "device packer with a scale")
    # sensitivity
    case, tiles, w, scale, shift, got, ref64, ref32 = keep
    x = (tiles.permute(0, 3, 1, 2).to(F64) / 255).contiguous()
    wf = w.to(F64) * scale.to(F64).view(64, 1, 1, 1)
    rpad = torch.relu(F.conv2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), wf, shift.to(F64))).permute(0, 2, 3, 1)
    _controls(rep, case, got, ref64, ref32, [("kx / ky swapped", R.stem_forward(tiles, w.transpose(-1, -2), scale, shift, 1, F64)),
                                             ("BGR channel order", R.stem_forward(tiles, w.flip(1), scale, shift, 1, F64)), ("replicate padding", rpad)])
    rep.finish()


# =====================================================================================================================================================
# output heads
# =====================================================================================================================================================
class Canvas(object):
    """A destination canvas of npix pixels x per elements, filled with `fill` and padded with it on both sides: whatever no window pixel maps to must still
    hold the fill after the launch."""
    PADE = 4096

    def __init__(self, npix, per, dtype, fill):
        self.per, self.fill = per, fill
        self.buf = torch.full((2 * self.PADE + npix * per,), fill, dtype=dtype, device="cuda")
        self.body = self.buf[self.PADE:self.PADE + npix * per]

    def ptr(self):
        return C.c_void_p(self.body.data_ptr())

    def window(self, offs, oh, ow, row_stride):
        """-> the window pixels [N][oh][ow][per] on the host, and whether everything else still holds the fill"""
        pix = offs.view(-1, 1, 1) + torch.arange(oh).view(1, oh, 1) * row_stride + torch.arange(ow).view(1, 1, ow)
        el = (pix.unsqueeze(-1) * self.per + torch.arange(self.per)).cuda()
        other = torch.ones(self.buf.numel(), dtype=torch.bool, device="cuda")
        other[self.PADE + el.reshape(-1)] = False
        return self.body[el].cpu(), bool((self.buf[other] == self.fill).all())


def _head_weights(gen, out_ch):
    return dict(w1=torch.randn(96, 64, generator=gen) / 8, b1=0.1 * torch.randn(96, generator=gen), scale=0.5 + torch.rand(96, generator=gen),
                shift=0.1 * torch.randn(96, generator=gen), w2=torch.randn(out_ch, 96, generator=gen) / 96 ** 0.5, b2=0.1 * torch.randn(out_ch, generator=gen))


def _head_ref(feat, wt, dt):
    return R.head_forward(feat, wt["w1"], wt["b1"], wt["scale"], wt["shift"], wt["w2"], wt["b2"], dt)


def _spec(wt, kind, out_ch, win=None, roi=0, logits=False, addr="off"):
    return dict(w=wt, kind=kind, out_ch=out_ch, win=win, roi=roi, logits=logits, addr=addr)


class HeadRun(object):
    """One call of cerb_devfwd_head over `specs`.  Per head afterwards: logits [N][H][W][out] or None, inst [N][oh][ow][out - 1] or the class ids of both TYPE
    outputs, the absmax word, and `clean`: the sentinel around and between the windows survived."""

    def __init__(self, L, launcher, feat, specs, planar=False):
        N, H, W, _ = feat.shape
        fd = D._to_planar(feat.cuda()) if planar else feat.cuda().contiguous()
        arr = (D.DevHead * len(specs))()
        self.keep, parts = [fd], []
        for i, s in enumerate(specs):
            y0, x0, oh, ow = s["win"] if s["win"] is not None else (0, 0, H, W)
            row_stride = ow if (s["addr"] == "off" and s["win"] is None) else ow + 5
            if s["addr"] == "off":   # the tiles in reverse order, 3 pixels apart, 2 pixels in
                offs = torch.tensor([2 + (N - 1 - n) * (oh * row_stride + 3) for n in range(N)], dtype=torch.long)
                off_dev, tile_stride = offs.cuda(), 0
            else:
                tile_stride = oh * row_stride + 7
                offs, off_dev = torch.arange(N, dtype=torch.long) * tile_stride, None
            npix = N * (oh * row_stride + 8) + 8
            h = arr[i]
            for k in ("w1", "b1", "scale", "shift", "w2", "b2"):
                setattr(h, k, D.hptr(s["w"][k]).value)
            h.out_ch, h.kind, h.crop_y0, h.crop_x0, h.out_h, h.out_w, h.roi = s["out_ch"], s["kind"], y0, x0, oh, ow, s["roi"]
            lg = D.Guarded((N, H, W, s["out_ch"])) if s["logits"] else None
            inst = u8 = i64 = None
            if s["kind"] == INST:
                inst = Canvas(npix, s["out_ch"] - 1, torch.float32, 777.0)
                h.out_inst = inst.ptr().value
            else:
                u8, i64 = Canvas(npix, 1, torch.uint8, 0xEE), Canvas(npix, 1, torch.int64, -99)
                h.out_type_u8, h.out_type_i64 = u8.ptr().value, i64.ptr().value
            word = torch.zeros(1, dtype=torch.int32, device="cuda")
            h.logits = D.ptr(lg).value if lg is not None else None
            h.tile_off = off_dev.data_ptr() if off_dev is not None else None
            h.tile_stride, h.row_stride, h.absmax_bits = tile_stride, row_stride, word.data_ptr()
            parts.append((lg, inst, u8, i64, word, offs, oh, ow, row_stride))
            self.keep += [off_dev, word]
        self.rc = L.cerb_devfwd_head(launcher, D.ptr(fd), 1 if planar else 0, N, H, W, C.cast(arr, C.c_void_p), len(specs), D.stream())
        torch.cuda.synchronize()
        self.heads = []
        for lg, inst, u8, i64, word, offs, oh, ow, row_stride in parts:
            r = dict(logits=None if lg is None else lg.cpu(), clean=lg is None or lg.intact(), absmax=struct.unpack("f", struct.pack("i", int(word.item())))[0])
            for name, cv in (("inst", inst), ("u8", u8), ("i64", i64)):
                if cv is not None:
                    r[name], ok = cv.window(offs, oh, ow, row_stride)
                    r["clean"] = r["clean"] and ok
                    r["untouched"] = r.get("untouched", True) and bool((cv.buf == cv.fill).all())
            self.heads.append(r)


def _argmax_rule(rep, case, name, got, ref, err32, pixels_cap=0.001):
    """got: class ids; ref: dict(top2 [..., 2], margin, logits) of the float64 reference over the same pixels"""
    got = got.reshape(-1).to(torch.long)
    top2, margin = ref["top2"].reshape(-1, 2), ref["margin"].reshape(-1)
    thr = 2 * (rep.k * err32 + 1e-7) * float(ref["logits"].abs().max())
    clear = margin > thr
    close = int((~clear).sum())
    print("%s %s %s: %d of %d pixels under the margin %.3e; %d differ from the float64 argmax" % (rep.family, case, name, close, got.numel(), thr, int((got != top2[:, 0]).sum())))
    rep.check(close <= pixels_cap * got.numel(), case, name + ": more than 0.1 % of the pixels under the margin: choose another seed")
    rep.check(bool((got[clear] == top2[clear, 0]).all()), case, name + ": the float64 argmax wherever the margin is clear")
    rep.check(bool(((got == top2[:, 0]) | (got == top2[:, 1]))[~clear].all()), case, name + ": one of the float64 top two under the margin")


def _win(t, s, H, W):
    y0, x0, oh, ow = s["win"] if s["win"] is not None else (0, 0, H, W)
    return t[:, y0:y0 + oh, x0:x0 + ow]


def _check_head(rep, case, r, s, ref64, ref32, absmax_from):
    """one head of a run against its references; absmax_from: the logits the same launcher stored for these weights (None: this run's own)"""
    H, W = ref64["logits"].shape[1:3]
    err32 = R.err(ref32["logits"], ref64["logits"])
    if s["logits"]:
        rep.bar(case, "logits", r["logits"], ref64["logits"], ref32["logits"])
    if s["kind"] == INST:
        rep.bar(case, "inst", r["inst"], _win(ref64["inst"], s, H, W), _win(ref32["inst"], s, H, W))
    else:
        sub = dict(top2=_win(ref64["top2"], s, H, W), margin=_win(ref64["margin"], s, H, W), logits=ref64["logits"])
        _argmax_rule(rep, case, "type_u8", r["u8"], sub, err32)
        rep.check(torch.equal(r["u8"].to(torch.long), r["i64"]), case, "out_type_u8 == out_type_i64")
    lg = r["logits"] if absmax_from is None else absmax_from
    if lg is not None and bool(torch.isfinite(lg).all()):
        want = float((lg if s["logits"] else _win(lg, s, H, W)).abs().max())
        rep.check(r["absmax"] == want, case, "absmax word %r != the largest |logit| %r over the counted pixels" % (r["absmax"], want))
    rep.check(r["clean"], case, "sentinel around the windows / the logits")


HEAD_SHAPES = [(INST, 2), (INST, 3), (TYPE, 3), (TYPE, 7), (TYPE, 2), (TYPE, 5), (TYPE, 8)]   # the first four: specialised bodies under launcher 2
WINDOW = (2, 13, 4, 33)   # rows [2, 6) x columns [13, 46) of 7 x 112: the 16-aligned cover [0, 48) is wider than the 33 kept columns


@dev_switches
def test_output_heads_vs_float64():
    L, rep, gen = D.lib(), Report("heads", K_HEAD), _gen(32)
    weights = {sh: _head_weights(gen, sh[1]) for sh in HEAD_SHAPES}
    stored = {}   # (geometry, launcher, shape) -> the logits that launcher stored
    feats, refs = {}, {}
    # 3 x 5 x 48: 45 sixteen-pixel blocks (odd: the last task has one).  3 x 7 x 112: 147 blocks = 5 workgroups of head_kernel (the last partial), 3 of the
    # grouped kernel, whose last has waves with 8, 2, 0, 0 tasks
    for geo in ((3, 5, 48), (3, 7, 112)):
        feat = torch.relu(torch.randn(*geo, 64, generator=gen))
        feats[geo] = feat
        for sh in HEAD_SHAPES:
            refs[geo, sh] = (_head_ref(feat, weights[sh], F64), _head_ref(feat, weights[sh], F32))
            hid = torch.relu((feat.to(F64) @ weights[sh]["w1"].to(F64).t() + weights[sh]["b1"].to(F64)) * weights[sh]["scale"].to(F64) + weights[sh]["shift"].to(F64))
            _zeros(rep, (geo, sh), hid, "the hidden layer")
        for launcher in (0, 1, 2):
            for sh in HEAD_SHAPES:
                wt, (r64, r32) = weights[sh], refs[geo, sh]
                base = (HEAD_LAUNCHERS[launcher], geo, "kind %d out %d" % sh)
                a = HeadRun(L, launcher, feat, [_spec(wt, sh[0], sh[1], logits=True, addr="off")])
                rep.check(a.rc == 0, base, "hipError %d" % a.rc)
                _check_head(rep, base + ("logits",), a.heads[0], _spec(wt, sh[0], sh[1], logits=True), r64, r32, None)
                stored[geo, launcher, sh] = a.heads[0]["logits"]
                variants = [("whole map, tile_stride", _spec(wt, sh[0], sh[1], addr="stride"))]
                if geo == (3, 7, 112):
                    variants += [("window roi 0", _spec(wt, sh[0], sh[1], win=WINDOW, roi=0, addr="stride")), ("window roi 1", _spec(wt, sh[0], sh[1], win=WINDOW, roi=1, addr="off"))]
                runs = {}
                for name, s in variants:
                    b = HeadRun(L, launcher, feat, [s])
                    rep.check(b.rc == 0, base + (name,), "hipError %d" % b.rc)
                    _check_head(rep, base + (name,), b.heads[0], s, r64, r32, stored[geo, launcher, sh])
                    runs[name] = b.heads[0]
                if "window roi 0" in runs:
                    for k in ("inst", "u8", "i64"):
                        if k in runs["window roi 0"]:
                            rep.check(torch.equal(runs["window roi 0"][k], runs["window roi 1"][k]), base, "roi 1 == roi 0 inside the window (%s)" % k)
                    rep.check(runs["window roi 0"]["absmax"] == runs["window roi 1"]["absmax"], base, "roi 1 and roi 0 count the same pixels")
    # grouped launches of 5 (mixed shapes, windows and addressing) and 8 heads
    geo = (3, 7, 112)
    feat = feats[geo]
    five = [_spec(weights[INST, 2], INST, 2, win=WINDOW, roi=1), _spec(weights[INST, 3], INST, 3, addr="stride"), _spec(weights[TYPE, 3], TYPE, 3, win=WINDOW, roi=0, addr="stride"),
            _spec(weights[TYPE, 7], TYPE, 7), _spec(weights[TYPE, 5], TYPE, 5, win=WINDOW, roi=1, addr="stride")]
    eight = five + [_spec(weights[TYPE, 2], TYPE, 2), _spec(weights[TYPE, 8], TYPE, 8, logits=True), _spec(weights[INST, 3], INST, 3, win=(0, 0, 7, 16), roi=1)]
    for launcher in (1, 2):
        for specs in (five, eight):
            g = HeadRun(L, launcher, feat, specs)
            base = (HEAD_LAUNCHERS[launcher], "%d heads" % len(specs))
            rep.check(g.rc == 0, base, "hipError %d" % g.rc)
            for i, s in enumerate(specs):
                sh = (s["kind"], s["out_ch"])
                _check_head(rep, base + (i, "kind %d out %d" % sh), g.heads[i], s, refs[geo, sh][0], refs[geo, sh][1], stored[geo, launcher, sh])
    # tile-planar features, 2 x 20 x 48 (the 16 x 16 blocks hang over the map): the planar and the NHWC run of one launcher are identical
    featp = torch.relu(torch.randn(2, 20, 48, 64, generator=gen))
    pspecs = [_spec(weights[INST, 3], INST, 3, logits=True), _spec(weights[TYPE, 7], TYPE, 7, win=(3, 5, 15, 40), roi=1, addr="stride"), _spec(weights[TYPE, 5], TYPE, 5, logits=True),
              _spec(weights[INST, 2], INST, 2, addr="stride")]
    for launcher in (1, 2):
        a, b = HeadRun(L, launcher, featp, pspecs), HeadRun(L, launcher, featp, pspecs, planar=True)
        base = (HEAD_LAUNCHERS[launcher], "2x20x48")
        rep.check(a.rc == 0 and b.rc == 0, base, "hipError %d / %d" % (a.rc, b.rc))
        for i, s in enumerate(pspecs):
            r64, r32 = _head_ref(featp, s["w"], F64), _head_ref(featp, s["w"], F32)
            _check_head(rep, base + (i, "NHWC"), a.heads[i], s, r64, r32, None)
            for k in ("logits", "inst", "u8", "i64", "absmax"):
                if a.heads[i].get(k) is not None:
                    same = torch.equal(a.heads[i][k], b.heads[i][k]) if torch.is_tensor(a.heads[i][k]) else a.heads[i][k] == b.heads[i][k]
                    rep.check(same, base + (i,), "tile-planar == NHWC (%s)" % k)
            rep.check(b.heads[i]["clean"], base + (i, "planar"), "sentinel")
    # refusals: nothing is launched, every output keeps what it held
    wt = weights[INST, 3]
    refusals = [("W = 40", torch.relu(torch.randn(1, 4, 40, 64, generator=gen)), [_spec(wt, INST, 3)]), ("9 heads", feat, [_spec(wt, INST, 3)] * 9),
                ("out_ch 9", feat, [_spec(_head_weights(gen, 9), TYPE, 9)]), ("INST with 4 channels", feat, [_spec(_head_weights(gen, 4), INST, 4)]),
                ("a window past the map", feat, [_spec(wt, INST, 3, win=(2, 100, 4, 16))])]
    for what, f, specs in refusals:
        for launcher in ((1, 2) if what == "9 heads" else (0, 1, 2)):
            if what == "9 heads":   # the entry's array holds 8: hand it 8 heads and the count 9 would read past it; the count alone must refuse
                arr = (D.DevHead * 9)()
                rc = L.cerb_devfwd_head(launcher, D.ptr(f.cuda()), 0, f.shape[0], f.shape[1], f.shape[2], C.cast(arr, C.c_void_p), 9, D.stream())
                rep.check(rc != 0, (what, launcher), "must be refused")
                continue
            g = HeadRun(L, launcher, f, specs)
            rep.check(g.rc != 0, (what, launcher), "must be refused")
            rep.check(g.heads[0]["clean"] and g.heads[0]["absmax"] == 0.0 and g.heads[0]["untouched"], (what, launcher), "a refused launch writes nothing")
            print("heads refusal, %s launcher %d: hipError %d" % (what, launcher, g.rc))
    # sensitivity: references made wrong on purpose against outputs that passed
    geo, launcher = (3, 7, 112), 2
    for sh in ((TYPE, 7), (INST, 3)):
        wt, (r64, r32) = weights[sh], refs[geo, sh]
        case = ("control", HEAD_LAUNCHERS[launcher], "kind %d out %d" % sh)
        f64 = feats[geo].to(F64)
        pre = (f64 @ wt["w1"].to(F64).t() + wt["b1"].to(F64)) * wt["scale"].to(F64) + wt["shift"].to(F64)
        no_relu = pre @ wt["w2"].to(F64).t() + wt["b2"].to(F64)
        sw = dict(wt, w2=wt["w2"][[1, 0] + list(range(2, sh[1]))].contiguous())
        _controls(rep, case, stored[geo, launcher, sh], r64["logits"], r32["logits"], [("no ReLU between the layers", no_relu), ("two rows of W2 swapped", _head_ref(feats[geo], sw, F64)["logits"])])
        if sh[0] == INST:
            got = HeadRun(L, launcher, feats[geo], [_spec(wt, INST, 3)]).heads[0]["inst"]
            wrong = torch.stack([r64["prob"][..., 0], r64["prob"][..., 2]], -1)
            _controls(rep, case, got, r64["inst"], r32["inst"], [("softmax channel 0 in place of 1", wrong), ("two rows of W2 swapped", _head_ref(feats[geo], sw, F64)["inst"])])
    rep.finish()


# =====================================================================================================================================================
# Patch-Class
# =====================================================================================================================================================
PC_MAPS = [(9, 9), (14, 14), (8, 8), (6, 6), (3, 8), (9, 14), (1, 1)]


def _pc_weights(gen, out_ch):
    """bn1 is the fold of a BatchNorm whose running mean is that of the pooled features (E relu(randn) = 0.4): scale in [0.5, 1.5], shift 0.1 randn - 0.4 scale,
    so that the first ReLU cuts; bn2 follows a zero-mean layer"""
    s1 = 0.5 + torch.rand(512, generator=gen)
    return dict(s1=s1, h1=0.1 * torch.randn(512, generator=gen) - 0.4 * s1, w1=torch.randn(256, 512, generator=gen) / 512 ** 0.5, b1=0.1 * torch.randn(256, generator=gen),
                s2=0.5 + torch.rand(256, generator=gen), h2=0.1 * torch.randn(256, generator=gen), w2=torch.randn(out_ch, 256, generator=gen) / 16, b2=0.1 * torch.randn(out_ch, generator=gen))


def _pc_ref(x4, wt, dt, **kw):
    return R.patch_class_forward(x4, wt["s1"], wt["h1"], wt["w1"], wt["b1"], wt["s2"], wt["h2"], wt["w2"], wt["b2"], dt, **kw)


def _pc_run(L, x4, wt, out_ch, with_logits, addr, oh, ow):
    N, Hf, Wf, _ = x4.shape
    xd = x4.cuda().contiguous()
    lg = D.Guarded((N, out_ch)) if with_logits else None
    row_stride = ow + 3
    if addr == "off":
        offs = torch.tensor([1 + (N - 1 - n) * (oh * row_stride + 2) for n in range(N)], dtype=torch.long)
        off_dev, tile_stride = offs.cuda(), 0
    else:
        tile_stride = oh * row_stride + 5
        offs, off_dev = torch.arange(N, dtype=torch.long) * tile_stride, None
    cv = Canvas(N * (oh * row_stride + 6) + 4, 1, torch.float32, 777.0)
    rc = L.cerb_devfwd_patch_class(D.ptr(xd), D.hptr(wt["s1"]), D.hptr(wt["h1"]), D.hptr(wt["w1"]), D.hptr(wt["b1"]), D.hptr(wt["s2"]), D.hptr(wt["h2"]), D.hptr(wt["w2"]),
                                   D.hptr(wt["b2"]), N, Hf, Wf, out_ch, oh, ow, D.ptr(lg), cv.ptr(), D.ptr(off_dev), tile_stride, row_stride, D.stream())
    torch.cuda.synchronize()
    got, clean = cv.window(offs, oh, ow, row_stride)
    return rc, lg, got.view(N, oh * ow), clean and (lg is None or lg.intact())


@dev_switches
def test_patch_class_vs_float64():
    L, rep, gen = D.lib(), Report("patch_class", K_PATCH_CLASS), _gen(33)
    N, kept = 5, {}
    for out_ch in (9, 2, 16):
        wt = _pc_weights(gen, out_ch)
        for Hf, Wf in PC_MAPS:
            case = ("%dx%d" % (Hf, Wf), "out %d" % out_ch)
            x4 = torch.relu(torch.randn(N, Hf, Wf, 512, generator=gen))
            r64, r32 = _pc_ref(x4, wt, F64), _pc_ref(x4, wt, F32)
            _zeros(rep, case, r64["v"], "relu1")
            _zeros(rep, case, r64["h"], "relu2")
            err32 = R.err(r32["logits"], r64["logits"])
            for with_logits, addr, oh, ow in ((True, "off", 5, 7), (False, "stride", 1, 1)):
                rc, lg, cls, clean = _pc_run(L, x4, wt, out_ch, with_logits, addr, oh, ow)
                rep.check(rc == 0, case, "hipError %d" % rc)
                if with_logits:
                    rep.bar(case, "logits", lg.cpu(), r64["logits"], r32["logits"])
                    kept[(Hf, Wf), out_ch] = (x4, wt, lg.cpu(), r64, r32)
                rep.check(bool((cls == cls[:, :1]).all()) and bool((cls == cls.round()).all()), case, "one class id broadcast over the window")
                _argmax_rule(rep, case, "class id (%s)" % addr, cls[:, 0], r64, err32)
                rep.check(clean, case, "sentinel around every window / the logits")
    wt = _pc_weights(gen, 2)
    x4 = torch.relu(torch.randn(N, 9, 9, 512, generator=gen))
    for bad in (0, 17):
        rc, lg, cls, clean = _pc_run(L, x4, wt, bad, False, "stride", 1, 1)
        rep.check(rc != 0 and clean and bool((cls == 777.0).all()), ("refusal", "out_ch %d" % bad), "must be refused and write nothing")
    # sensitivity: the crop restated wrongly
    def crop_one_side(x):   # crops although one side is 9
        H, W = x.shape[1], x.shape[2]
        h0, w0 = int((H - 9) * 0.5), int((W - 9) * 0.5)
        return x[:, h0:h0 + 9, w0:w0 + 9]

    def crop_clamped(x):   # a negative start clamped to 0 instead of counted from the end
        H, W = x.shape[1], x.shape[2]
        h0, w0 = max(int((H - 9) * 0.5), 0), max(int((W - 9) * 0.5), 0)
        return x[:, h0:h0 + 9, w0:w0 + 9]

    for key, kind, fn in ((((9, 14), 9), "the crop applied when one side is 9", crop_one_side), (((6, 6), 9), "a slice start clamped to 0 on the 6x6 map", crop_clamped)):
        x4, wt, got, r64, r32 = kept[key]
        _controls(rep, ("control",) + key, got, r64["logits"], r32["logits"], [(kind, _pc_ref(x4, wt, F64, crop=fn)["logits"])])
    rep.finish()


# =====================================================================================================================================================
# decoder entry, max-pool, tile-planar exit
# =====================================================================================================================================================
def _upadd_ref(skip, prev, G, dt):
    return torch.stack([R.upadd(skip, prev[min(g, prev.shape[0] - 1)], dt) for g in range(G)])


@dev_switches
def test_decoder_entry_pool_and_layout_vs_torch():
    L, gen = D.lib(), _gen(34)
    rep = Report("upsample2_add", K_ENTRY)
    N = 2
    for (H, W), Cc, G, shared, roi in (((2, 2), 64, 1, False, None), ((4, 6), 512, 5, True, None), ((6, 10), 64, 5, False, None), ((16, 16), 64, 1, False, None),
                                       ((16, 16), 512, 5, False, None), ((16, 16), 64, 5, True, (5, 11, 3, 9)), ((16, 16), 512, 1, False, (5, 11, 3, 9))):
        case = ("NHWC", "%dx%d" % (H, W), "C%d G%d" % (Cc, G), "shared prev" if shared else "own prev", "roi" if roi else "")
        skip = torch.randn(N, H, W, Cc, generator=gen)
        prev = torch.randn(1 if shared else G, N, H // 2, W // 2, Cc, generator=gen)
        r64, r32 = _upadd_ref(skip, prev, G, F64), _upadd_ref(skip, prev, G, F32)
        out = D.Guarded((G, N, H, W, Cc))
        sd, pd = skip.cuda(), prev.cuda()
        rc = L.cerb_devfwd_upsample2_add_roi(D.ptr(sd), D.ptr(pd), D.ptr(out), G, N, H, W, Cc, 0 if shared else N * (H // 2) * (W // 2) * Cc, None if roi is None else (C.c_int * 4)(*roi), D.stream())
        D.ok(rc, case)
        if roi is None:
            rep.bar(case, "out", out.cpu(), r64, r32)
        else:
            left = _roi_bar(rep, case, out.cpu(), r64, r32, roi)
            rep.check(left > 0, case, "the region leaves something untouched")
        rep.intact(case, out)
    for (H, W), Cc, G, prev_planar, roi in (((20, 20), 64, 2, 0, None), ((20, 20), 128, 1, 1, None), ((12, 36), 256, 2, 1, None), ((12, 36), 64, 1, 0, None), ((20, 20), 256, 1, 0, None),
                                            ((20, 20), 64, 2, 1, (5, 11, 3, 9)), ((12, 36), 128, 2, 0, (2, 9, 17, 30))):
        case = ("planar", "%dx%d" % (H, W), "C%d G%d" % (Cc, G), "prev planar" if prev_planar else "prev NHWC", "roi" if roi else "")
        skip = torch.randn(N, H, W, Cc, generator=gen)
        prev = torch.randn(G, N, H // 2, W // 2, Cc, generator=gen)
        r64, r32 = _upadd_ref(skip, prev, G, F64), _upadd_ref(skip, prev, G, F32)
        idx, size = D._planar_idx(N, H, W, Cc)
        rep.check(size == L.cerb_devfwd_planar_elems(N, H, W, Cc), case, "planar size")
        out = D.Guarded((G * size,), init=torch.zeros(G * size))
        ov = out.t.view(G, size)
        for g in range(G):
            ov[g][idx] = float("nan")
        sd = skip.cuda()
        if prev_planar:
            pd = torch.cat([D._to_planar(prev[g].cuda()) for g in range(G)])
            prev_gs = pd.numel() // G
        else:
            pd, prev_gs = prev.cuda(), N * (H // 2) * (W // 2) * Cc
        rc = L.cerb_devfwd_upsample2_add_planar_roi(D.ptr(sd), D.ptr(pd), D.ptr(out), G, N, H, W, Cc, prev_gs, size, None if roi is None else (C.c_int * 4)(*roi), prev_planar, D.stream())
        D.ok(rc, case)
        got = torch.stack([ov[g][idx] for g in range(G)]).cpu()
        if roi is None:
            rep.bar(case, "out", got, r64, r32)
        else:
            left = _roi_bar(rep, case, got, r64, r32, roi)
            rep.check(left > 0, case, "the region leaves something untouched")
        written = torch.zeros(size, dtype=torch.bool, device="cuda")
        written[idx.reshape(-1)] = True
        rep.check(bool((ov[:, ~written] == 0).all()) and out.intact(), case, "every float no pixel maps to is still zero; sentinel bands")
    for what, H, W, Cc in (("C 96", 20, 20, 96), ("H 18", 18, 20, 64)):
        size = L.cerb_devfwd_planar_elems(N, H, W, Cc)
        out = D.Guarded((size,))
        sd, pd = torch.zeros(N, H, W, Cc, device="cuda"), torch.zeros(N, H // 2, W // 2, Cc, device="cuda")
        rc = L.cerb_devfwd_upsample2_add_planar_roi(D.ptr(sd), D.ptr(pd), D.ptr(out), 1, N, H, W, Cc, pd.numel(), size, None, 0, D.stream())
        torch.cuda.synchronize()
        rep.check(rc != 0 and bool(torch.isnan(out.cpu()).all()) and out.intact(), ("planar refusal", what), "must be refused and write nothing")
    # max-pool 3x3 / 2 / 1: EQUAL to F.max_pool2d; every input below -1, so a border padded with 0 instead of -inf wins the maximum and fails
    pool = Report("maxpool", 0)
    for planar, n, H, W, Cc in ((0, 2, 5, 7, 8), (0, 3, 2, 2, 64), (0, 2, 32, 48, 64), (1, 2, 32, 32, 64), (1, 1, 64, 32, 128)):
        case = ("planar" if planar else "NHWC", n, H, W, Cc)
        x = -torch.randn(n, H, W, Cc, generator=gen).abs() - 1
        ref = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).contiguous()
        Ho, Wo = ref.shape[1:3]
        xd = x.cuda()
        if planar:
            idx, size = D._planar_idx(n, Ho, Wo, Cc)
            out = D.Guarded((size,), init=torch.zeros(size))
            out.t[idx] = float("nan")
        else:
            out = D.Guarded((n, Ho, Wo, Cc))
        D.ok(L.cerb_devfwd_maxpool(D.ptr(xd), D.ptr(out), n, H, W, Cc, planar, D.stream()), case)
        if planar:
            pool.equal(case, "pooled", out.t[idx], ref)
            written = torch.zeros(size, dtype=torch.bool, device="cuda")
            written[idx.reshape(-1)] = True
            pool.check(bool((out.t[~written] == 0).all()), case, "every float no pixel maps to is still zero")
        else:
            pool.equal(case, "pooled", out.cpu(), ref)
        pool.intact(case, out)
    # the tile-planar exit: the inverse of dev_kernels._to_planar
    lay = Report("planar_to_nhwc", 0)
    for n, H, W, Cc in ((3, 16, 16, 64), (1, 32, 48, 128)):
        x = torch.randn(n, H, W, Cc, generator=gen)
        out = D.Guarded((n, H, W, Cc))
        pd = D._to_planar(x.cuda())
        D.ok(L.cerb_devfwd_planar_to_nhwc(D.ptr(pd), D.ptr(out), n, H, W, Cc, D.stream()), (n, H, W, Cc))
        lay.equal((n, H, W, Cc), "NHWC", out.cpu(), x)
        lay.intact((n, H, W, Cc), out)
    for what, H, W, Cc in (("H 20", 20, 16, 64), ("C 32", 16, 16, 32)):
        out = D.Guarded((1, H, W, Cc))
        pd = torch.zeros(L.cerb_devfwd_planar_elems(1, H, W, max(Cc, 64)), device="cuda")
        rc = L.cerb_devfwd_planar_to_nhwc(D.ptr(pd), D.ptr(out), 1, H, W, Cc, D.stream())
        torch.cuda.synchronize()
        lay.check(rc != 0 and bool(torch.isnan(out.cpu()).all()) and out.intact(), ("refusal", what), "must be refused and write nothing")
    _finish_all(rep, pool, lay)
