"""Plain references of the training step's backward operations, one per kernel family of tests/test_kernel_parity_gpu.py (CPU, torch).

Every operation is torch.nn.functional under autograd on the SAME inputs the kernel gets, in the dtype the caller names: float64 is the reference,
float32 the yardstick `ref32` of the kernel's bar (err(kernel) <= k * err(ref32) + 1e-7 with err(a) = max|a - ref64| / max|ref64| per tensor).
Activations are NHWC with a leading group axis [G][N][H][W][C], weights [G][Cout][Cin][k][k] -- the kernels' own layouts (tests/dev_kernels.py).
Two references are written by hand: wgrad_wino_formula (the F(4x4,3x3) Winograd-domain weight gradient, the second yardstick of that kernel) and
dilate2; tests/test_kernel_refs.py ties both to autograd on the host.  The forward convolutions (tests/test_conv_forward_parity_gpu.py) have conv_forward
(F.conv2d + bias + residual + ReLU, the decoder entry in front of it) and wino_forward_formula, the F(2x2) / F(4x4) algorithm of the Winograd kernels
evaluated plainly: the yardstick of those kernels, tied to conv2d in the same host test.  The stem, the output heads, Patch-Class (its crop a real Python
slice) and the heads' training passes (tests/test_net_kernels_parity_gpu.py, tests/test_head_train_parity_gpu.py) are plain torch expressions under
autograd, tied to the torch.nn module chains in the same host test."""
import torch
import torch.nn.functional as F


def err(a, ref64):
    """max|a - ref64| / max|ref64| of one tensor; NaN / inf anywhere in `a` gives inf (a poisoned output that was accumulated into)."""
    a = a.detach().to(torch.float64).cpu()
    ref64 = ref64.detach().to(torch.float64)
    assert a.shape == ref64.shape, (tuple(a.shape), tuple(ref64.shape))
    if a.numel() == 0:
        return 0.0
    if not bool(torch.isfinite(a).all()):
        return float("inf")
    scale = float(ref64.abs().max())
    d = float((a - ref64).abs().max())
    return d / scale if scale > 0 else (0.0 if d == 0 else float("inf"))


# ---- convolutions -------------------------------------------------------------------------------------------------------------------------------
def conv_grads(x, dy, w, ks, stride, dt, bias_grad=True):
    """x [G][N][H][W][Cin], dy [G][N][Ho][Wo][Cout], w [G][Cout][Cin][ks][ks] or None (zeros: the weight gradient of a convolution does not depend on the
    weights) -> dw [G][Cout][Cin][ks][ks], db [G][Cout], dx [G][N][H][W][Cin] (dx only when w is given).  Padding ks // 2: a 3x3 stride-2 window reads rows
    2 yo - 1 + ky."""
    G, Cin, Cout = x.shape[0], x.shape[-1], dy.shape[-1]
    dws, dbs, dxs = [], [], []
    for g in range(G):
        xg = x[g].permute(0, 3, 1, 2).to(dt).contiguous().requires_grad_(w is not None)
        wg = (torch.zeros(Cout, Cin, ks, ks, dtype=dt) if w is None else w[g].to(dt).clone()).requires_grad_(True)
        bg = torch.zeros(Cout, dtype=dt, requires_grad=True)
        y = F.conv2d(xg, wg, bg, stride=stride, padding=ks // 2)
        go = dy[g].permute(0, 3, 1, 2).to(dt)
        assert y.shape == go.shape, (tuple(y.shape), tuple(go.shape))
        y.backward(go)
        dws.append(wg.grad)
        dbs.append(bg.grad)
        if w is not None:
            dxs.append(xg.grad.permute(0, 2, 3, 1).contiguous())
    return torch.stack(dws), torch.stack(dbs), (torch.stack(dxs) if dxs else None)


_BT = [[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]]
_G = [[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]]
_AT = [[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]]


def wgrad_wino_formula(x, dy, dt):
    """The algorithm of conv_wgrad_wino.hip evaluated plainly in `dt`, with the standard F(4x4,3x3) matrices (Y = A^T [(G g G^T) .* (B^T d B)] A):
    dU = sum over the 4x4-output tiles of (A dY A^T) .* (B^T d B), dg = G^T dU G.  x [G][N][H][W][Cin], dy [G][N][H][W][Cout], H and W multiples of 4."""
    BT, Gm, AT = torch.tensor(_BT, dtype=dt), torch.tensor(_G, dtype=torch.float64).to(dt), torch.tensor(_AT, dtype=dt)
    out = []
    for g in range(x.shape[0]):
        xg, yg = x[g].permute(0, 3, 1, 2).to(dt), dy[g].permute(0, 3, 1, 2).to(dt)
        N, Ci, H, W = xg.shape
        Co, T = yg.shape[1], (H // 4) * (W // 4)
        d = F.unfold(F.pad(xg, (1, 1, 1, 1)), 6, stride=4).view(N, Ci, 6, 6, T)   # the 6x6 input patch of every tile, zero padded
        q = F.unfold(yg, 4, stride=4).view(N, Co, 4, 4, T)                        # its 4x4 output gradients
        V = torch.einsum("ij,ncjkt,lk->ncilt", BT, d, BT)
        Z = torch.einsum("ji,ncjkt,kl->ncilt", AT, q, AT)
        dU = torch.einsum("noabt,niabt->oiab", Z, V)
        out.append(torch.einsum("ax,oiab,by->oixy", Gm, dU, Gm))
    return torch.stack(out)


# ---- forward convolutions -------------------------------------------------------------------------------------------------------------------------
def upadd(skip, prev, dt):
    """skip [N][H][W][C] + bilinear x2 (align_corners=False) of prev [N][H/2][W/2][C], NHWC in and out (the decoder entry, as in upadd_grads)"""
    up = F.interpolate(prev.permute(0, 3, 1, 2).to(dt), scale_factor=2, mode="bilinear", align_corners=False)
    return skip.to(dt) + up.permute(0, 2, 3, 1)


def conv_epilogue(y, bias, resid, relu, dt):
    """y [G][N][Ho][Wo][Cout] (+ bias [G or 1][Cout]) (+ resid, same shape) -> ReLU as asked, in dt"""
    y = y.to(dt)
    if bias is not None:
        y = y + bias.to(dt).view(bias.shape[0], 1, 1, 1, -1)
    if resid is not None:
        y = y + resid.to(dt)
    return torch.relu(y) if relu else y


def conv_forward(x, w, bias, resid, prev, ks, stride, relu, dt):
    """x [G or 1][N][H][W][Cin] (1: every group reads the same input), w [G][Cout][Cin][ks][ks], bias [G or 1][Cout] or None, resid [G][N][Ho][Wo][Cout] or
    None, prev [G or 1][N][H/2][W/2][Cin] or None (then the input of group g is x + bilinear x2 of prev) -> [G][N][Ho][Wo][Cout]: F.conv2d with padding
    ks // 2, + bias, + residual, ReLU as asked.  float64 is the reference, float32 the yardstick of the direct kernel."""
    out = []
    for g in range(w.shape[0]):
        xg = x[min(g, x.shape[0] - 1)]
        xg = xg.to(dt) if prev is None else upadd(xg, prev[min(g, prev.shape[0] - 1)], dt)
        out.append(F.conv2d(xg.permute(0, 3, 1, 2).contiguous(), w[g].to(dt), None, stride=stride, padding=ks // 2).permute(0, 2, 3, 1))
    return conv_epilogue(torch.stack(out), bias, resid, relu, dt)


def dgrad_filter(w):
    """w [G][Cout][Cin][3][3] -> the data-gradient filter [G][Cin][Cout][3][3], W'[ci][co][tap] = W[co][ci][8 - tap] (rotated by 180 degrees, transposed)"""
    return w.flip(-1, -2).transpose(1, 2).contiguous()


_BT2 = [[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]]
_G2 = [[1, 0, 0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0, 0, 1]]
_AT2 = [[1, 1, 1, 0], [0, 1, -1, -1]]


def wino_forward_formula(x, w, m, dt):
    """The algorithm of the Winograd convolution kernels evaluated plainly in `dt`: Y = A^T [(G g G^T) .* (B^T d B), summed over the input channels] A per
    m x m output tile, m = 2 (conv_wino.hip; the matrices of its packer) or m = 4 (conv_wino4*.hip; the matrices above).  The filter transform runs in
    double and is rounded once to dt, as the packers do; maps that are no multiple of m are zero-extended.  x [G or 1][N][H][W][Cin],
    w [G][Cout][Cin][3][3] -> [G][N][H][W][Cout] (3x3, stride 1, zero padding 1; no bias)."""
    bt, gm, at = (_BT2, _G2, _AT2) if m == 2 else (_BT, _G, _AT)
    BT, AT, Gm = torch.tensor(bt, dtype=dt), torch.tensor(at, dtype=dt), torch.tensor(gm, dtype=torch.float64)
    out = []
    for g in range(w.shape[0]):
        xg = x[min(g, x.shape[0] - 1)].permute(0, 3, 1, 2).to(dt)
        N, Ci, H, W = xg.shape
        Hp, Wp = (H + m - 1) // m * m, (W + m - 1) // m * m
        T = (Hp // m) * (Wp // m)
        U = torch.einsum("ax,oixy,by->oiab", Gm, w[g].to(torch.float64), Gm).to(dt)
        d = F.unfold(F.pad(xg, (1, 1 + Wp - W, 1, 1 + Hp - H)), m + 2, stride=m).view(N, Ci, m + 2, m + 2, T)
        V = torch.einsum("ij,ncjkt,lk->ncilt", BT, d, BT)
        M = torch.einsum("oiab,niabt->noabt", U, V)
        Y = torch.einsum("ia,noabt,jb->noijt", AT, M, AT)
        y = F.fold(Y.reshape(N, -1, T), (Hp, Wp), m, stride=m)
        out.append(y[:, :, :H, :W].permute(0, 2, 3, 1))
    return torch.stack(out)


def stem_wgrad(tiles, dy, dt):
    """tiles uint8 [N][H][W][3], dy [N][H][W][64] -> dw [64][3][7][7] of conv2d(tiles / 255, w, padding=3)."""
    x = (tiles.permute(0, 3, 1, 2).to(dt) / 255).contiguous()
    w = torch.zeros(64, 3, 7, 7, dtype=dt, requires_grad=True)
    F.conv2d(x, w, padding=3).backward(dy.permute(0, 3, 1, 2).to(dt))
    return w.grad


# ---- BatchNorm ----------------------------------------------------------------------------------------------------------------------------------
def bn_stats(y, dt, eps=1e-5):
    """y [G][rows][C] -> mean, 1 / sqrt(biased var + eps), unbiased var, each [G][C]."""
    v = y.to(dt)
    m = v.mean(1)
    var = v.var(1, unbiased=False)
    n = v.shape[1]
    return m, 1.0 / torch.sqrt(var + eps), var * (n / max(n - 1, 1))


def bn_forward(y, gamma, beta, resid, relu, eval_groups, run_mean, run_var, dt, eps=1e-5):
    """z = relu?(batch_norm(y) (+ resid)), per group; groups in eval_groups normalise with the running statistics.  Leaves (y, gamma, beta, resid) come
    back too, for bn_backward."""
    G = y.shape[0]
    leaves, zs = [], []
    for g in range(G):
        yv = y[g].to(dt).clone().requires_grad_(True)
        ga, be = gamma[g].to(dt).clone().requires_grad_(True), beta[g].to(dt).clone().requires_grad_(True)
        rs = None if resid is None else resid[g].to(dt).clone().requires_grad_(True)
        ev = g in eval_groups
        z = F.batch_norm(yv, run_mean[g].to(dt).clone() if ev else None, run_var[g].to(dt).clone() if ev else None, ga, be, training=not ev, eps=eps)
        if rs is not None:
            z = z + rs
        if relu:
            z = F.relu(z)
        leaves.append((yv, ga, be, rs))
        zs.append(z)
    return leaves, zs


def bn_backward(leaves, zs, dz, dt):
    """-> dy [G][rows][C], dresid (or None), dgamma [G][C], dbeta [G][C]"""
    for g, z in enumerate(zs):
        z.backward(dz[g].to(dt))
    dy = torch.stack([l[0].grad for l in leaves])
    dres = None if leaves[0][3] is None else torch.stack([l[3].grad for l in leaves])
    return dy, dres, torch.stack([l[1].grad for l in leaves]), torch.stack([l[2].grad for l in leaves])


# ---- decoder entry: out_g = skip + up2(prev_g) ---------------------------------------------------------------------------------------------------
def upadd_grads(dout, shared_prev, live, dt):
    """dout [G][N][H][W][C]; live: per group, False = the group's gradient counts as zero.  -> dskip [N][H][W][C], dprev [G or 1][N][H/2][W/2][C]
    (shared_prev: one `prev` feeds every group, its gradient is the sum over the groups)."""
    G, N, H, W, C = dout.shape
    skip = torch.zeros(N, C, H, W, dtype=dt, requires_grad=True)
    prev = torch.zeros(1 if shared_prev else G, N, C, H // 2, W // 2, dtype=dt, requires_grad=True)
    for g in range(G):
        out = skip + F.interpolate(prev[0 if shared_prev else g], scale_factor=2, mode="bilinear", align_corners=False)
        out.backward(dout[g].permute(0, 3, 1, 2).to(dt) * (1.0 if live[g] else 0.0))
    return skip.grad.permute(0, 2, 3, 1).contiguous(), prev.grad.permute(0, 1, 3, 4, 2).contiguous()


# ---- max-pool 3x3 / 2 / 1 -----------------------------------------------------------------------------------------------------------------------
def maxpool(x, dy, dt):
    """x [N][H][W][C], dy [N][H/2][W/2][C] -> pooled map, dx (the gradient goes to the element torch's CPU backward picks: the first maximum in scan order)."""
    xv = x.permute(0, 3, 1, 2).to(dt).contiguous().requires_grad_(True)
    p = F.max_pool2d(xv, 3, 2, 1)
    p.backward(dy.permute(0, 3, 1, 2).to(dt).contiguous())
    return p.detach().permute(0, 2, 3, 1).contiguous(), xv.grad.permute(0, 2, 3, 1).contiguous()


# ---- pointwise layers ---------------------------------------------------------------------------------------------------------------------------
def pointwise_grads(x, dy, w, in_scale, dt):
    """out = (x * in_scale) @ w^T + b on [rows][cin] -> dx, dw [cout][cin], db [cout]"""
    xv = x.to(dt).clone().requires_grad_(True)
    wv = w.to(dt).clone().requires_grad_(True)
    b = torch.zeros(w.shape[0], dtype=dt, requires_grad=True)
    xs = xv if in_scale is None else xv * in_scale.to(dt)
    (xs @ wv.t() + b).backward(dy.to(dt))
    return xv.grad, wv.grad, b.grad


# ---- small pieces -------------------------------------------------------------------------------------------------------------------------------
def colsum(d, dt):
    """d [G][rows][C] -> [G][C]"""
    return d.to(dt).sum(1)


def crop_gap(x, dg, y0, ch, x0, cw, dt):
    """x [N][H][W][C] -> mean over the window [y0, y0 + ch) x [x0, x0 + cw): [N][C]; and the gradient of x for the upstream dg [N][C]"""
    xv = x.to(dt).clone().requires_grad_(True)
    out = xv[:, y0:y0 + ch, x0:x0 + cw, :].mean((1, 2))
    out.backward(dg.to(dt))
    return out.detach(), xv.grad


def dilate2(dy):
    """dy [n][H/2][W/2][C] -> D [n][H][W][C] with D[:, 2 y, 2 x] = dy[:, y, x], zero elsewhere (exact)"""
    n, h, w, c = dy.shape
    d = torch.zeros(n, 2 * h, 2 * w, c, dtype=dy.dtype)
    d[:, ::2, ::2, :] = dy
    return d


# ---- between the convolutions and the user: stem, output heads, Patch-Class (tests/test_net_kernels_parity_gpu.py) ---------------------------------
def stem_forward(tiles, w, scale, shift, relu, dt):
    """tiles [N][H][W][3] (uint8 or float pixel values), w [64][3][7][7], scale / shift [64] (the folded BatchNorm) -> [N][H][W][64]:
    conv2d(tiles / 255, w * scale, shift, padding = 3), then ReLU as asked"""
    x = (tiles.permute(0, 3, 1, 2).to(dt) / 255).contiguous()
    y = F.conv2d(x, w.to(dt) * scale.to(dt).view(64, 1, 1, 1), shift.to(dt), padding=3)
    return (torch.relu(y) if relu else y).permute(0, 2, 3, 1).contiguous()


def top2_margin(logits):
    """logits [..., C] -> the two largest classes [..., 2] and the gap between their logits (softmax is monotone: the argmax of the probabilities is that of
    the logits, and how close a decision is shows in the logits)"""
    v, i = logits.topk(2, dim=-1)
    return i, v[..., 0] - v[..., 1]


def head_forward(feat, w1, b1, scale, shift, w2, b2, dt):
    """feat [N][H][W][64]; w1 [96][64], b1, scale / shift [96] (the BatchNorm behind the first 1x1, folded), w2 [out][96], b2 [out] ->
    dict(logits [N][H][W][out], prob = softmax, inst = prob[..., 1:], type = argmax, top2 [..., 2], margin)"""
    hid = torch.relu((feat.to(dt) @ w1.to(dt).t() + b1.to(dt)) * scale.to(dt) + shift.to(dt))
    logits = hid @ w2.to(dt).t() + b2.to(dt)
    prob = torch.softmax(logits, -1)
    top2, margin = top2_margin(logits)
    return dict(logits=logits, prob=prob, inst=prob[..., 1:], type=prob.argmax(-1), top2=top2, margin=margin)


def patch_class_crop(x):
    """x [N][Hf][Wf][C] -> the window Patch-Class pools: the centre crop to 9 x 9 as the Python slice x[h0 : h0 + 9] with h0 = int((H - 9) * 0.5) (a negative
    start counts from the end, a stop past the end is clipped: slicing does both), applied only when BOTH sides differ from 9"""
    H, W = x.shape[1], x.shape[2]
    if H != 9 and W != 9:
        h0, w0 = int((H - 9) * 0.5), int((W - 9) * 0.5)
        x = x[:, h0:h0 + 9, w0:w0 + 9]
    return x


def patch_class_forward(x4, bn1_scale, bn1_shift, w1, b1, bn2_scale, bn2_shift, w2, b2, dt, crop=patch_class_crop):
    """x4 [N][Hf][Wf][512]: crop -> average pool -> BN1 -> ReLU -> 1x1 512->256 -> BN2 -> ReLU -> 1x1 256->out (the BatchNorms as scale / shift).
    -> dict(logits [N][out], cls = argmax(softmax), top2, margin)"""
    v = crop(x4.to(dt)).mean((1, 2))
    v = torch.relu(v * bn1_scale.to(dt) + bn1_shift.to(dt))
    h = torch.relu((v @ w1.to(dt).t() + b1.to(dt)) * bn2_scale.to(dt) + bn2_shift.to(dt))
    logits = h @ w2.to(dt).t() + b2.to(dt)
    if logits.shape[-1] > 1:
        top2, margin = top2_margin(logits)
    else:
        top2, margin = torch.zeros(logits.shape[0], 2, dtype=torch.long), torch.full((logits.shape[0],), float("inf"), dtype=dt)
    return dict(logits=logits, cls=torch.softmax(logits, -1).argmax(-1), top2=top2, margin=margin, v=v, h=h)


# ---- the output heads of the training step (tests/test_head_train_parity_gpu.py) -------------------------------------------------------------------
def bn_const(y, mean, rstd, gamma, beta, dt):
    """(y - mean) rstd gamma + beta with the statistics as constants"""
    return (y.to(dt) - mean.to(dt)) * rstd.to(dt) * gamma.to(dt) + beta.to(dt)


def head_train_forward(prev, w1, b1, gamma, beta, w2, b2, dt, in_bn=None, hid=None, stats=None, eps=1e-5):
    """prev [rows][64] -> p = relu(bn_in(prev)) when in_bn = (mean, rstd, gamma, beta) is given, else prev; hid = p W1^T + b1 (or the `hid` handed in: a
    leaf, as for the kernels that take it as an input); z = relu(batch_norm(hid)) with batch statistics, or with stats = (mean, rstd) as constants
    (eval mode); logits = z W2^T + b2.  Returns a dict of the tensors; p, hid (when handed in), w1, b1, gamma, beta, w2, b2 are autograd leaves."""
    t = dict()
    leaf = lambda v: v.detach().to(dt).clone().requires_grad_(True)
    t["w1"], t["b1"], t["gamma"], t["beta"], t["w2"], t["b2"] = [leaf(v) for v in (w1, b1, gamma, beta, w2, b2)]
    p = prev.to(dt) if in_bn is None else torch.relu(bn_const(prev, *in_bn, dt))
    t["p"] = leaf(p)
    t["hid_of_p"] = t["p"] @ t["w1"].t() + t["b1"]
    t["hid"] = t["hid_of_p"] if hid is None else leaf(hid)
    if stats is None:
        bn = F.batch_norm(t["hid"], None, None, t["gamma"], t["beta"], training=True, eps=eps)
    else:
        bn = (t["hid"] - stats[0].to(dt)) * stats[1].to(dt) * t["gamma"] + t["beta"]   # (tests/test_kernel_refs.py: == BatchNorm2d in eval mode)
    t["bn"] = bn
    t["z"] = torch.relu(bn)
    t["logits"] = t["z"] @ t["w2"].t() + t["b2"]
    return t


def head_train_backward(t, dlog, dt, prev=None, in_bn=None):
    """autograd over head_train_forward(hid = a leaf): -> dict(dhid, dw2, db2, dgamma, dbeta, dprev = dhid W1 (the gradient with respect to p, NOT the raw
    prev), dw1, db1) and, with prev / in_bn, in_part = (sum dz, sum dz xhat) of the BatchNorm in front, dz = dprev where relu(bn_in(prev)) > 0"""
    t["logits"].backward(dlog.to(dt))
    dhid = t["hid"].grad
    if t["hid"] is t["hid_of_p"]:
        raise ValueError("hand `hid` to head_train_forward: the backward kernels take it as an input")
    t["hid_of_p"].backward(dhid)
    g = dict(dhid=dhid, dw2=t["w2"].grad, db2=t["b2"].grad, dgamma=t["gamma"].grad, dbeta=t["beta"].grad, dprev=t["p"].grad, dw1=t["w1"].grad, db1=t["b1"].grad)
    if in_bn is not None:
        mean, rstd = in_bn[0].to(dt), in_bn[1].to(dt)
        dz = g["dprev"] * (bn_const(prev, *in_bn, dt) > 0).to(dt)
        g["in_part"] = torch.stack([dz.sum(0), (dz * (prev.to(dt) - mean) * rstd).sum(0)], -1)
    return g


def pointwise_forward(x, w, bias, in_scale, dt):
    """(x * in_scale) @ w^T + bias on [rows][cin]; in_scale [rows][cin] (a dropout mask times 1 / (1 - p), per row and channel) or None"""
    xs = x.to(dt) if in_scale is None else x.to(dt) * in_scale.to(dt)
    return xs @ w.to(dt).t() + bias.to(dt)


def bn_apply(src, resid, mean, rstd, gamma, beta, relu, dt):
    """src [G][rows][C], statistics and affine [G][C]: relu?((src - mean) rstd gamma + beta (+ resid))"""
    v = (src.to(dt) - mean.to(dt).unsqueeze(1)) * (rstd.to(dt) * gamma.to(dt)).unsqueeze(1) + beta.to(dt).unsqueeze(1)
    if resid is not None:
        v = v + resid.to(dt)
    return torch.relu(v) if relu else v
