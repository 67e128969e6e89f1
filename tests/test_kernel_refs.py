"""The hand-written references of tests/kernel_refs.py against autograd, on the host: a reference that is wrong pins a kernel to the wrong answer."""
import torch

import kernel_refs as R


def test_hand_written_references_equal_autograd_in_float64():
    gen = torch.Generator().manual_seed(7)
    # the F(4x4,3x3) Winograd-domain weight gradient == the weight gradient of conv2d, to rounding of float64: one tile row, a non-square map with a
    # partial chunk of tiles, several images (a tile at the top of image n + 1 must see zero padding, not image n) and groups
    for G, N, H, W, Ci, Co in ((1, 1, 8, 8, 8, 4), (1, 1, 12, 20, 4, 8), (2, 3, 12, 20, 8, 8), (1, 2, 28, 28, 4, 4)):
        x = torch.relu(torch.randn(G, N, H, W, Ci, generator=gen))
        dy = 1e-3 * torch.randn(G, N, H, W, Co, generator=gen)
        ref, _, _ = R.conv_grads(x, dy, None, 3, 1, torch.float64)
        got = R.wgrad_wino_formula(x, dy, torch.float64)
        e = R.err(got, ref)
        print("wgrad_wino_formula", (G, N, H, W, Ci, Co), "err vs autograd %.2e" % e)
        assert e <= 1e-12, ((G, N, H, W, Ci, Co), e)
        # ... and its float32 evaluation is a usable yardstick: away from zero, far below any defect of interest
        e32 = R.err(R.wgrad_wino_formula(x, dy, torch.float32), ref)
        assert 0 < e32 < 1e-4, e32
    # dilate2 == the gradient of the strided slice D[:, ::2, ::2] (exactly)
    dy = torch.randn(3, 3, 5, 8, generator=gen, dtype=torch.float64)
    D = torch.zeros(3, 6, 10, 8, dtype=torch.float64, requires_grad=True)
    D[:, ::2, ::2, :].backward(dy)
    assert torch.equal(R.dilate2(dy), D.grad)


def test_winograd_forward_formulas_equal_conv2d_in_float64():
    """F(2x2,3x3) and F(4x4,3x3) evaluated plainly == conv2d to rounding of float64, on maps that are multiples of the tile and maps that are not (zero
    extension), with several images and groups, own and shared input; their float32 evaluations are usable yardsticks."""
    gen = torch.Generator().manual_seed(8)
    for G, Gx, N, H, W, Ci, Co in ((1, 1, 2, 18, 22, 8, 4), (1, 1, 1, 16, 16, 16, 8), (1, 1, 1, 7, 7, 16, 8), (2, 2, 2, 8, 12, 4, 8), (3, 1, 1, 3, 5, 4, 4)):
        x = torch.relu(torch.randn(Gx, N, H, W, Ci, generator=gen))
        w = torch.randn(G, Co, Ci, 3, 3, generator=gen) / (3 * Ci ** 0.5)
        ref = R.conv_forward(x, w, None, None, None, 3, 1, 0, torch.float64)
        for m in (2, 4):
            e = R.err(R.wino_forward_formula(x, w, m, torch.float64), ref)
            print("wino_forward_formula F(%dx%d)" % (m, m), (G, Gx, N, H, W, Ci, Co), "err vs conv2d %.2e" % e)
            assert e <= 1e-12, ((G, N, H, W, Ci, Co), m, e)
            e32 = R.err(R.wino_forward_formula(x, w, m, torch.float32), ref)
            assert 0 < e32 < 1e-4, e32


def test_conv_forward_is_conv2d_with_bias_residual_relu_and_the_decoder_entry():
    gen = torch.Generator().manual_seed(9)
    G, N, H, W, Ci, Co = 2, 2, 4, 6, 4, 8
    skip = torch.randn(1, N, H, W, Ci, generator=gen, dtype=torch.float64)
    prev = torch.randn(G, N, H // 2, W // 2, Ci, generator=gen, dtype=torch.float64)
    w = torch.randn(G, Co, Ci, 3, 3, generator=gen, dtype=torch.float64)
    bias = torch.randn(G, Co, generator=gen, dtype=torch.float64)
    resid = torch.randn(G, N, H // 2, W // 2, Co, generator=gen, dtype=torch.float64)
    got = R.conv_forward(skip, w, bias, resid, prev, 3, 2, 1, torch.float64)
    for g in range(G):
        xin = skip[0].permute(0, 3, 1, 2) + torch.nn.functional.interpolate(prev[g].permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=False)
        y = torch.nn.functional.conv2d(xin, w[g], bias[g], stride=2, padding=1) + resid[g].permute(0, 3, 1, 2)
        assert torch.allclose(got[g], torch.relu(y).permute(0, 2, 3, 1), rtol=0, atol=1e-13)
    # dx of a convolution == the forward convolution of dy with the rotated, transposed filter (what the data-gradient launches compute)
    x = torch.randn(G, N, H, W, Ci, generator=gen)
    dy = torch.randn(G, N, H, W, Co, generator=gen)
    w32 = torch.randn(G, Co, Ci, 3, 3, generator=gen)
    dx = R.conv_grads(x, dy, w32, 3, 1, torch.float64)[2]
    assert R.err(R.conv_forward(dy, R.dgrad_filter(w32), None, None, None, 3, 1, 0, torch.float64), dx) <= 1e-13


def _rand_bn(bn, gen):
    """a BatchNorm module with random affine and running statistics -> its eval-mode fold (scale, shift)"""
    C = bn.num_features
    with torch.no_grad():
        bn.weight.copy_(0.5 + torch.rand(C, generator=gen, dtype=torch.float64))
        bn.bias.copy_(0.1 * torch.randn(C, generator=gen, dtype=torch.float64))
        bn.running_mean.copy_(0.2 * torch.randn(C, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(0.5 + torch.rand(C, generator=gen, dtype=torch.float64))
    scale = bn.weight.detach() / torch.sqrt(bn.running_var + bn.eps)
    return scale, bn.bias.detach() - bn.running_mean * scale


def _rand_conv(conv, gen):
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=gen, dtype=torch.float64) / conv.weight[0].numel() ** 0.5)
        if conv.bias is not None:
            conv.bias.copy_(0.1 * torch.randn(conv.bias.shape, generator=gen, dtype=torch.float64))


def test_stem_and_head_references_equal_the_torch_nn_chains_in_float64():
    nn, gen = torch.nn, torch.Generator().manual_seed(21)
    # stem: Conv2d(3, 64, 7, padding 3, no bias) on tiles / 255 -> BatchNorm2d in eval mode -> ReLU, on bytes and on float pixel values
    conv, bn = nn.Conv2d(3, 64, 7, padding=3, bias=False).double(), nn.BatchNorm2d(64).double().eval()
    _rand_conv(conv, gen)
    scale, shift = _rand_bn(bn, gen)
    for tiles in (torch.randint(0, 256, (2, 5, 7, 3), generator=gen, dtype=torch.uint8), 300 * torch.rand(3, 13, 9, 3, generator=gen) - 20):
        x = tiles.permute(0, 3, 1, 2).double() / 255.0
        with torch.no_grad():
            raw, full = conv(x), torch.relu(bn(conv(x)))
        assert R.err(R.stem_forward(tiles, conv.weight.detach(), scale, shift, 1, torch.float64), full.permute(0, 2, 3, 1)) <= 1e-14
        one, zero = torch.ones(64, dtype=torch.float64), torch.zeros(64, dtype=torch.float64)
        assert R.err(R.stem_forward(tiles, conv.weight.detach(), one, zero, 0, torch.float64), raw.permute(0, 2, 3, 1)) <= 1e-14
        e32 = R.err(R.stem_forward(tiles, conv.weight.detach().float(), scale.float(), shift.float(), 1, torch.float32), full.permute(0, 2, 3, 1))
        assert 0 < e32 < 1e-5, e32
    # output head: Conv2d(64, 96, 1) -> BatchNorm2d eval -> ReLU -> Conv2d(96, out, 1); Softmax over the channels
    for out in (2, 3, 7, 8):
        c1, b1, c2 = nn.Conv2d(64, 96, 1).double(), nn.BatchNorm2d(96).double().eval(), nn.Conv2d(96, out, 1).double()
        _rand_conv(c1, gen)
        _rand_conv(c2, gen)
        scale, shift = _rand_bn(b1, gen)
        feat = torch.relu(torch.randn(2, 3, 16, 64, generator=gen, dtype=torch.float64))
        with torch.no_grad():
            logits = c2(torch.relu(b1(c1(feat.permute(0, 3, 1, 2)))))
            prob = nn.Softmax(dim=1)(logits)
        r = R.head_forward(feat, c1.weight.detach().view(96, 64), c1.bias.detach(), scale, shift, c2.weight.detach().view(out, 96), c2.bias.detach(), torch.float64)
        assert R.err(r["logits"], logits.permute(0, 2, 3, 1)) <= 1e-14 and R.err(r["prob"], prob.permute(0, 2, 3, 1)) <= 1e-14
        assert torch.equal(r["inst"], r["prob"][..., 1:]) and torch.equal(r["type"], prob.argmax(1))
        assert torch.equal(r["top2"][..., 0], r["type"]) and bool((r["margin"] >= 0).all())
        srt = r["logits"].sort(-1, descending=True).values
        assert torch.equal(r["margin"], srt[..., 0] - srt[..., 1])


def test_patch_class_reference_is_the_module_chain_behind_a_real_slice():
    """crop (only when both sides differ from 9) -> AdaptiveAvgPool2d(1) -> bn1, relu1, (dropout: identity in eval mode), conv1, bn2, relu2, conv2"""
    nn, gen = torch.nn, torch.Generator().manual_seed(22)
    windows = {(9, 9): (9, 9), (14, 14): (9, 9), (8, 8): (8, 8), (6, 6): (1, 1), (3, 8): (3, 8), (9, 14): (9, 14), (1, 1): (1, 1)}
    for (H, W), win in windows.items():
        x = torch.arange(2 * H * W * 1, dtype=torch.float64).view(2, H, W, 1)
        c = R.patch_class_crop(x)
        assert tuple(c.shape[1:3]) == win, ((H, W), tuple(c.shape))
    assert R.patch_class_crop(torch.arange(36.0).view(1, 6, 6, 1)).item() == 35.0          # rows [5, 6) x columns [5, 6): the negative start counts from the end
    assert torch.equal(R.patch_class_crop(torch.arange(196.0).view(1, 14, 14, 1)), torch.arange(196.0).view(1, 14, 14, 1)[:, 2:11, 2:11])
    for out in (1, 2, 9, 16):
        chain = nn.Sequential(nn.BatchNorm2d(512), nn.ReLU(), nn.Dropout(0.3), nn.Conv2d(512, 256, 1), nn.BatchNorm2d(256), nn.ReLU(), nn.Conv2d(256, out, 1)).double().eval()
        _rand_conv(chain[3], gen)
        _rand_conv(chain[6], gen)
        s1, h1 = _rand_bn(chain[0], gen)
        s2, h2 = _rand_bn(chain[4], gen)
        for H, W in windows:
            x4 = torch.relu(torch.randn(2, H, W, 512, generator=gen, dtype=torch.float64))
            xc = x4.permute(0, 3, 1, 2)
            if H != 9 and W != 9:   # net_desc.py:173-174 with cropping_center(batch=True)
                h0, w0 = int((H - 9) * 0.5), int((W - 9) * 0.5)
                xc = xc[:, :, h0:h0 + 9, w0:w0 + 9]
            with torch.no_grad():
                logits = chain(nn.AdaptiveAvgPool2d((1, 1))(xc)).view(2, out)
            r = R.patch_class_forward(x4, s1, h1, chain[3].weight.detach().view(256, 512), chain[3].bias.detach(), s2, h2, chain[6].weight.detach().view(out, 256),
                                      chain[6].bias.detach(), torch.float64)
            assert R.err(r["logits"], logits) <= 1e-14, ((H, W), out)
            assert torch.equal(r["cls"], torch.softmax(logits, -1).argmax(-1))


def test_head_training_references_equal_the_module_chain_under_autograd():
    """p = relu(bn_in(prev)); Conv2d(64, 96, 1) -> BatchNorm2d (train and eval mode) -> ReLU -> Conv2d(96, out, 1), forward and every gradient; dprev is the
    gradient with respect to p, in_part the backward sums of the BatchNorm in front"""
    nn, gen = torch.nn, torch.Generator().manual_seed(23)
    rows = 48
    for out, train, with_in in ((2, True, False), (3, True, True), (7, False, True), (7, True, False)):
        c1, bn, c2 = nn.Conv2d(64, 96, 1).double(), nn.BatchNorm2d(96).double(), nn.Conv2d(96, out, 1).double()
        _rand_conv(c1, gen)
        _rand_conv(c2, gen)
        _rand_bn(bn, gen)
        bn.train(train)
        prev = torch.randn(rows, 64, generator=gen, dtype=torch.float64)
        dlog = torch.randn(rows, out, generator=gen, dtype=torch.float64)
        in_bn = None
        if with_in:
            in_bn = (prev.mean(0), 1.0 / torch.sqrt(prev.var(0, unbiased=False) + 1e-5), 0.5 + torch.rand(64, generator=gen, dtype=torch.float64),
                     0.1 * torch.randn(64, generator=gen, dtype=torch.float64))
        prev_leaf = prev.clone().requires_grad_(True)
        p = prev_leaf if in_bn is None else torch.relu((prev_leaf - in_bn[0]) * in_bn[1] * in_bn[2] + in_bn[3])   # (statistics as constants)
        p.retain_grad()
        hid = c1(p.t().reshape(1, 64, rows, 1))
        hid.retain_grad()
        mom = bn.momentum
        bn.momentum = 0.0   # (the running statistics stay what the eval-mode reference is handed)
        logits = c2(torch.relu(bn(hid)))
        bn.momentum = mom
        logits.backward(dlog.t().reshape(1, out, rows, 1))
        flat = lambda v: v.detach().reshape(v.shape[1], rows).t()
        stats = None if train else (bn.running_mean.clone(), 1.0 / torch.sqrt(bn.running_var + bn.eps))
        args = (prev, c1.weight.detach().view(96, 64), c1.bias.detach(), bn.weight.detach(), bn.bias.detach(), c2.weight.detach().view(out, 96), c2.bias.detach(), torch.float64)
        fwd = R.head_train_forward(*args, in_bn=in_bn)
        assert R.err(fwd["hid"], flat(hid)) <= 1e-14 and R.err(fwd["p"], p.detach()) <= 1e-14
        t = R.head_train_forward(*args, in_bn=in_bn, hid=flat(hid), stats=stats)
        assert R.err(t["logits"], flat(logits)) <= 1e-13
        g = R.head_train_backward(t, dlog, torch.float64, prev=prev, in_bn=in_bn)
        want = dict(dhid=flat(hid.grad), dw2=c2.weight.grad.view(out, 96), db2=c2.bias.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, dprev=p.grad, dw1=c1.weight.grad.view(96, 64),
                    db1=c1.bias.grad)
        for k, v in want.items():
            if k == "db1" and train:   # behind batch statistics sum(dhid) is zero by construction: both are rounding noise of a sum of terms of size |dhid|
                assert float((g[k] - v).abs().max()) <= 1e-12 * float(g["dhid"].abs().sum(0).max()) and float(v.abs().max()) <= 1e-12 * float(g["dhid"].abs().sum(0).max())
                continue
            assert R.err(g[k], v) <= 1e-12, (k, out, train, with_in, R.err(g[k], v))
        if with_in:   # the sums of a BatchNorm backward over dz = the gradient behind its ReLU: sum dz = d/d beta, sum dz xhat = d/d gamma
            ga = in_bn[2].clone().requires_grad_(True)
            be = in_bn[3].clone().requires_grad_(True)
            torch.relu((prev - in_bn[0]) * in_bn[1] * ga + be).backward(p.grad)
            assert R.err(g["in_part"][:, 0], be.grad) <= 1e-12 and R.err(g["in_part"][:, 1], ga.grad) <= 1e-12
    # the separate passes: Conv2d 1x1 with a per-channel input scale, and BatchNorm2d applied with given statistics (+ residual, ReLU)
    x, sc = torch.randn(33, 64, generator=gen, dtype=torch.float64), (torch.rand(33, 64, generator=gen) > 0.3).double() / 0.7
    c = nn.Conv2d(64, 7, 1).double()
    _rand_conv(c, gen)
    with torch.no_grad():
        y = c((x * sc).t().reshape(1, 64, 33, 1)).view(7, 33).t()
    assert R.err(R.pointwise_forward(x, c.weight.detach().view(7, 64), c.bias.detach(), sc, torch.float64), y) <= 1e-14
    bn = nn.BatchNorm2d(96).double().eval()
    _rand_bn(bn, gen)
    src, res = torch.randn(2, 33, 96, generator=gen, dtype=torch.float64), torch.randn(2, 33, 96, generator=gen, dtype=torch.float64)
    G2 = lambda v: torch.stack([v.detach(), v.detach()])
    with torch.no_grad():
        y = torch.relu(torch.stack([bn(src[g].t().reshape(1, 96, 33, 1)).view(96, 33).t() for g in range(2)]) + res)
    got = R.bn_apply(src, res, G2(bn.running_mean), G2(1.0 / torch.sqrt(bn.running_var + bn.eps)), G2(bn.weight), G2(bn.bias), 1, torch.float64)
    assert R.err(got, y) <= 1e-14


def test_err_reports_a_poisoned_output_as_infinite():
    ref = torch.ones(4, dtype=torch.float64)
    a = torch.ones(4)
    assert R.err(a, ref) == 0.0
    a[2] = float("nan")
    assert R.err(a, ref) == float("inf")
    assert abs(R.err(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0], dtype=torch.float64)) - 0.5) < 1e-15
