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


def test_err_reports_a_poisoned_output_as_infinite():
    ref = torch.ones(4, dtype=torch.float64)
    a = torch.ones(4)
    assert R.err(a, ref) == 0.0
    a[2] = float("nan")
    assert R.err(a, ref) == float("inf")
    assert abs(R.err(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0], dtype=torch.float64)) - 0.5) < 1e-15
