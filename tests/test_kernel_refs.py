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


def test_err_reports_a_poisoned_output_as_infinite():
    ref = torch.ones(4, dtype=torch.float64)
    a = torch.ones(4)
    assert R.err(a, ref) == 0.0
    a[2] = float("nan")
    assert R.err(a, ref) == float("inf")
    assert abs(R.err(torch.tensor([1.0, 3.0]), torch.tensor([1.0, 2.0], dtype=torch.float64)) - 0.5) < 1e-15
