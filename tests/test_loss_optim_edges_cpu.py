"""CPU side of tests/test_loss_optim_edges_gpu.py: its inputs are what it says they are, and the one bound it derives -- 4 x the
float32 oracle's distance from the float64 oracle on the saturated combo-loss input -- is measured here, next to the distances
that show why every other case keeps the bound stated for it."""
import pytest
import torch

import cdnet_ref as O
import _loss_edge_cases as E


def _combo32(z, m, w, upstream):
    lg = z.clone().requires_grad_(True)
    ch = [O.combo_loss_channel(lg[:, c], m[:, c]) for c in range(z.shape[1])]
    loss = sum(float(wc) * l for wc, l in zip(w.tolist(), ch))
    (loss * upstream).backward()
    return float(loss), [float(c) for c in ch], lg.grad


def test_saturated_combo_loss_float32_oracle_distance_is_what_the_gpu_test_quotes():
    z, m, rows = E.combo_saturation_inputs()
    assert rows == 6 and sorted(set(z[0, 0, :rows, 0].abs().tolist())) == [16.0, 17.0, 25.0]
    assert bool((m[:, :, :rows, :10] == 1).all()) and bool((m[:, :, :rows, 10:] == 0).all())
    w = torch.tensor(O.XBD_CHANNEL_WEIGHTS)
    wl, wch, wg = E.combo_ref(z, m, w, 1.7)
    l32, ch32, g32 = _combo32(z, m, w, 1.7)
    d_loss = abs(l32 - wl) / wl
    d_ch = max(abs(a - b) / max(1.0, b) for a, b in zip(ch32, wch))
    d_grad = float((g32.double() - wg).abs().max() / wg.abs().max())
    print("saturated combo: float32 oracle vs float64 oracle: loss %.3e, worst channel %.3e, gradient %.3e of max" % (d_loss, d_ch, d_grad))
    # the figures in the GPU test's comment (1.974e-4, 2.004e-4): its bounds 7.9e-4 / 8.0e-4 are 4 x these
    assert d_loss == pytest.approx(1.974e-4, rel=2e-2) and d_ch == pytest.approx(2.004e-4, rel=2e-2)
    assert d_loss > 2e-6                  # the stated bound is out of a float32 implementation's reach here ...
    assert 4 * d_grad < 1e-5              # ... the gradient's is not


def test_well_conditioned_combo_inputs_leave_the_stated_bounds_in_reach():
    """at COMBO_SCALE the float32 oracle is within a quarter of the stated 2e-6 / 1e-5 of its float64 self"""
    for shape, seed in (((3, 5, 211, 157), 5100 + 211), ((2, 1, 24, 20), 5301), ((2, 16, 24, 20), 5316)):
        z, m = E.combo_inputs(*shape, seed)
        w = torch.rand(shape[1], generator=torch.Generator().manual_seed(5200 + shape[1])) + 0.05
        wl, wch, wg = E.combo_ref(z, m, w, 1.7)
        l32, ch32, g32 = _combo32(z, m, w, 1.7)
        assert 4 * abs(l32 - wl) <= 2e-6 * wl
        assert 4 * float((g32.double() - wg).abs().max()) <= 1e-5 * float(wg.abs().max())


@pytest.mark.parametrize("C", [2, 5])
def test_saturated_and_tied_inputs_are_what_they_claim(C):
    z, tgt = E.saturation_inputs(C)
    ref = z.double().requires_grad_(True)
    want = O.focal_loss(ref, tgt)
    want.backward()
    assert bool(torch.isfinite(ref.grad).all())
    # the mean stays small enough for 1e-6 absolute to be a float32 statement: the float32 oracle is within 2.5e-7
    assert float(want) < 4.0 and 4 * abs(float(O.focal_loss(z, tgt)) - float(want)) < 1e-6
    gap = (z.max(1).values - z.min(1).values).reshape(-1)
    assert int((gap > 104.0).sum()) >= 8
    assert float(torch.exp(torch.tensor(-104.0))) == 0.0             # float32 expf underflows to exactly 0 there
    zt, tt, binary = E.tie_inputs(C)
    assert E.tied_fraction(zt) >= 0.5
    assert set((zt * 2).reshape(-1).tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert all(int((tt == v).sum()) > 0 for v in (255, C, -1))


def test_grid_pass_arithmetic_of_the_shapes():
    stride = 1024 * 256
    regimes = []
    for B, H, W in E.PASS_SHAPES:
        HW = H * W
        assert B * HW > stride                                       # a second pass of the loss and metric kernels
        regimes.append((stride // HW, stride % HW))
    assert regimes == [(0, 262144), (4, 46852), (657, 1)]            # focal_kernel's (db, dp)
    assert E.CE_BWD_SHAPE[1] * E.CE_BWD_SHAPE[2] > 4096 * 256
    assert 3 * 211 * 157 > 256 * 256 and 3 * 5 * 531 * 527 > 16384 * 256
    assert E.OPT_N == 3 * 4096 * 256 + 77 and E.OPT_N // 4 > 1024 * 256
    N, C, H, W = E.POOL_LARGE
    assert N * (H // 2) * (W // 2) * (C // 4) > 8192 * 256
