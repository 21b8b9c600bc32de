"""tests/optim_ref.py against an independent implementation: its float64 mirrors of sgd, sgdm, sgdmom, adagrad and rmsprop
against torch.optim (SGD plain / momentum / Nesterov momentum, Adagrad, RMSprop) at a constant learning rate, without weight
decay and clamp.  With a constant lr, torch's momentum buffer b (b <- a b + g, x <- x - lr b) is sgdm's v / lr, and its
Nesterov step x <- x - lr (g + a b) is sgdmom's -a m + (1 + a) m' with m = -lr b: this pins the reading of the two momentum
rules.  Adam is left out: torch adds eps after the bias correction of v, the reference before it, and ae_ref_torch.Adam
already pins that rule.  Bound 1e-12 absolute: both sides are float64 and differ by the order of a few additions."""
import numpy as np
import pytest
import torch

import optim_ref

N, STEPS = 64, 5
LR, ALPHA, EPS = (float(np.float32(v)) for v in (3e-2, 0.8, 1e-8))  # the mirror takes its scalars through float32, as the device does

CASES = [
    (optim_ref.SGD, lambda p: torch.optim.SGD([p], lr=LR)),
    (optim_ref.SGDM, lambda p: torch.optim.SGD([p], lr=LR, momentum=ALPHA)),
    (optim_ref.SGDMOM, lambda p: torch.optim.SGD([p], lr=LR, momentum=ALPHA, nesterov=True)),
    (optim_ref.ADAGRAD, lambda p: torch.optim.Adagrad([p], lr=LR, eps=EPS)),
    (optim_ref.RMSPROP, lambda p: torch.optim.RMSprop([p], lr=LR, alpha=ALPHA, eps=EPS)),
]


@pytest.mark.parametrize("rule,make", CASES, ids=[optim_ref.NAMES[c[0]] for c in CASES])
def test_float64_mirror_matches_torch_optim(rule, make):
    rng = np.random.default_rng(17 + rule)
    x = rng.uniform(-0.08, 0.08, N)
    grads = [rng.standard_normal(N) * 0.1 for _ in range(STEPS)]
    p = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    opt = make(p)
    mirror = optim_ref.Optim(rule, N, np.float64)
    worst = 0.0
    for g in grads:
        p.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        x, _, _ = mirror.update(x, g, LR, ALPHA, 0.999, EPS, 0.0, 0.0)
        worst = max(worst, float(np.abs(x - p.detach().numpy()).max()))
    print(optim_ref.NAMES[rule], "max |mirror - torch| =", worst)
    assert worst < 1e-12, worst


def test_statistics_and_orders():
    """the two statistics are of x before the update and g after clamp and decay; wd_first swaps clamp and decay"""
    x = np.array([0.5, -0.001, 0.0, 0.2], np.float32)
    g = np.array([1.0, -1.0, 0.0, 1e-4], np.float32)
    got, norm, count = optim_ref.Optim(optim_ref.SGD, 4).update(x, g, 0.1, wd=0.5, clamp=0.01)
    gg = np.clip(g, -0.01, 0.01) + np.float32(0.5) * x            # clamp, then decay
    assert np.array_equal(got, (x - np.float32(0.1) * gg).astype(np.float32))
    assert norm == pytest.approx(float(np.sqrt((x.astype(np.float64) ** 2).sum())))
    assert count == int((np.abs(gg * np.float32(0.1)) >= np.abs(x) * np.float32(0.01)).sum()) == 4
    got2, _, _ = optim_ref.Optim(optim_ref.SGD, 4, wd_first=True).update(x, g, 0.1, wd=0.5, clamp=0.01)
    g2 = np.clip(g + np.float32(0.5) * x, -0.01, 0.01)              # decay, then clamp
    assert np.array_equal(got2, (x - np.float32(0.1) * g2).astype(np.float32))
    assert not np.array_equal(got, got2)
