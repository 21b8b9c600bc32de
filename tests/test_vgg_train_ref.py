"""The float64 fixed-pattern model of the VGG-16 body (tests/vgg_train_ref_torch.py), anchored on the CPU: its forward against
tests/vgg_body_ref.py, its backward against torch autograd through relu / max_pool2d, nn.L2Normalize's backward, the three
scaled update rules against a line-by-line transcription of misc/optim_updates.lua, and -- for the inputs of every GPU case --
how far a float32 run's pattern may stray from the float64 one: the cap tests/test_gpu_vgg_train.py holds the device to."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vgg_body_ref as vref
import vgg_train_ref_torch as vt


@functools.lru_cache(maxsize=None)
def _weights(orc, div, hw):
    return np.asarray(orc.VggOracle(div, hw).synth_weights(), np.float32)  # what set_weights stores


def _relmax(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(np.asarray(b)).max())


@pytest.mark.parametrize("name", ["narrow", "half"])
def test_forward_equals_the_body_model(orc, name):
    c = vt.CASES[name]
    img, x, _ = vt.case_inputs(c)
    w = _weights(orc, c["div"], c["hw"])
    want, m6, m7 = vref.body_fc7_raw(c["div"], c["hw"], w, img, c["xoff"], c["yoff"], c["dr"])
    got, acts, pat, _ = vt.free_forward(c["div"], c["hw"], w, x, c["dr"])
    assert (want > 0).mean() > 0.02
    assert _relmax(got.numpy(), want) < 1e-10
    if c["dr"] is not None:
        assert np.array_equal(pat["fc"][1].numpy() > 0, (m7 > 0) & (pat["fc"][1].numpy() > 0)) and not np.any(got.numpy()[m7 == 0])
    # the fixed-pattern network under the pattern it took is the same function, and the pattern can be read off the outputs
    fixed, facts = vt.fixed_forward(c["div"], c["hw"], torch.as_tensor(w, dtype=torch.float64), x, pat)
    assert _relmax(fixed.numpy(), want) < 1e-10
    back = vt.pattern_of([a.numpy() for a in acts], c["dr"])
    for kind in ("relu", "sel", "fc"):
        for a, b in zip(pat[kind], back[kind]):
            assert _relmax(b.to(torch.float64), a.to(torch.float64)) < 1e-7 if kind == "fc" else torch.equal(a, b)


def _autograd_grads(div, hw, flat, x, dr, dfeats, through_l2norm):
    """the ordinary network through torch's own relu / max_pool2d backward"""
    w = torch.tensor(np.asarray(flat, np.float64), requires_grad=True)
    t = vt.split(div, hw, w)
    h = torch.as_tensor(x)
    for i in range(13):
        h = F.relu(F.conv2d(h, t[2 * i], t[2 * i + 1], padding=1))
        if vt.POOL_AFTER[i]:
            h = F.max_pool2d(h, 2, 2)
    h = h.reshape(h.shape[0], -1)
    drops = vt.fc_masks(h.shape[0], t[26].shape[0], dr)
    for k in range(2):
        h = F.relu(h @ t[26 + 2 * k].t() + t[27 + 2 * k]) * torch.as_tensor(drops[k])
    if through_l2norm:
        h = h / h.norm(dim=1, keepdim=True)
    (h * torch.as_tensor(dfeats, dtype=torch.float64)).sum().backward()
    return w.grad.numpy()


@pytest.mark.parametrize("l2", [False, True])
def test_fixed_pattern_backward_equals_autograd_under_its_own_pattern(orc, l2):
    c = vt.CASES["narrow"]
    _, x, dfeats = vt.case_inputs(c)
    w = _weights(orc, c["div"], c["hw"])
    _, _, pat, _ = vt.free_forward(c["div"], c["hw"], w, x, c["dr"])
    got = vt.fixed_backward(c["div"], c["hw"], w, x, pat, dfeats, l2)
    want = _autograd_grads(c["div"], c["hw"], w, x, c["dr"], dfeats, l2)
    for name, a, b in zip(vt.tensor_names(), vt.split(c["div"], c["hw"], got), vt.split(c["div"], c["hw"], want)):
        assert np.abs(b).max() > 0, name
        assert _relmax(a, b) < 1e-12, (name, _relmax(a, b))


def test_l2normalize_backward_equals_autograd_and_the_lua_formula():
    rng = np.random.default_rng(3)
    n, d = 4, 24
    f, dy = np.abs(rng.standard_normal((n, d))), rng.standard_normal((n, d))
    got = vt.l2norm_backward(f, dy)
    x = torch.tensor(f, requires_grad=True)
    ((x / x.pow(2).sum(1, keepdim=True).sqrt()) * torch.as_tensor(dy)).sum().backward()
    assert _relmax(got, x.grad.numpy()) < 1e-12
    # misc/L2Normalize.lua:22-40, statement by statement
    inp = torch.as_tensor(f)
    norm_squared = (inp * inp).sum(1, keepdim=True)
    buffer = norm_squared.sqrt()
    eye = torch.eye(d, dtype=torch.float64).repeat(n, 1).view(n, d, d)
    diag = eye * norm_squared.view(n, 1, 1).expand(n, d, d)
    diag = diag + (-torch.bmm(inp.view(n, d, 1), inp.view(n, 1, d)))
    diag = diag / buffer.pow(3).view(n, 1, 1).expand(n, d, d)
    lua = torch.bmm(diag, torch.as_tensor(dy).view(n, d, 1)).view(n, d)
    assert _relmax(got, lua.numpy()) < 1e-12


def _lua_rule(rule, x, dx, lr, alpha, beta, epsilon, state, lrs):
    """misc/optim_updates.lua's sgd (:4-10), sgdm (:12-24) and adam (:78-111) with lrs given, line by line on torch tensors"""
    if rule == vt.SGD:
        x.addcmul_(dx, lrs, value=-lr)
    elif rule == vt.SGDM:
        if "v" not in state:
            state["v"] = torch.zeros_like(x)
        state["v"].mul_(alpha)
        state["v"].addcmul_(dx, lrs, value=lr)
        x.add_(state["v"], alpha=-1)
    else:
        if "m" not in state:
            state["t"] = 0
            state["m"] = torch.zeros_like(dx)
            state["v"] = torch.zeros_like(dx)
            state["tmp"] = torch.zeros_like(dx)
        state["m"].mul_(alpha).add_(dx, alpha=1 - alpha)
        state["v"].mul_(beta).addcmul_(dx, dx, value=1 - beta)
        state["tmp"].copy_(state["v"]).sqrt_().add_(epsilon)
        state["t"] = state["t"] + 1
        bias1 = 1 - alpha ** state["t"]
        bias2 = 1 - beta ** state["t"]
        step = lr * np.sqrt(bias2) / bias1
        update = torch.div(state["m"], state["tmp"])
        x.addcmul_(update, lrs, value=-step)


@pytest.mark.parametrize("rule", [vt.SGD, vt.SGDM, vt.ADAM], ids=["sgd", "sgdm", "adam"])
def test_scaled_rules_equal_the_lua_transcription(rule):
    rng = np.random.default_rng(5)
    n, lr, alpha, beta, eps, wd, clamp, scale = 1000, 2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3, 0.01
    x0 = rng.uniform(-0.1, 0.1, n)
    mine, x = vt.ScaledRule(rule, n), x0.copy()
    lx, state, lrs = torch.tensor(x0), {}, torch.full((n,), scale, dtype=torch.float64)
    for it in range(3):
        g = rng.standard_normal(n) * 2e-3
        # the script (arch2 :323-327): weight decay through the scales, then the clamp
        lg = torch.tensor(g)
        lg.add_(torch.mul(lx, lrs), alpha=wd)
        lg.clamp_(-clamp, clamp)
        want_norm = float(lx.norm())
        want_count = int(torch.ge(torch.abs(lg * lr), torch.abs(lx) * 0.01).sum())
        _lua_rule(rule, lx, lg, lr, alpha, beta, eps, state, lrs)
        x, norm, count = mine.update(x, g, lr, alpha, beta, eps, wd, clamp, scale)
        assert _relmax(x, lx.numpy()) < 1e-13
        assert abs(norm - want_norm) < 1e-12 * want_norm and count == want_count and 0 < count < n
    assert _relmax(x, x0) > 1e-6  # the weights moved


@pytest.mark.parametrize("name", sorted(vt.CASES))
def test_float32_pattern_strays_from_float64_only_at_near_ties(orc, name):
    """The cap of the GPU test, shown reachable: on each GPU case's inputs a float32 run of the same network differs from the
    float64 run in at most PATTERN_SHARE of a layer's units, and every such unit is a near-tie (margin below NEAR_TIE of the
    layer's largest magnitude)."""
    c = vt.CASES[name]
    _, x, _ = vt.case_inputs(c)
    w = _weights(orc, c["div"], c["hw"])
    _, _, p64, margins = vt.free_forward(c["div"], c["hw"], w, x, c["dr"])
    _, _, p32, _ = vt.free_forward(c["div"], c["hw"], w, x, c["dr"], torch.float32)
    for layer, units, differ, worst in vt.pattern_diff(p64, p32, margins):
        print(name, layer, "units", units, "differ", differ, "largest margin", worst)
        assert differ <= vt.PATTERN_SHARE * units and worst < vt.NEAR_TIE, (layer, units, differ, worst)
    assert float(p64["relu"][12].double().mean()) > 0.05  # conv5_3 is alive
