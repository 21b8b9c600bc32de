"""Fine-tuning the VGG-16 body on the device (nvqa_vgg16_train_* / _backward / _update) against the float64 fixed-pattern model
of tests/vgg_train_ref_torch.py, at three sizes: a narrow network (general loaders, K = 12 at conv5_x, many slabs at conv1_x),
a half-width one (C_in a multiple of the tiles) and full-width tiles, each with n < max_batch, one with drop6 / drop7 live.

Bounds.  Saved activations: 1e-4 of the layer's largest value, the forward tests' bound.  Pattern: the device's ReLU masks,
pool selections and fc masks, read off its saved activations, may differ from the float64 run's in at most 1e-4 of a layer's
units, each a near-tie (margin below 1e-4 of the layer's largest magnitude) -- the cap tests/test_vgg_train_ref.py shows a
float32 run to keep.  Gradients, on the device's own pattern: per tensor max |g - g64| / max |g64| <= max(1e-4, 8 d32), d32 the
same distance of the same backward run in torch float32 (the factor 8: slabs are summed in another order than torch's sums).
Update: tests/test_gpu_optim.py's bounds (max |x - mirror| < 1e-6, norm 1e-6 relative, count within max(2, count // 1000))."""
import functools

import numpy as np
import pytest
import torch

import vgg_body_ref as vref
import vgg_train_ref_torch as vt

pytestmark = pytest.mark.gpu

TOL_ACT, TOL_X, TOL_NORM = 1e-4, 1e-6, 1e-6
LR, ALPHA, BETA, EPS, WD, CLAMP, SCALE = 2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3, 0.01
# (lr, wd, clamp) per rule, scale 0.01 throughout, chosen so that every part of a rule moves a weight by far more than TOL_X:
# sgd / sgdm step by lr scale |g| <= 1 x 0.01 x 0.1 = 1e-3 (the clamp acts: the bias gradients of fc7 are O(1)), the decay term
# wd (scale x) = 0.005 x shifts g by up to 5e-3 and the step by up to 5e-5, sgdm's second step carries 0.8 x the first (wd = 1
# would put every weight with a zero gradient exactly on the statistics' tie |lr g| = 0.01 |x|).  Adam steps by
# lr scale = 2e-4 whatever |g| is; a larger rate would only scale up the float32 formula's own conditioning where wd x and
# the clamped gradient cancel to |g| ~ eps (tests/test_gpu_optim.py's docstring on adagrad).
RULE_ARGS = {vt.SGD: (1.0, 0.5, 0.1), vt.SGDM: (1.0, 0.5, 0.1), vt.ADAM: (LR, WD, CLAMP)}
MIN_STEP, TOL_STEP = 1e-4, 1e-3  # the largest move of an update is at least MIN_STEP, and the error at most TOL_STEP of it


@functools.lru_cache(maxsize=None)
def _weights(orc, div, hw):
    return np.asarray(orc.VggOracle(div, hw).synth_weights(), np.float32)  # what set_weights stores


def _relmax(a, b):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b)).max())


def _dropout(pkg, c):
    return pkg.binding.Dropout(*c["dr"]) if c["dr"] is not None else None


def _body(pkg, orc, c, w=None, train=True):
    v = pkg.binding.Vgg16(0, c["div"], c["hw"], max_batch=c["n"] + 1)
    v.set_weights(_weights(orc, c["div"], c["hw"]) if w is None else w)
    if train:
        v.train_enable(True)
    return v


@functools.lru_cache(maxsize=None)
def _reference(orc, name):
    """the float64 run of a case, computed once"""
    c = vt.CASES[name]
    img, x, dfeats = vt.case_inputs(c)
    w = _weights(orc, c["div"], c["hw"])
    feats, acts, pat, margins = vt.free_forward(c["div"], c["hw"], w, x, c["dr"])
    return dict(img=img, x=x, dfeats=dfeats, w=w, feats=feats.numpy(), acts=[a.numpy() for a in acts], pat=pat, margins=margins)


@functools.lru_cache(maxsize=None)
def _device(pkg, orc, name):
    """one device run of a case: features on both routes, the saved activations, three backward passes"""
    c, r = vt.CASES[name], _reference(orc, name)
    dr = _dropout(pkg, c)
    v = _body(pkg, orc, c, train=False)
    try:
        out = {"frozen_before": v.fc7_raw(r["img"], c["xoff"], c["yoff"], dropout=dr)}
        v.train_enable(True)
        out["frozen_after"] = v.fc7_raw(r["img"], c["xoff"], c["yoff"], dropout=dr)
        out["feats"] = v.train_forward_raw(r["img"], c["xoff"], c["yoff"], dropout=dr)
        out["acts"] = [v.train_activation(i) for i in range(15)]
        v.backward(r["dfeats"])
        out["grads"] = v.get_grads()
        v.backward(r["dfeats"])
        out["grads_again"] = v.get_grads()
        v.backward(r["dfeats"], through_l2norm=True)
        out["grads_l2"] = v.get_grads()
    finally:
        v.close()
    return out


def _check_grads(c, r, pat, got, l2, label):
    """every tensor of `got` against the float64 fixed-pattern backward on `pat`, bound max(1e-4, 8 d32)"""
    g64 = vt.fixed_backward(c["div"], c["hw"], r["w"], r["x"], pat, r["dfeats"], l2)
    g32 = vt.fixed_backward(c["div"], c["hw"], r["w"], r["x"], pat, r["dfeats"], l2, torch.float32)
    bad = []
    for name, a, b32, b in zip(vt.tensor_names(), vt.split(c["div"], c["hw"], got), vt.split(c["div"], c["hw"], g32),
                               vt.split(c["div"], c["hw"], g64)):
        assert np.abs(b).max() > 0, name
        d32, err = _relmax(b32, b), _relmax(a, b)
        bound = max(1e-4, 8 * d32)
        print("%s %s: d32 %.3e device %.3e bound %.3e" % (label, name, d32, err, bound))
        if not err <= bound:
            bad.append((name, d32, err, bound))
    assert not bad, bad


CASE_NAMES = sorted(vt.CASES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_training_forward_keeps_the_frozen_bits(pkg, orc, name):
    d = _device(pkg, orc, name)
    assert (d["feats"] > 0).mean() > 0.02
    assert np.array_equal(d["feats"], d["frozen_before"])
    assert np.array_equal(d["frozen_after"], d["frozen_before"])
    assert np.array_equal(d["acts"][14], d["feats"])


@pytest.mark.parametrize("name", CASE_NAMES)
def test_saved_activations_match_float64(pkg, orc, name):
    d, r = _device(pkg, orc, name), _reference(orc, name)
    for i, (got, want) in enumerate(zip(d["acts"], r["acts"])):
        assert got.shape == want.shape
        err = _relmax(got, want)
        print(name, "layer", i, "rel-max err", err)
        assert err < TOL_ACT, (i, err)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_device_pattern_differs_from_float64_only_at_near_ties(pkg, orc, name):
    c, d, r = vt.CASES[name], _device(pkg, orc, name), _reference(orc, name)
    pat = vt.pattern_of(d["acts"], c["dr"])
    for layer, units, differ, worst in vt.pattern_diff(r["pat"], pat, r["margins"]):
        print(name, layer, "units", units, "differ", differ, "largest margin", worst)
        assert differ <= vt.PATTERN_SHARE * units and worst < vt.NEAR_TIE, (layer, units, differ, worst)


@pytest.mark.parametrize("l2", [False, True], ids=["plain", "l2norm"])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_gradients_match_the_fixed_pattern_backward(pkg, orc, name, l2):
    c, d, r = vt.CASES[name], _device(pkg, orc, name), _reference(orc, name)
    _check_grads(c, r, vt.pattern_of(d["acts"], c["dr"]), d["grads_l2" if l2 else "grads"], l2, name)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_backward_is_bit_reproducible(pkg, orc, name):
    d = _device(pkg, orc, name)
    assert np.array_equal(d["grads"], d["grads_again"])
    assert not np.array_equal(d["grads"], d["grads_l2"])


def test_get_weights_inverts_set_weights(pkg, orc):
    for name in ("narrow", "half"):
        c = vt.CASES[name]
        v = _body(pkg, orc, c, train=False)
        try:
            assert np.array_equal(v.get_weights(), _weights(orc, c["div"], c["hw"]))
        finally:
            v.close()


def _count_ok(count, want):
    return abs(count - want) <= max(2, want // 1000)


@pytest.mark.parametrize("rule", [vt.SGD, vt.SGDM, vt.ADAM], ids=["sgd", "sgdm", "adam"])
def test_update_matches_the_float64_rule(pkg, orc, rule):
    """two updates per rule (the second exercises the rule's state) on the device's own gradients, wd > 0, scale 0.01; the
    error is held to 1e-6 absolute and to 1e-3 of the update's largest move, which is itself at least 1e-4: a wrong sign, a
    missing momentum, decay or scale term, or a kernel that does nothing fails"""
    c, r = vt.CASES["narrow"], _reference(orc, "narrow")
    dr = _dropout(pkg, c)
    v = _body(pkg, orc, c)
    mirror = vt.ScaledRule(rule, r["w"].size)
    lr, wd, clamp = RULE_ARGS[rule]
    try:
        x = v.get_weights()
        for it in range(2):
            v.train_forward_raw(r["img"], c["xoff"], c["yoff"], dropout=dr, want_feats=False)
            v.backward(r["dfeats"])
            g = v.get_grads()
            norm, count = v.update(rule, lr, ALPHA, BETA, EPS, wd, clamp, SCALE)
            want, wnorm, wcount = mirror.update(x, g, *(np.float32(a).item() for a in (lr, ALPHA, BETA, EPS, wd, clamp, SCALE)))
            x_old, x = x, v.get_weights()
            err, step = float(np.abs(x - want).max()), float(np.abs(want - x_old).max())
            print("rule", rule, "step", it, "max_abs", err, "largest move", step, "norm", norm, wnorm, "count", count, wcount)
            assert step >= MIN_STEP, step
            assert err < TOL_X and err <= TOL_STEP * step, (err, step)
            assert abs(norm - wnorm) / wnorm < TOL_NORM
            assert _count_ok(count, wcount), (count, wcount)
            assert float(np.abs(x - r["w"]).max()) > 0
    finally:
        v.close()


def test_after_two_updates_every_weight_image_follows(pkg, orc):
    """two large Adam steps move every weight; the frozen forward then equals the float64 forward on get_weights() (the images
    the forward reads were updated) and a fresh gradient check passes (W' of d(input) was rebuilt)"""
    c, r = vt.CASES["narrow"], _reference(orc, "narrow")
    dr = _dropout(pkg, c)
    v = _body(pkg, orc, c)
    try:
        for _ in range(2):
            v.train_forward_raw(r["img"], c["xoff"], c["yoff"], dropout=dr, want_feats=False)
            v.backward(r["dfeats"])
            v.update(vt.ADAM, 0.5, 0.9, 0.999, 1e-8, 0.0, 0.0, SCALE, want_stats=False)
        w = v.get_weights()
        moved = np.abs(w - r["w"])
        assert float(moved.max()) > 4e-3 and float((moved > 0).mean()) > 0.1  # Adam's first step alone is lr x scale = 5e-3
        got = v.fc7_raw(r["img"], c["xoff"], c["yoff"], dropout=dr)
        want, _, _, _ = vt.free_forward(c["div"], c["hw"], w, r["x"], c["dr"])
        assert _relmax(r["feats"], want.numpy()) > 1e-2  # the features moved far beyond the tolerance
        assert _relmax(got, want.numpy()) < TOL_ACT
        feats = v.train_forward_raw(r["img"], c["xoff"], c["yoff"], dropout=dr)
        assert np.array_equal(feats, got)
        acts = [v.train_activation(i) for i in range(15)]
        v.backward(r["dfeats"])
        _check_grads(c, dict(r, w=w), vt.pattern_of(acts, c["dr"]), v.get_grads(), False, "after updates")
    finally:
        v.close()


def test_refusals_leave_the_extractor_usable(pkg, orc):
    b = pkg.binding
    c, r = vt.CASES["narrow"], _reference(orc, "narrow")
    img, n = r["img"], c["n"]
    v = _body(pkg, orc, c, train=False)
    try:
        want = v.fc7_raw(img, c["xoff"], c["yoff"])
        for call in (lambda: v.train_forward_raw(img, c["xoff"], c["yoff"]), lambda: v.backward(r["dfeats"]), v.get_grads,
                     lambda: v.update(vt.SGD, LR), lambda: v.train_activation(0)):
            with pytest.raises(b.NvqaError):       # training not enabled
                call()
        v.set_precision(1)
        with pytest.raises(b.NvqaError, match="bf16"):
            v.train_enable(True)                    # a bf16 extractor does not train
        v.set_precision(0)
        v.train_enable(True)
        with pytest.raises(b.NvqaError, match="bf16"):
            v.set_precision(1)                      # nor does a training one turn bf16
        with pytest.raises(b.NvqaError, match="training forward"):
            v.backward(r["dfeats"])                 # no training forward yet
        with pytest.raises(b.NvqaError):
            v.get_grads()                           # no backward yet
        with pytest.raises(b.NvqaError):
            v.train_forward_raw(vref.raw_images(n + 2, c["S"], 1), 0, 0)  # n > max_batch
        assert np.array_equal(v.train_forward_raw(img, c["xoff"], c["yoff"]), want)
        with pytest.raises(b.NvqaError):
            v.backward(r["dfeats"][:n - 1])         # another n than the forward's
        with pytest.raises(b.NvqaError):
            v.backward(np.zeros((n + 2, v.feature_dim), np.float32))  # n > max_batch
        v.backward(r["dfeats"])
        g = v.get_grads()
        for rule in (2, 3, 4, -1, 6):               # not one of -cnn_optim's
            with pytest.raises(b.NvqaError, match="rule"):
                v.update(rule, LR)
        assert np.array_equal(v.get_weights(), r["w"]) and np.array_equal(v.get_grads(), g)
        v.train_enable(False)
        with pytest.raises(b.NvqaError):
            v.backward(r["dfeats"])
        assert np.array_equal(v.fc7_raw(img, c["xoff"], c["yoff"]), want)
    finally:
        v.close()
