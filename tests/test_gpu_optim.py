"""nvqa_optim_update / nvqa_ae_wp_projection_update on the device: every rule of misc/optim_updates.lua against its NumPy
mirror (tests/optim_ref.py) with clamp and weight decay both acting, the old and the new entry points bit for bit on shared
state, per-segment gradient scales, the weak-paired contexts (frozen lookup, the projection's wd -> clamp order), the
refusals, and the trainers' -optim names.

Bounds: those of tests/test_gpu_ae.py's test_adam_update_matches_numpy_mirror -- max |x - mirror| < 1e-6 (x is O(0.1): one
f32 ulp of it is 7.5e-9, and a rule is a handful of f32 operations, fused or not), paramsNorm 1e-6 relative, the update count
within max(2, count // 1000) for |lr g| vs 0.01 |x| ties at f32 rounding.  Measured errors go to util.record.

One case misses 1e-6, adagrad at 4 234 271 values, in its first step: x moves by lr g / (|g| + eps), whose slope in g is
lr / eps = 2e6 where |g| <~ eps, and among 4 M values a few have the clamped gradient and the decay wd x cancel to |g| ~ 1e-8.
There the one rounding by which fma(wd, x, g) and round(wd x) + g differ (5e-11) moves x by 1e-5.  That is the float32
formula's own conditioning, so the bound for that case is twice the float32 mirror's distance from the float64 mirror on the same
inputs (never less than 1e-6).  Measured, first step: float32 mirror against float64 mirror 8.45e-6 (CPU, the float64 model's
gradient); device against float32 mirror 8.47e-6 (MI355X) -- the device's fused form sits within 1e-8 of the float64 mirror;
second and third step below 1e-6 on both counts."""
import zlib

import numpy as np
import pytest

import ae1wp_ref_torch as ref1wp
import ae2wp_ref_torch as ref2wp
import ae_ref_torch as ref
import optim_ref
from optim_ref import ADAGRAD, ADAM, RMSPROP, SGD, SGDM, SGDMOM
from util import record

pytestmark = pytest.mark.gpu

# the template's arguments: a large lr makes the update count non-trivial; the clamp (1e-3) and the weight decay (1e-2) both act
LR, ALPHA, BETA, EPS, WD, CLAMP = 2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3
ARGS = (LR, ALPHA, BETA, EPS, WD, CLAMP)
TOL_X, TOL_NORM = 1e-6, 1e-6

TINY = (4, 4, 11, 8, 8, 1)       # 1 356 values: whole float4s
TINY_TAIL = (4, 4, 10, 8, 8, 1)  # 1 339 values: 3 trailing elements, and the padding behind them
PASSES = (8, 4, 30, 512, 512, 1)  # 4 234 271 values: more than four grid-stride passes of 1024 x 256 float4s, 3 trailing


def _count_ok(count, want):
    return abs(count - want) <= max(2, want // 1000)


def _tokens(rng, B, D, V):
    lens = rng.integers(1, D + 1, B)
    lens[0] = D
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def _ae(pkg, dims, arch=3):
    return pkg.binding.Context(pkg.binding.Dims(arch, *dims, 0, 0, 0), 0)


def _inputs(dims, steps=3, seed=9):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"]).astype(np.float32)
    return p, [_tokens(rng, *dims[:3]) for _ in range(steps)]


def test_flat_lengths_of_the_three_shapes():
    assert [ref.layout(*d)["_total"] for d in (TINY, TINY_TAIL, PASSES)] == [1356, 1339, 4234271]
    assert 4234271 // 4 > 4 * 1024 * 256


MEASURED_BOUND = {(PASSES, ADAGRAD)}  # see the module docstring

MIRROR_CASES = [(d, r) for d in (TINY, TINY_TAIL) for r in range(6)] + [(PASSES, SGDMOM), (PASSES, ADAGRAD)]


@pytest.mark.parametrize("dims,rule", MIRROR_CASES,
                         ids=["%s-n%d" % (optim_ref.NAMES[r], ref.layout(*d)["_total"]) for d, r in MIRROR_CASES])
def test_rule_matches_numpy_mirror(pkg, dims, rule):
    p, toks = _inputs(dims)
    mirror = optim_ref.Optim(rule, p.size)
    mirror64 = optim_ref.Optim(rule, p.size, np.float64) if (dims, rule) in MEASURED_BOUND else None
    ctx = _ae(pkg, dims)
    try:
        assert ctx.param_count == p.size
        ctx.set_params(p)
        x = p.copy()
        for it, tok in enumerate(toks):
            ctx.ae_step(tok, None)
            g = ctx.get_grads()
            norm, count = ctx.optim_update(rule, *ARGS, stats=True)
            x_before = x
            x, wnorm, wcount = mirror.update(x, g, *ARGS)
            tol = TOL_X
            if mirror64 is not None:  # twice the float32 mirror's own distance from float64 on the same x and g
                tol = max(TOL_X, 2 * float(np.abs(mirror64.update(x_before, g, *ARGS)[0] - x.astype(np.float64)).max()))
            got = ctx.get_params()
            err = float(np.abs(got - x).max())
            record("optim_%s_n%d_step%d" % (optim_ref.NAMES[rule], p.size, it), {"max_abs": err, "tol": tol, "count": count, "count_ref": wcount})
            print(optim_ref.NAMES[rule], p.size, it, "max_abs", err, "tol", tol, "count", count, wcount, "norm", norm, wnorm)
            assert err < tol, (err, tol)
            assert abs(norm - wnorm) / wnorm < TOL_NORM
            assert _count_ok(count, wcount), (count, wcount)
            assert 0 < wcount < p.size  # the count is neither trivial bound
            x = got  # continue from the device's values
    finally:
        ctx.close()


def _run_entry_points(pkg, dims, p, toks, calls):
    """one context; calls[it](ctx) is the update of step it; returns the parameters and statistics after every step"""
    ctx = _ae(pkg, dims)
    out = []
    try:
        ctx.set_params(p)
        for it, tok in enumerate(toks):
            ctx.ae_step(tok, None)
            stats = calls[it](ctx)
            out.append((ctx.get_params(), stats))
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("dims", [TINY, TINY_TAIL], ids=["n1356", "n1339"])
def test_old_and_new_entry_points_give_the_same_bits(pkg, dims):
    p, toks = _inputs(dims, seed=10)

    def old_adam(c): return c.adam_update(*ARGS, stats=True)
    def new_adam(c): return c.optim_update(ADAM, *ARGS, stats=True)
    def old_rms(c): return c.rmsprop_update(LR, ALPHA, EPS, WD, CLAMP)
    def new_rms(c): return c.optim_update(RMSPROP, *ARGS)

    a = _run_entry_points(pkg, dims, p, toks, [old_adam] * 3)
    b = _run_entry_points(pkg, dims, p, toks, [new_adam] * 3)
    c = _run_entry_points(pkg, dims, p, toks, [old_adam, new_adam, old_adam])  # shared m / v / step counter
    for it in range(3):
        assert np.array_equal(a[it][0], b[it][0]) and np.array_equal(a[it][0], c[it][0]), ("adam", it)
        assert a[it][1] == b[it][1] == c[it][1], ("adam statistics", it)
    assert not np.array_equal(a[0][0], p)
    a = _run_entry_points(pkg, dims, p, toks, [old_rms] * 3)
    b = _run_entry_points(pkg, dims, p, toks, [new_rms] * 3)
    c = _run_entry_points(pkg, dims, p, toks, [new_rms, old_rms, new_rms])     # shared mean-square buffer
    for it in range(3):
        assert np.array_equal(a[it][0], b[it][0]) and np.array_equal(a[it][0], c[it][0]), ("rmsprop", it)
    assert not np.array_equal(a[0][0], p)


def test_state_is_per_rule_and_reset_by_init_params(pkg):
    """sgdm's velocity must not leak into sgdmom's buffer, and nvqa_init_params starts every rule afresh"""
    dims = TINY_TAIL
    p, toks = _inputs(dims, seed=12)
    ctx = _ae(pkg, dims)
    try:
        def first_update(rule):
            ctx.set_params(p)
            ctx.ae_step(toks[0], None)
            ctx.optim_update(rule, *ARGS)
            return ctx.get_params()
        fresh = {r: first_update(r) for r in (SGDM, SGDMOM, ADAGRAD)}  # each rule's first use: zero state
        ctx.init_params(1)
        for r in (SGDM, SGDMOM, ADAGRAD):
            assert np.array_equal(first_update(r), fresh[r]), optim_ref.NAMES[r]
        assert not np.array_equal(first_update(SGDM), fresh[SGDM])     # without a reset the velocity carries on
    finally:
        ctx.close()


@pytest.mark.parametrize("rule", [SGDM, ADAGRAD], ids=["sgdm", "adagrad"])
def test_segment_scales_on_a_vqa_context(pkg, orc, rule):
    d = orc.make_dims(arch=1, B=8, T=5, V=20, E=8, R=8, L=1, I=8, C=8, A=8)
    ctx = pkg.binding.Context(pkg.binding.Dims(*[getattr(d, n) for n, _ in d._fields_]), 0)
    scales = np.array([0.5, 0.25, 1.0], np.float32)
    try:
        params = orc.synth_params(d)
        tok, lens, img, lab = orc.synth_batch(d, full_length=False)
        seg = ctx.segments()
        s = np.repeat(scales, seg)
        ctx.set_params(params)
        mirror = optim_ref.Optim(rule, params.size)
        x = params.copy()
        for it in range(2):
            ctx.step(tok, lens, img, lab, None)
            g = ctx.get_grads()
            ctx.set_grad_scales(scales)
            norm, count = ctx.optim_update(rule, *ARGS, stats=True)
            ctx.set_grad_scales(np.ones(3, np.float32))  # get_grads above stays the unscaled gradient
            x, wnorm, wcount = mirror.update(x, g * s, *ARGS)
            got = ctx.get_params()
            err = float(np.abs(got - x).max())
            record("optim_seg_%s_step%d" % (optim_ref.NAMES[rule], it), {"max_abs": err})
            assert err < TOL_X, err
            assert abs(norm - wnorm) / wnorm < TOL_NORM
            assert _count_ok(count, wcount), (count, wcount)
            if it == 0 and rule == SGDM:  # the bound can tell: the mirror fed the unscaled gradient lies farther from the scaled one
                far, _, _ = optim_ref.Optim(rule, params.size).update(params, g, *ARGS)
                assert float(np.abs(x - far).max()) > TOL_X
            x = got
    finally:
        ctx.close()


WP2 = (6, 5, 21, 8, 12, 1, 16)   # B, D, V, E, R, L, I
WP1 = (6, 5, 21, 8, 12, 16)      # B, D, V, E, R, I


def _feats(rng, B, I):
    f = rng.uniform(0, 1, (B, I)).astype(np.float32)
    f[rng.uniform(0, 1, (B, I)) < 0.3] = 0.0
    return f


def _wp2(pkg, seed_name):
    B, D, V, E, R, L, I = WP2
    b = pkg.binding
    rng = np.random.default_rng(zlib.crc32(seed_name.encode()))
    lo = ref2wp.layout(B, D, V, E, R, L)
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    w = rng.uniform(-0.08, 0.08, (E, I)).astype(np.float32)
    bb = rng.uniform(-0.05, 0.05, E).astype(np.float32)
    ctx = b.Context(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), 0)
    ctx.set_params(p)
    ctx.ae_wp_set_projection(w, bb)
    return ctx, lo, p, w, bb, _feats(rng, B, I), _tokens(rng, B, D, V)


@pytest.mark.parametrize("rule", [RMSPROP, ADAGRAD], ids=["rmsprop", "adagrad"])
def test_ae2wp_update_leaves_the_frozen_lookup_alone(pkg, rule):
    ctx, lo, p, _, _, f, tok = _wp2(pkg, "optim_frozen")
    n = lo["_seg0"] + lo["_seg1"]
    mirror = optim_ref.Optim(rule, n)
    try:
        x = p.copy()
        for it in range(2):
            ctx.ae_wp_step(f, tok, enc_tokens=tok)
            g = ctx.get_grads()
            norm, count = ctx.optim_update(rule, *ARGS, stats=True)
            want, wnorm, wcount = mirror.update(x[:n], g[:n], *ARGS)   # the statistics: [encoder | decoder] only
            got = ctx.get_params()
            assert np.array_equal(got[n:], p[n:]), "W_lk moved"
            assert float(np.abs(got[:n] - want).max()) < TOL_X
            assert abs(norm - wnorm) / wnorm < TOL_NORM
            assert _count_ok(count, wcount), (count, wcount)
            x = got
    finally:
        ctx.close()


@pytest.mark.parametrize("rule", [RMSPROP, ADAGRAD], ids=["rmsprop", "adagrad"])
def test_ae1wp_update_runs_over_the_whole_vector(pkg, rule):
    B, D, V, E, R, I = WP1
    b = pkg.binding
    rng = np.random.default_rng(31)
    lo = ref1wp.layout(D, V, E, R, I)
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    wlk = rng.uniform(-1.0, 1.0, (V + 1, E)).astype(np.float32)
    f, tok = _feats(rng, B, I), _tokens(rng, B, D, V)
    mirror = optim_ref.Optim(rule, p.size)
    ctx = b.Context(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, 2 * R, 0), 0)
    try:
        ctx.set_params(p)
        ctx.ae1_wp_set_lookup(wlk)
        x = p.copy()
        for it in range(2):
            ctx.ae1_wp_step(f, tok, enc_tokens=tok)
            g = ctx.get_grads()
            norm, count = ctx.optim_update(rule, *ARGS, stats=True)
            want, wnorm, wcount = mirror.update(x, g, *ARGS)
            got = ctx.get_params()
            assert float(np.abs(got - want).max()) < TOL_X
            assert abs(norm - wnorm) / wnorm < TOL_NORM
            assert _count_ok(count, wcount), (count, wcount)
            x = got
        assert np.array_equal(ctx.ae1_wp_get_lookup(), wlk), "W_lk moved"
    finally:
        ctx.close()


@pytest.mark.parametrize("rule", [SGD, SGDM], ids=["sgd", "sgdm"])
def test_projection_update_matches_mirror_with_decay_then_clamp(pkg, rule):
    B, D, V, E, R, L, I = WP2
    ctx, _, _, w, bb, f, tok = _wp2(pkg, "optim_proj")
    lr, wd, clamp = 1e-2, 0.5, 2e-3   # test_projection_adam_matches_numpy_with_decay_then_clamp's: the clamp bites after the decay
    mirror = optim_ref.Optim(rule, E * I + E, wd_first=True)
    try:
        x = np.concatenate([w.ravel(), bb])
        for it in range(3):
            ctx.ae_wp_step(f, tok, enc_tokens=tok)
            gw, gb = ctx.ae_wp_get_projection_grads()
            norm, count = ctx.ae_wp_projection_update(rule, lr, ALPHA, BETA, EPS, wd, clamp, stats=True)
            want, _, wcount = mirror.update(x, np.concatenate([gw.ravel(), gb]), lr, ALPHA, BETA, EPS, wd, clamp)
            wnorm = float(np.sqrt((x[:E * I].astype(np.float64) ** 2).sum()))   # the weight only
            w2, b2 = ctx.ae_wp_get_projection()
            got = np.concatenate([w2.ravel(), b2])
            assert float(np.abs(got - want).max()) < TOL_X
            assert abs(norm - wnorm) / wnorm < TOL_NORM
            assert _count_ok(count, wcount), (count, wcount)
            x = got
    finally:
        ctx.close()


def test_projection_adam_rule_equals_projection_adam_bitwise(pkg):
    out = []
    for new in (False, True, None):   # None: the two entry points alternate on one context
        ctx, _, _, _, _, f, tok = _wp2(pkg, "optim_proj_adam")
        try:
            for it in range(3):
                ctx.ae_wp_step(f, tok, enc_tokens=tok)
                use_new = (it % 2 == 1) if new is None else new
                if use_new:
                    stats = ctx.ae_wp_projection_update(ADAM, 1e-2, ALPHA, BETA, EPS, 0.5, 2e-3, stats=True)
                else:
                    stats = ctx.ae_wp_projection_adam(1e-2, ALPHA, BETA, EPS, 0.5, 2e-3, stats=True)
                out.append((new, it, np.concatenate([a.ravel() for a in ctx.ae_wp_get_projection()]), stats))
        finally:
            ctx.close()
    for it in range(3):
        a, b, c = out[it], out[3 + it], out[6 + it]
        assert np.array_equal(a[2], b[2]) and np.array_equal(a[2], c[2]), it
        assert a[3] == b[3] == c[3], it


def test_refusals(pkg):
    E = pkg.binding.NvqaError
    b = pkg.binding
    tok = np.array([[1, 2, 0, 0]] * 4, np.int32)
    ctx = _ae(pkg, TINY)
    try:
        ctx.init_params(1)
        with pytest.raises(E, match="before any step"):
            ctx.optim_update(SGD, 1e-3)
        ctx.ae_step(tok, None)
        for bad in (-1, 6, 99):
            with pytest.raises(E, match="unknown rule"):
                ctx.optim_update(bad, 1e-3)
        with pytest.raises(E, match="nvqa_ae_wp_projection_update"):   # not a weak-paired context
            ctx.ae_wp_projection_update(SGD, 1e-3)
        x = ctx.get_params()
        ctx.optim_update(SGD, 1e-3)   # and the context still works
        assert not np.array_equal(ctx.get_params(), x)
    finally:
        ctx.close()
    wp1 = b.Context(b.Dims(b.ARCH_AE1_WP, 4, 4, 9, 8, 8, 1, 8, 16, 0), 0)
    try:
        with pytest.raises(E, match="nvqa_ae_wp_projection_update"):
            wp1.ae_wp_projection_update(SGD, 1e-3)
    finally:
        wp1.close()
    ctx, _, _, _, _, f, tok5 = _wp2(pkg, "optim_refusals")
    try:
        with pytest.raises(E, match="before any"):
            ctx.ae_wp_projection_update(SGDM, 1e-3)
        ctx.ae_wp_step(f, tok5, enc_tokens=tok5)
        for bad in (SGDMOM, ADAGRAD, RMSPROP, -1, 6):
            with pytest.raises(E, match="cnn_optim"):
                ctx.ae_wp_projection_update(bad, 1e-3)
        with pytest.raises(E, match="weak-paired"):   # the old call keeps its refusal; the rule runs
            ctx.rmsprop_update(1e-3)
        ctx.optim_update(RMSPROP, 1e-3)
    finally:
        ctx.close()


@pytest.mark.parametrize("optim", ["sgd", "sgdm", "sgdmom", "adagrad"])
def test_trainer_runs_the_new_rules(pkg, optim):
    import re
    b = pkg.binding
    B, D, V, E, R, L = TINY
    rng = np.random.default_rng(4)
    labels = np.concatenate([_tokens(rng, B, D, V) for _ in range(3)])
    lines = []
    for decay_start in (-1, 0):
        tr = pkg.ae.AETrainer(b.Dims(b.ARCH_AE1, B, D, V, E, R, L, 0, 0, 0), learning_rate=1e-2, optim=optim,
                              learning_rate_decay_start=decay_start, learning_rate_decay_every=1, drop_prob=0.0)
        try:
            out = []
            losses = tr.train(pkg.ae.DataLoader(labels={"train": labels}), 3, log=out.append)
            x = tr.ctx.get_params()
        finally:
            tr.ctx.close()
        assert len(losses) == 3 and np.all(np.isfinite(losses)) and np.all(np.isfinite(x))
        for it, line in enumerate(out, start=1):
            assert re.fullmatch(r"iter %d: loss: \d+\.\d{3} \| # updates: +\d+ \| paramsNorm: \d+\.\d{4}" % it, line), line
        lines.append((out, x))
    same = lines[0][0] == lines[1][0] and np.array_equal(lines[0][1], lines[1][1])
    assert same == (optim == "sgd"), "sgd alone takes the undecayed learning rate"


def test_trainers_reject_unknown_names(pkg):
    b = pkg.binding
    with pytest.raises(ValueError, match="optim"):
        pkg.ae.AETrainer(b.Dims(b.ARCH_AE1, *TINY, 0, 0, 0), optim="lbfgs")
    with pytest.raises(ValueError, match="cnn_optim"):
        pkg.ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2_WP, *WP2[:6], WP2[6], 0, 0), cnn_optim="rmsprop")


def _wp_loader(pkg, B, D, V, I, seed):
    rng = np.random.default_rng(seed)
    labels = np.concatenate([_tokens(rng, B, D, V) for _ in range(3)])
    return pkg.ae.WeakPairedDataLoader(labels={"train": labels}, feats={"train": _feats(rng, 3 * B, I)})


@pytest.mark.parametrize("cnn_optim", ["sgd", "sgdm"])
def test_weak_paired_trainer_runs_optim_and_cnn_optim(pkg, cnn_optim):
    """WeakPairedAETrainer(optim='sgd', cnn_optim=...) with the projection fine-tuned from the first iteration; the cnn rule
    takes the decayed cnn rate (sgd included, as in the script), so a decay changes the projection"""
    import re
    b = pkg.binding
    B, D, V, E, R, L, I = WP2
    runs = []
    for decay_start in (-1, 0):
        tr = pkg.ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), learning_rate=1e-2, optim="sgd",
                                        cnn_optim=cnn_optim, cnn_learning_rate=1e-2, cnn_weight_decay=1e-3, finetune_cnn_after=0,
                                        learning_rate_decay_start=decay_start, learning_rate_decay_every=1, drop_prob=0.0)
        try:
            w0 = np.concatenate([a.ravel() for a in tr.ctx.ae_wp_get_projection()])
            out = []
            losses = tr.train(_wp_loader(pkg, B, D, V, I, 6), 3, log=out.append)
            x = tr.ctx.get_params()
            w = np.concatenate([a.ravel() for a in tr.ctx.ae_wp_get_projection()])
        finally:
            tr.ctx.close()
        assert np.all(np.isfinite(losses)) and np.all(np.isfinite(x)) and np.all(np.isfinite(w))
        assert not np.array_equal(w, w0), "the projection was not updated"
        for it, line in enumerate(out, start=1):
            assert re.fullmatch(r"iter %d: loss: \d+\.\d{3} \| # updates: +\d+ \| paramsNorm: \d+\.\d{4} \| # cnn updates: +\d+ "
                                r"\| cnnParamsNorm: \d+\.\d{4}" % it, line), line
        runs.append((x, w))
    assert not np.array_equal(runs[0][1], runs[1][1]), "the cnn rule ignores the decayed rate"


@pytest.mark.parametrize("optim", ["sgd", "rmsprop"])
def test_weak_paired_arch1_trainer_runs_optim(pkg, optim):
    import re
    b = pkg.binding
    B, D, V, E, R, I = WP1
    runs = []
    for decay_start in (-1, 0):
        tr = pkg.ae.WeakPairedAE1Trainer(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, 2 * R, 0), learning_rate=1e-2, optim=optim,
                                         skip_prob=0.0, learning_rate_decay_start=decay_start, learning_rate_decay_every=1,
                                         drop_prob=0.0)
        try:
            out = []
            losses = tr.train(_wp_loader(pkg, B, D, V, I, 7), 3, log=out.append)
            x = tr.ctx.get_params()
        finally:
            tr.ctx.close()
        assert np.all(np.isfinite(losses)) and np.all(np.isfinite(x))
        for it, line in enumerate(out, start=1):
            assert re.fullmatch(r"iter %d: loss: \d+\.\d{3} \| # updates: +\d+ \| paramsNorm: \d+\.\d{4}" % it, line), line
        runs.append((out, x))
    same = runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1])
    assert same == (optim == "sgd"), "sgd alone takes the undecayed learning rate"
