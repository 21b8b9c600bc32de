"""The weak-paired steps that hand d(loss)/d(f^) to a fine-tuning VGG-16 body, at the shapes of
tests/test_gpu_ae_wp_images.py with its (16, 32) body: nvqa_ae_wp_step_dfeats against autograd on tests/ae2wp_ref_torch.py at
tests/test_gpu_ae2wp.py's tolerance, with loss and gradients bit-equal to nvqa_ae_wp_step; both *_finetune steps bit-equal to
the composed route (training forward, the host-fed step with dfeats_out, nvqa_vgg16_backward(..., 1)) in loss, auto-encoder
gradients, projection gradients and body gradients, for both encoder modes with the dropouts live; two fine-tuning steps back to
back without a synchronisation; the refusal of an extractor that is not training-enabled.  The body's backward itself is held to
the float64 model in tests/test_gpu_vgg_train.py, so equality with the composed route is the whole claim here."""
import numpy as np
import pytest

import ae2wp_ref_torch as ref2
import vgg_body_ref as vref
from test_gpu_ae_wp_images import S, WP1, WP2, _body, _ctx1, _ctx2, _tokens
from test_gpu_ae2wp import TOL_GRAD, rel_err

pytestmark = pytest.mark.gpu


def _train_body(pkg, orc):
    v = _body(pkg, orc)
    v.train_enable(True)
    return v


@pytest.mark.parametrize("enc", ["same", "null"])
def test_ae2wp_step_dfeats_matches_autograd_and_keeps_the_step(pkg, enc):
    b = pkg.binding
    B, D, V, E, R, L, I = WP2
    ctx, rng = _ctx2(pkg, "ft_dfeats_" + enc)
    try:
        tok = _tokens(rng, B, D, V)
        et = None if enc == "null" else tok
        feats = np.abs(rng.standard_normal((B, I))).astype(np.float32)
        dr = b.Dropout(1, 0.5, 78, 3)
        want = (ctx.ae_wp_step(feats, tok, enc_tokens=et, dropout=dr), ctx.get_grads(), *ctx.ae_wp_get_projection_grads())
        loss, df = ctx.ae_wp_step(feats, tok, enc_tokens=et, dropout=dr, want_dfeats=True)
        got = (loss, ctx.get_grads(), *ctx.ae_wp_get_projection_grads())
        p, (w, bb) = ctx.get_params(), ctx.ae_wp_get_projection()
    finally:
        ctx.close()
    assert got[0] == want[0]
    for g, x in zip(got[1:], want[1:]):
        assert np.array_equal(g, x)
    model = ref2.forward(WP2, p.astype(np.float64), w, bb, feats, tok, enc_tokens=et, dr=dr)
    want_df = model["dx0"] @ np.asarray(w, np.float64).reshape(E, I)  # x0 = f^ W_p^T + b_p
    err = rel_err(df, want_df)
    print("d f^ rel err", enc, err)
    assert np.abs(want_df).max() > 0 and err < TOL_GRAD, err


CASES2 = [("same", "same"), ("null_sentence", "null")]
CASES1 = [("encoder", "same"), ("encoder_skip", "skip")]


@pytest.mark.parametrize("name,enc", CASES2, ids=[c[0] for c in CASES2])
def test_ae2wp_finetune_step_equals_composed_route(pkg, orc, name, enc):
    b = pkg.binding
    B, D, V, E, R, L, I = WP2
    ctx, rng = _ctx2(pkg, "ft2_" + name)
    v = _train_body(pkg, orc)
    try:
        tok, img = _tokens(rng, B, D, V), vref.raw_images(B, S, 61)
        et = None if enc == "null" else tok
        bdr, dr = b.Dropout(1, 0.5, 77, 3), b.Dropout(1, 0.5, 78, 3)
        feats = v.train_forward_raw(img, 7, 3, dropout=bdr)
        wl, df = ctx.ae_wp_step(feats, tok, enc_tokens=et, dropout=dr, want_dfeats=True)
        v.backward(df, through_l2norm=True)
        want = (wl, ctx.get_grads(), *ctx.ae_wp_get_projection_grads(), v.get_grads())
        frozen = ctx.ae_wp_step_images(v, img, 7, 3, tok, enc_tokens=et, body_dropout=bdr, dropout=dr)
        v.backward(np.zeros_like(df))  # wipe the body's gradients: the fused step must rebuild them
        assert not np.any(v.get_grads()[:100])
        gl = ctx.ae_wp_step_images(v, img, 7, 3, tok, enc_tokens=et, body_dropout=bdr, dropout=dr, finetune=True)
        got = (gl, ctx.get_grads(), *ctx.ae_wp_get_projection_grads(), v.get_grads())
        assert np.array_equal(v.train_activation(14), feats)
    finally:
        ctx.close()
        v.close()
    assert np.isfinite(wl) and frozen == wl and all(np.any(x) for x in want[1:])
    assert got[0] == want[0]
    for g, x in zip(got[1:], want[1:]):
        assert np.array_equal(g, x), float(np.abs(g - x).max())


@pytest.mark.parametrize("name,enc", CASES1, ids=[c[0] for c in CASES1])
def test_ae1wp_finetune_step_equals_composed_route(pkg, orc, name, enc):
    b = pkg.binding
    B, D, V, E, R, L, I = WP1
    ctx, rng = _ctx1(pkg, "ft1_" + name)
    v = _train_body(pkg, orc)
    try:
        tok, img = _tokens(rng, B, D, V), vref.raw_images(B, S, 62)
        kw = {"enc_state": rng.uniform(-0.5, 0.5, (B, 2 * R)).astype(np.float32)} if enc == "skip" else {"enc_tokens": tok}
        bdr, dr = b.Dropout(1, 0.5, 77, 3), b.Dropout(1, 0.5, 78, 3)
        feats = v.train_forward_raw(img, 8, 8, dropout=bdr)
        wl, wdf = ctx.ae1_wp_step(feats, tok, dropout=dr, want_dfeats=True, **kw)
        v.backward(wdf, through_l2norm=True)
        want = (ctx.get_grads(), wdf, v.get_grads())
        v.backward(np.zeros_like(wdf))
        gl, gdf = ctx.ae1_wp_step_images(v, img, 8, 8, tok, body_dropout=bdr, dropout=dr, want_dfeats=True, finetune=True, **kw)
        got = (ctx.get_grads(), gdf, v.get_grads())
        v.backward(np.zeros_like(wdf))
        gl2 = ctx.ae1_wp_step_images(v, img, 8, 8, tok, body_dropout=bdr, dropout=dr, finetune=True, **kw)  # without dfeats_out
        got2 = v.get_grads()
    finally:
        ctx.close()
        v.close()
    assert np.isfinite(wl) and all(np.any(x) for x in want)
    assert gl == wl and gl2 == wl
    for g, x in zip(got, want):
        assert np.array_equal(g, x), float(np.abs(g - x).max())
    assert np.array_equal(got2, want[2])


def test_two_finetune_steps_back_to_back_without_a_sync(pkg, orc):
    """step k + 1's training forward overwrites the saved activations and the context's next backward overwrites d f^: both
    are ordered by the streams' events alone (want_loss=False: no call waits for a kernel)"""
    b = pkg.binding
    B, D, V, E, R, L, I = WP2
    bdr, dr = b.Dropout(1, 0.5, 77, 3), b.Dropout(1, 0.5, 78, 3)
    out = []
    for sync in (True, False):
        ctx, rng = _ctx2(pkg, "ft_b2b")
        v = _train_body(pkg, orc)
        try:
            tok = [_tokens(rng, B, D, V) for _ in range(2)]
            img = [vref.raw_images(B, S, 63 + k) for k in range(2)]
            for k in range(2):
                loss = ctx.ae_wp_step_images(v, img[k], 7 - k, 3 + k, tok[k], enc_tokens=tok[k], body_dropout=bdr, dropout=dr,
                                             want_loss=sync, finetune=True)
                assert (loss is not None) == sync
                if k == 0:
                    v.update(b.OPT_ADAM, 0.5, 0.9, 0.999, 1e-8, 0.0, 0.0, 0.01, want_stats=sync)
            out.append((ctx.get_grads(), ctx.ae_wp_get_projection_grads()[0], v.get_grads(), v.get_weights()))
        finally:
            ctx.close()
            v.close()
    for a, c in zip(*out):
        assert np.any(a) and np.array_equal(a, c)


def test_finetune_refuses_an_extractor_that_does_not_train(pkg, orc):
    b = pkg.binding
    B, D, V, E, R, L, I = WP2
    ctx, rng = _ctx2(pkg, "ft_refuse")
    v = _body(pkg, orc)
    try:
        tok, img = _tokens(rng, B, D, V), vref.raw_images(B, S, 65)
        with pytest.raises(b.NvqaError, match="train_enable"):
            ctx.ae_wp_step_images(v, img, 7, 3, tok, enc_tokens=tok, finetune=True)
        want = ctx.ae_wp_step_images(v, img, 7, 3, tok, enc_tokens=tok)
        v.train_enable(True)
        assert ctx.ae_wp_step_images(v, img, 7, 3, tok, enc_tokens=tok, finetune=True) == want
        assert np.any(v.get_grads())
    finally:
        ctx.close()
        v.close()


def _loader(pkg, dims, seed):
    B, D, V = dims[:3]
    rng = np.random.default_rng(seed)
    labels = {"train": _tokens(rng, B, D, V)}
    images = {"train": vref.raw_images(B, S, seed + 1)}
    return pkg.ae.WeakPairedImageLoader(labels, images, ix_to_word={str(i): "w%d" % i for i in range(1, V + 1)})


def _run_trainer(pkg, orc, make, dims, seed, **kw):
    """three iterations on one batch; per iteration (train_step's tuple, the context's parameters, the body's weights)"""
    v = _body(pkg, orc)
    tr = make(body=v, **kw)
    loader = _loader(pkg, dims, seed)
    out = []
    try:
        for _ in range(3):
            labels, images, _ = loader.get_batch("train", dims[0])
            step = tr.train_step_images(labels, images)
            out.append((step, tr.ctx.get_params(), v.get_weights()))
    finally:
        tr.ctx.close()
        v.close()
    return out


def _check_trainer_runs(frozen, tuned, w0):
    # finetune_body=False: the body never moves
    assert all(np.array_equal(w, w0) for _, _, w in frozen)
    # iteration 1 (before finetune_cnn_after = 2): the same numbers, the body bit-unchanged
    assert tuned[0][0][0] == frozen[0][0][0] and np.array_equal(tuned[0][1], frozen[0][1]) and np.array_equal(tuned[0][2], w0)
    # iteration 2: the same forward and auto-encoder update (the body's update comes last), and the body has moved
    assert tuned[1][0][0] == frozen[1][0][0] and np.array_equal(tuned[1][1], frozen[1][1])
    assert not np.array_equal(tuned[1][2], w0) and float(np.abs(tuned[1][2] - w0).max()) > 1e-4
    # iteration 3 runs on the moved body
    assert tuned[2][0][0] != frozen[2][0][0] and not np.array_equal(tuned[2][2], tuned[1][2])


def test_arch2_trainer_finetunes_the_body_from_finetune_cnn_after(pkg, orc):
    b, ae = pkg.binding, pkg.ae
    B, D, V, E, R, L, I = WP2
    w0 = np.asarray(orc.VggOracle(16, 32).synth_weights(), np.float32)

    def make(**kw):
        return ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), learning_rate=1e-2, finetune_cnn_after=2,
                                      cnn_learning_rate=1e-1, cnn_weight_decay=1e-3, cnn_optim="adam", **kw)  # Adam's first step: lr x scale = 1e-3
    frozen = _run_trainer(pkg, orc, make, WP2, 91)                     # today's trainer: the projection alone fine-tunes
    same = _run_trainer(pkg, orc, make, WP2, 91, finetune_body=False)
    tuned = _run_trainer(pkg, orc, make, WP2, 91, finetune_body=True)
    for (s0, p0, _), (s1, p1, _) in zip(frozen, same):
        assert s0 == s1 and np.array_equal(p0, p1)
    _check_trainer_runs(frozen, tuned, w0)
    for k in range(2):  # every figure of the log line, the cnn ones included, stays the projection's (:353-354)
        assert tuned[k][0] == frozen[k][0]
    import re
    assert re.fullmatch(r"iter 3: loss: \d+\.\d{3} \| # updates: +\d+ \| paramsNorm: \d+\.\d{4} \| # cnn updates: +\d+ \| cnnParamsNorm: \d+\.\d{4}",
                        tuned[2][0][-1])
    with pytest.raises(ValueError, match="body"):
        ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), finetune_body=True)


def test_arch1_trainer_finetunes_the_body_from_finetune_cnn_after(pkg, orc):
    b, ae = pkg.binding, pkg.ae
    B, D, V, E, R, L, I = WP1
    w0 = np.asarray(orc.VggOracle(16, 32).synth_weights(), np.float32)
    mean = np.random.default_rng(7).uniform(-0.5, 0.5, 2 * R).astype(np.float32)

    def make(**kw):
        tr = ae.WeakPairedAE1Trainer(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, 2 * R, 0), learning_rate=1e-2, **kw)
        tr.set_mean_vector(mean)
        return tr
    cnn = dict(finetune_cnn_after=2, cnn_learning_rate=1e-3, cnn_weight_decay=1e-3, cnn_optim="adam")
    frozen = _run_trainer(pkg, orc, make, WP1, 93)                     # today's trainer
    same = _run_trainer(pkg, orc, make, WP1, 93, finetune_body=False, **cnn)  # the cnn options are not read
    tuned = _run_trainer(pkg, orc, make, WP1, 93, finetune_body=True, **cnn)
    for (s0, p0, _), (s1, p1, _) in zip(frozen, same):
        assert s0 == s1 and np.array_equal(p0, p1) and len(s0) == 5
    _check_trainer_runs(frozen, tuned, w0)
    import re
    for k in range(3):  # the script's fields, the cnn figures from the body (:374-375)
        step = tuned[k][0]
        assert len(step) == 7 and step[-1].startswith(frozen[k][0][-1] if k < 2 else "iter 3: ")
        assert re.fullmatch(r"iter \d: loss: \d+\.\d{3} \| # updates: +\d+ \| paramsNorm: \d+\.\d{4} \| # cnn updates: +\d+ \| cnnParamsNorm: \d+\.\d{4}",
                            step[-1])
        want_norm = float(np.sqrt((w0.astype(np.float64) ** 2).sum())) if k < 2 else float(np.sqrt((tuned[1][2].astype(np.float64) ** 2).sum()))
        assert abs(step[5] - want_norm) < 1e-5 * want_norm  # cnnParamsNorm is the body's, before the update
    assert tuned[0][0][4] == int((w0 == 0).sum())
