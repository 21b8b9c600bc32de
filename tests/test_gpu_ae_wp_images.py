"""The weak-paired steps with the VGG-16 body in the loop (nvqa_ae_wp_step_images and its three siblings): bit-equal to the
host-fed step given nvqa_vgg16_fc7_raw's features -- the composed route, which test_gpu_ae2wp.py / test_gpu_ae1wp.py hold to
the float64 models, so equality is the whole claim --, the buffer-reuse edge between two un-synchronised steps, the refusals,
and the trainer on a WeakPairedImageLoader."""
import functools
import zlib

import numpy as np
import pytest

import ae1wp_ref_torch as ref1
import vgg_body_ref as vref

pytestmark = pytest.mark.gpu

DIV, HW, S = 16, 32, 40                     # body: F = 256
WP2 = (5, 5, 17, 12, 8, 1, 256)             # (B, D, V, E, R, L, I)
WP1 = (6, 5, 23, 8, 12, 1, 256)             # (B, D, V, E, R, L, I), C = 2R = 24


@functools.lru_cache(maxsize=None)
def _weights(orc):
    return orc.VggOracle(DIV, HW).synth_weights()


def _body(pkg, orc, max_batch=6, div=DIV):
    v = pkg.binding.Vgg16(0, div, HW, max_batch=max_batch)
    v.set_weights(_weights(orc) if div == DIV else orc.VggOracle(div, HW).synth_weights())
    return v


def _tokens(rng, B, D, V):
    lens = rng.integers(1, D + 1, B)
    lens[0] = D
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def _ctx2(pkg, name, dims=WP2):
    b = pkg.binding
    B, D, V, E, R, L, I = dims
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ctx = b.Context(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), 0)
    ctx.set_params(rng.uniform(-0.08, 0.08, ctx.param_count).astype(np.float32))
    ctx.ae_wp_set_projection(rng.uniform(-0.08, 0.08, (E, I)).astype(np.float32), rng.uniform(-0.05, 0.05, E).astype(np.float32))
    return ctx, rng


def _ctx1(pkg, name, dims=WP1):
    b = pkg.binding
    B, D, V, E, R, L, I = dims
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    ctx = b.Context(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, 2 * R, 0), 0)
    lo = ref1.layout(D, V, E, R, I)
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    for w, fan_in in (("w_q", 2 * R), ("b_q", 2 * R), ("w_v", I), ("b_v", I)):  # the bridge as the trainer draws it
        o, n = lo[w]
        p[o:o + n] = rng.uniform(-1, 1, n) / np.sqrt(fan_in)
    ctx.set_params(p)
    ctx.ae1_wp_set_lookup(rng.uniform(-1.0, 1.0, (V + 1, E)).astype(np.float32))
    return ctx, rng


# name, body dropout, LSTM dropout, encoder input
CASES2 = [("plain", False, False, "same"), ("both_dropouts", True, True, "same"), ("null_sentence", True, False, "null")]
CASES1 = [("plain", False, False, "same"), ("both_dropouts", True, True, "same"), ("encoder_skip", True, True, "skip")]


@pytest.mark.parametrize("name,bdrop,drop,enc", CASES2, ids=[c[0] for c in CASES2])
def test_ae2wp_step_images_equals_composed_route(pkg, orc, name, bdrop, drop, enc):
    b = pkg.binding
    B, D, V, E, R, L, I = WP2
    ctx, rng = _ctx2(pkg, "wp2_" + name)
    v = _body(pkg, orc)
    try:
        tok, img = _tokens(rng, B, D, V), vref.raw_images(B, S, 51)
        et = None if enc == "null" else tok
        bdr = b.Dropout(1, 0.5, 77, 3) if bdrop else None
        dr = b.Dropout(1, 0.5, 78, 3) if drop else None
        feats = v.fc7_raw(img, 7, 3, dropout=bdr)
        want = (ctx.ae_wp_step(feats, tok, enc_tokens=et, dropout=dr), ctx.get_grads(), *ctx.ae_wp_get_projection_grads())
        got = (ctx.ae_wp_step_images(v, img, 7, 3, tok, enc_tokens=et, body_dropout=bdr, dropout=dr), ctx.get_grads(),
               *ctx.ae_wp_get_projection_grads())
        # the window reaches the body: another origin gives other features, seen in dW_p = dx0^T f^ (the f32 loss cannot
        # resolve it: the features enter through one projected row of the encoder's input)
        ctx.ae_wp_step_images(v, img, 3, 7, tok, enc_tokens=et, body_dropout=bdr, dropout=dr)
        other = ctx.ae_wp_get_projection_grads()[0]
    finally:
        ctx.close()
        v.close()
    assert np.isfinite(want[0]) and np.any(want[1]) and np.any(want[2])
    assert got[0] == want[0], (got[0], want[0])
    for g, w in zip(got[1:], want[1:]):
        assert np.array_equal(g, w), float(np.abs(g - w).max())
    assert not np.array_equal(other, want[2])


@pytest.mark.parametrize("name,bdrop,drop,enc", CASES1, ids=[c[0] for c in CASES1])
def test_ae1wp_step_images_equals_composed_route(pkg, orc, name, bdrop, drop, enc):
    b = pkg.binding
    B, D, V, E, R, L, I = WP1
    ctx, rng = _ctx1(pkg, "wp1_" + name)
    v = _body(pkg, orc)
    try:
        tok, img = _tokens(rng, B, D, V), vref.raw_images(B, S, 52)
        kw = {"enc_state": rng.uniform(-0.5, 0.5, (B, 2 * R)).astype(np.float32)} if enc == "skip" else {"enc_tokens": tok}
        bdr = b.Dropout(1, 0.5, 77, 3) if bdrop else None
        dr = b.Dropout(1, 0.5, 78, 3) if drop else None
        feats = v.fc7_raw(img, 8, 8, dropout=bdr)
        wl, wdf = ctx.ae1_wp_step(feats, tok, dropout=dr, want_dfeats=True, **kw)
        wg = ctx.get_grads()
        gl, gdf = ctx.ae1_wp_step_images(v, img, 8, 8, tok, body_dropout=bdr, dropout=dr, want_dfeats=True, **kw)
        gg = ctx.get_grads()
        gl2 = ctx.ae1_wp_step_images(v, img, 8, 8, tok, body_dropout=bdr, dropout=dr, **kw)  # without d(f^): the same step
        gg2 = ctx.get_grads()
    finally:
        ctx.close()
        v.close()
    assert np.isfinite(wl) and np.any(wg) and np.any(wdf)
    assert gl == wl and gl2 == wl, (gl, gl2, wl)
    assert np.array_equal(gg, wg) and np.array_equal(gg2, wg)
    assert np.array_equal(gdf, wdf)


def test_evaluate_images_equals_composed_route(pkg, orc):
    """n < B rows: loss and greedy samples, both archs; the padding rows of the feature slot stay zero"""
    b = pkg.binding
    n = 3
    v = _body(pkg, orc)
    ctx2, rng2 = _ctx2(pkg, "wp2_eval")
    ctx1, rng1 = _ctx1(pkg, "wp1_eval")
    try:
        img = vref.raw_images(n, S, 53)
        feats = v.fc7_raw(img, 3, 3)
        tok2, tok1 = _tokens(rng2, n, WP2[1], WP2[2]), _tokens(rng1, n, WP1[1], WP1[2])
        # a full step first, so that rows n..B of the feature slot hold something to be cleared
        ctx2.ae_wp_step_images(v, vref.raw_images(WP2[0], S, 54), 0, 0, _tokens(rng2, WP2[0], WP2[1], WP2[2]))
        ctx1.ae1_wp_step_images(v, vref.raw_images(WP1[0], S, 55), 0, 0, _tokens(rng1, WP1[0], WP1[1], WP1[2]),
                                enc_tokens=_tokens(rng1, WP1[0], WP1[1], WP1[2]))
        w2 = ctx2.ae_wp_evaluate(feats, tok2, enc_tokens=tok2, samples=True)
        g2 = ctx2.ae_wp_evaluate_images(v, img, 3, 3, tok2, enc_tokens=tok2, samples=True)
        w1 = ctx1.ae1_wp_evaluate(feats, tok1, tok1, samples=True)
        g1 = ctx1.ae1_wp_evaluate_images(v, img, 3, 3, tok1, tok1, samples=True)
        # the arch2 script's never-evaluate()d body: dropout in the evaluation's body pass
        bdr = b.Dropout(1, 0.5, 5, 9)
        feats_d = v.fc7_raw(img, 3, 3, dropout=bdr)
        w2d = ctx2.ae_wp_evaluate(feats_d, tok2, enc_tokens=tok2, samples=True)
        g2d = ctx2.ae_wp_evaluate_images(v, img, 3, 3, tok2, enc_tokens=tok2, body_dropout=bdr, samples=True)
    finally:
        ctx2.close()
        ctx1.close()
        v.close()
    for got, want in ((g2, w2), (g1, w1), (g2d, w2d)):
        assert np.isfinite(want[0]) and got[0] == want[0], (got[0], want[0])
        assert np.array_equal(got[1], want[1])
    assert not np.array_equal(feats_d, feats)


def test_back_to_back_steps_without_a_sync(pkg, orc):
    """Two steps on different images enqueued with loss_out = NULL, each followed by nvqa_adam_update, one sync at the end:
    the parameters equal those of the same two steps with a sync after every call.  The second body pass overwrites the
    features and the extractor's activation buffers of the first: it must wait until the context has taken its copy."""
    b = pkg.binding
    B, D, V, E, R, L, I = WP2
    out = []
    for synced in (True, False):
        ctx, rng = _ctx2(pkg, "wp2_b2b")
        v = _body(pkg, orc)
        try:
            toks = [_tokens(rng, B, D, V) for _ in range(2)]
            imgs = [vref.raw_images(B, S, 61), vref.raw_images(B, S, 62)]
            for i in range(2):
                ctx.ae_wp_step_images(v, imgs[i], 7 - i, 3 + i, toks[i], enc_tokens=toks[i], body_dropout=b.Dropout(1, 0.5, 77, i + 1),
                                      dropout=b.Dropout(1, 0.5, 78, i + 1), want_loss=False)
                if synced:
                    ctx.sync()
                ctx.adam_update(1e-2, clamp=0.1)
                if synced:
                    ctx.sync()
            ctx.sync()
            out.append((ctx.get_params(), ctx.get_grads(), *ctx.ae_wp_get_projection_grads()))
        finally:
            ctx.close()
            v.close()
    for a, c in zip(*out):
        assert np.all(np.isfinite(a)) and np.array_equal(a, c)
    assert np.any(out[0][1]) and np.any(out[0][2])


def _raises(b, fn, *a, **kw):
    with pytest.raises(b.NvqaError):
        fn(*a, **kw)


def test_refusals(pkg, orc):
    import torch
    b = pkg.binding
    B2, D2, V2 = WP2[:3]
    B1, D1, V1 = WP1[:3]
    ctx2, rng2 = _ctx2(pkg, "wp2_refuse")
    ctx1, rng1 = _ctx1(pkg, "wp1_refuse")
    ae2 = b.Context(b.Dims(b.ARCH_AE2, B2, D2, V2, 12, 8, 1, 0, 0, 0), 0)
    v = _body(pkg, orc)
    wide = _body(pkg, orc, div=8)                     # F = 512 != dims.I
    empty = b.Vgg16(0, DIV, HW, max_batch=6)          # no weights
    try:
        tok2, tok1 = _tokens(rng2, B2, D2, V2), _tokens(rng1, B1, D1, V1)
        img2, img1 = vref.raw_images(B2, S, 71), vref.raw_images(B1, S, 72)
        want2 = ctx2.ae_wp_step_images(v, img2, 7, 3, tok2, enc_tokens=tok2)
        want2g = ctx2.get_grads()
        want1 = ctx1.ae1_wp_step_images(v, img1, 7, 3, tok1, enc_tokens=tok1)
        # the wrong context arch, in both directions and for a context that is not weak-paired
        _raises(b, ctx1.ae_wp_step_images, v, img1, 7, 3, tok1, enc_tokens=tok1)
        _raises(b, ctx1.ae_wp_evaluate_images, v, img1, 7, 3, tok1, enc_tokens=tok1)
        _raises(b, ctx2.ae1_wp_step_images, v, img2, 7, 3, tok2, enc_tokens=tok2)
        _raises(b, ctx2.ae1_wp_evaluate_images, v, img2, 7, 3, tok2, tok2)
        _raises(b, ae2.ae_wp_step_images, v, img2, 7, 3, tok2, enc_tokens=tok2)
        _raises(b, ae2.ae1_wp_step_images, v, img2, 7, 3, tok2, enc_tokens=tok2)
        # the extractor: feature width, no weights, and what nvqa_vgg16_fc7_raw refuses
        _raises(b, ctx2.ae_wp_step_images, wide, img2, 7, 3, tok2, enc_tokens=tok2)
        _raises(b, ctx1.ae1_wp_step_images, wide, img1, 7, 3, tok1, enc_tokens=tok1)
        _raises(b, ctx2.ae_wp_step_images, empty, img2, 7, 3, tok2, enc_tokens=tok2)
        _raises(b, ctx2.ae_wp_step_images, v, vref.raw_images(B2, HW - 8, 1), 0, 0, tok2, enc_tokens=tok2)
        for xoff, yoff in [(-1, 0), (0, -1), (S - HW + 1, 0), (0, S - HW + 1)]:
            _raises(b, ctx2.ae_wp_step_images, v, img2, xoff, yoff, tok2, enc_tokens=tok2)
            _raises(b, ctx1.ae1_wp_evaluate_images, v, img1[:2], xoff, yoff, tok1[:2], tok1[:2])
        _raises(b, ctx2.ae_wp_step_images, v, img2, 7, 3, tok2, enc_tokens=tok2, body_dropout=b.Dropout(1, 1.0, 1, 1))
        _raises(b, ctx1.ae1_wp_step_images, v, img1, 7, 3, tok1, enc_tokens=tok1, body_dropout=b.Dropout(1, -0.5, 1, 1))
        small = b.Vgg16(0, DIV, HW, max_batch=B2 - 1)  # n = B above the extractor's max_batch
        small.set_weights(_weights(orc))
        _raises(b, ctx2.ae_wp_step_images, small, img2, 7, 3, tok2, enc_tokens=tok2)
        small.close()
        if torch.cuda.device_count() > 1:            # an extractor on another device
            far = b.Vgg16(1, DIV, HW, max_batch=6)
            far.set_weights(_weights(orc))
            _raises(b, ctx2.ae_wp_step_images, far, img2, 7, 3, tok2, enc_tokens=tok2)
            far.close()
        # what the host-fed calls refuse
        bad = tok2.copy()
        bad[1, 0] = V2 + 1
        _raises(b, ctx2.ae_wp_step_images, v, img2, 7, 3, bad, enc_tokens=tok2)
        _raises(b, ctx2.ae_wp_step_images, v, img2, 7, 3, tok2, enc_tokens=bad)
        _raises(b, ctx2.ae_wp_step_images, v, img2, 7, 3, np.zeros_like(tok2), enc_tokens=tok2)
        _raises(b, ctx1.ae1_wp_step_images, v, img1, 7, 3, tok1)                                     # neither encoder input
        _raises(b, ctx1.ae1_wp_step_images, v, img1, 7, 3, tok1, enc_tokens=tok1,
                enc_state=np.zeros((B1, 2 * WP1[4]), np.float32))                                    # both
        _raises(b, ctx1.ae1_wp_step_images, v, img1, 7, 3, tok1, enc_tokens=np.zeros_like(tok1))     # an empty encoder
        with pytest.raises((ValueError, b.NvqaError)):
            ctx2.ae_wp_evaluate_images(v, vref.raw_images(B2 + 1, S, 3), 7, 3, _tokens(rng2, B2 + 1, D2, V2))  # n > B
        with pytest.raises(ValueError):
            ctx2.ae_wp_step_images(v, img2.astype(np.float32), 7, 3, tok2)
        # every refusal came before any launch: the same good calls give the same bits
        assert ctx2.ae_wp_step_images(v, img2, 7, 3, tok2, enc_tokens=tok2) == want2
        assert np.array_equal(ctx2.get_grads(), want2g)
        assert ctx1.ae1_wp_step_images(v, img1, 7, 3, tok1, enc_tokens=tok1) == want1
    finally:
        for h in (ctx2, ctx1, ae2, v, wide, empty):
            h.close()


def test_trainer_with_the_body_in_the_loop(pkg, orc):
    """WeakPairedAETrainer(body=...) on a WeakPairedImageLoader: three iterations of train(), then eval_split"""
    b, ae = pkg.binding, pkg.ae
    B, D, V, E, R, L, I = WP2
    rng = np.random.default_rng(81)
    labels = {"train": _tokens(rng, B, D, V), "val": _tokens(rng, B, D, V)}
    images = {"train": vref.raw_images(B, S, 82), "val": vref.raw_images(B, S, 83)}
    loader = ae.WeakPairedImageLoader(labels, images, ix_to_word={str(i): "w%d" % i for i in range(1, V + 1)})
    v = _body(pkg, orc)
    tr = ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), learning_rate=1e-2, body=v)
    try:
        losses = tr.train(loader, 3, log=None)
        print("trainer losses", losses)
        assert tr.iter == 4 and all(np.isfinite(x) for x in losses)
        assert losses[1] <= losses[0] and losses[2] <= losses[1], losses
        loss, preds = tr.eval_split(loader, "val")
        assert np.isfinite(loss) and len(preds) == B
        tr.body_dropout_in_eval = True
        loss_d, _ = tr.eval_split(loader, "val")
        assert np.isfinite(loss_d)  # (that the flag reaches the body: tests/test_vgg_body_ref.py)
        tr.body = None
        with pytest.raises(ValueError):
            tr.train_step_images(labels["train"], images["train"])  # raw images without a body
        assert tr.iter == 4
    finally:
        tr.ctx.close()
        v.close()
