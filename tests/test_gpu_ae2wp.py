"""Weak-paired auto-encoder on the device (NVQA_ARCH_AE2_WP): loss, the encoder / decoder gradients and the projection's dW_p,
db_p against the float64 PyTorch model of tests/ae2wp_ref_torch.py; the frozen lookup; the cross-checks against AE2's
nvqa_ae_step_images fed host-projected rows; evaluate; both Adam updates against numpy; determinism; the refusals; and the
pipeline AE2 export -> weak-paired training -> arch2 VQATrainer with the projection as cnn_w."""
import ctypes
import zlib

import numpy as np
import pytest

import ae2wp_ref_torch as ref
from util import record

pytestmark = pytest.mark.gpu

# test_gpu_ae2.py's tolerances (the same kernels and sums); dW_p and db_p are held to the gradients' bound
TOL_LOSS = 1e-6
TOL_GRAD = 2e-5


def make(pkg, B, D, V, E, R, L, I):
    b = pkg.binding
    return b.Context(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), 0)


def tokens(rng, B, D, V, lo=1, tmax=None):
    lens = rng.integers(lo, D + 1, B)
    if tmax is not None:
        lens = np.minimum(lens, tmax)
        lens[0] = tmax
    else:
        lens[0] = D
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def features(rng, B, I):
    """post-ReLU-like rows: non-negative with zeros"""
    f = rng.uniform(0, 1, (B, I)).astype(np.float32)
    f[rng.uniform(0, 1, (B, I)) < 0.3] = 0.0
    return f


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def seg_errors(lo, got, want):
    out = {}
    for k, (o, n) in ((k, v) for k, v in lo.items() if not k.startswith("_") and k != "w_lk"):
        out[k] = rel_err(got[o:o + n], want[o:o + n])
    return out


def setup(pkg, dims, seed_name, tmax=None, enc="same"):
    B, D, V, E, R, L, I = dims
    rng = np.random.default_rng(zlib.crc32(seed_name.encode()))
    lo = ref.layout(B, D, V, E, R, L)
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    w = rng.uniform(-0.08, 0.08, (E, I)).astype(np.float32)
    bb = rng.uniform(-0.05, 0.05, E).astype(np.float32)
    tok = tokens(rng, B, D, V, tmax=tmax)
    et = {"same": tok, "null": None, "other": tokens(rng, B, D, V, tmax=max(1, (tmax or D) - 1))}[enc]
    return rng, lo, p, w, bb, features(rng, B, I), tok, et


CASES = [
    # name, (B, D, V, E, R, L, I), dropout, encoder tokens (same = tokens, null, other), tmax (None: a full-length batch)
    ("null_l1", (6, 5, 23, 8, 12, 1, 16), False, "null", None),
    ("same_l1", (6, 5, 23, 8, 12, 1, 16), False, "same", None),
    ("ragged_l2_same", (7, 6, 19, 8, 8, 2, 12), False, "same", 4),
    ("ragged_other", (7, 6, 19, 8, 8, 1, 8), False, "other", 4),
    ("drop_l1_same", (5, 5, 17, 12, 8, 1, 16), True, "same", None),
    ("drop_l2_null_ragged", (6, 6, 21, 8, 12, 2, 20), True, "null", 3),
    ("e512_r512_i4096", (8, 4, 30, 512, 512, 1, 4096), False, "same", None),
    ("i2048", (6, 5, 25, 16, 16, 1, 2048), False, "same", None),
    ("full_vocab", (4, 5, 14773, 16, 16, 1, 32), False, "same", None),
    ("b20_null", (20, 16, 50, 32, 32, 1, 64), False, "null", None),
    ("b20_drop_same", (20, 6, 50, 16, 16, 1, 64), True, "same", 5),
    ("b13_odd_other", (13, 6, 40, 16, 16, 1, 24), False, "other", None),
]


@pytest.mark.parametrize("name,dims,drop,enc,tmax", CASES, ids=[c[0] for c in CASES])
def test_ae2wp_step_matches_float64_model(pkg, name, dims, drop, enc, tmax):
    rng, lo, p, w, bb, f, tok, et = setup(pkg, dims, name, tmax, enc)
    dr = pkg.binding.Dropout(1, 0.5, 77, 3) if drop else None
    ctx = make(pkg, *dims)
    try:
        assert ctx.param_count == lo["_total"]
        assert ctx.segments() == (lo["_seg0"], lo["_seg1"], lo["_seg2"])
        ctx.set_params(p)
        ctx.ae_wp_set_projection(w, bb)
        loss = ctx.ae_wp_step(f, tok, enc_tokens=et, dropout=dr)
        g = ctx.get_grads()
        gw, gb = ctx.ae_wp_get_projection_grads()
        w2, b2 = ctx.ae_wp_get_projection()
    finally:
        ctx.close()
    assert np.array_equal(w2, w) and np.array_equal(b2, bb)  # the step does not move the projection
    want = ref.forward(dims, p.astype(np.float64), w, bb, f, tok, enc_tokens=et, dr=dr)
    assert want["te"] == ref.encoder_steps(et)
    el = abs(loss - want["loss"]) / abs(want["loss"])
    eg = seg_errors(lo, g, want["grads"])
    ew, eb = rel_err(gw, want["dw_p"]), rel_err(gb, want["db_p"])
    record("ae2wp_" + name, {"loss_rel": el, "grad_rel_max": max(eg.values()), "worst": max(eg, key=eg.get), "dw_p_rel": ew,
                             "db_p_rel": eb})
    o, n = lo["w_lk"]
    assert not np.any(g[o:o + n]), "the frozen lookup table received a gradient"
    assert el < TOL_LOSS, (loss, want["loss"])
    assert max(eg.values()) < TOL_GRAD, eg
    assert ew < TOL_GRAD and eb < TOL_GRAD, (ew, eb)


def _raw_step(ctx, f, et, tok, dr):
    """nvqa_ae_wp_step through ctypes, so that an all-zero enc_tokens array is passed as such"""
    f32, i32 = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    loss = ctypes.c_float(0)
    f = np.ascontiguousarray(f, np.float32)
    tok = np.ascontiguousarray(tok, np.int32)
    etp = None if et is None else np.ascontiguousarray(et, np.int32).ctypes.data_as(i32)
    rc = ctx.lib.nvqa_ae_wp_step(ctx._h, f.ctypes.data_as(f32), etp, tok.ctypes.data_as(i32), ctypes.byref(dr), ctypes.byref(loss))
    assert rc == 0, ctx.lib.nvqa_last_error()
    return float(loss.value)


def test_zero_enc_tokens_equal_null_bit_for_bit(pkg):
    dims = B, D, V, E, R, L, I = (8, 6, 25, 16, 16, 2, 32)
    _, _, p, w, bb, f, tok, _ = setup(pkg, dims, "zero_vs_null", tmax=5)
    dr = pkg.binding.Dropout(1, 0.5, 9, 2)
    ctx = make(pkg, *dims)
    out = []
    try:
        ctx.set_params(p)
        ctx.ae_wp_set_projection(w, bb)
        for et in (None, np.zeros((B, D), np.int32)):
            loss = _raw_step(ctx, f, et, tok, dr)
            out.append((loss, ctx.get_grads(), *ctx.ae_wp_get_projection_grads()))
    finally:
        ctx.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
def test_same_tokens_match_ae2_step_images_on_projected_rows(pkg, drop):
    """enc_tokens = tokens: the encoder is AE2's with the image row x0, so an AE2 context fed the host-projected rows gives the
    same loss and [encoder | decoder] gradients, and its d(images) gives dW_p = d(images)^T f^, db_p = colsum(d(images))"""
    dims = B, D, V, E, R, L, I = (12, 6, 33, 16, 24, 2, 40)
    _, lo, p, w, bb, f, tok, _ = setup(pkg, dims, "vs_ae2", tmax=5)
    dr = pkg.binding.Dropout(1, 0.5, 31, 7) if drop else None
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ctx.ae_wp_set_projection(w, bb)
        loss = ctx.ae_wp_step(f, tok, enc_tokens=tok, dropout=dr)
        g = ctx.get_grads()
        gw, gb = ctx.ae_wp_get_projection_grads()
    finally:
        ctx.close()
    fhat = ref.l2_normalize(f)
    x0 = (fhat @ w.astype(np.float64).T + bb).astype(np.float32)
    b = pkg.binding
    a2 = b.Context(b.Dims(b.ARCH_AE2, B, D, V, E, R, L, 0, 0, 0), 0)
    try:
        a2.set_params(p)
        l2, dimg = a2.ae_step(tok, dr, images=x0, want_dimages=True)
        g2 = a2.get_grads()
    finally:
        a2.close()
    n = lo["_seg0"] + lo["_seg1"]
    dimg = dimg.astype(np.float64)
    errs = {"loss": abs(loss - l2) / abs(l2), "encdec": rel_err(g[:n], g2[:n]), "dw_p": rel_err(gw, dimg.T @ fhat),
            "db_p": rel_err(gb, dimg.sum(0))}
    record("ae2wp_vs_ae2_" + ("drop" if drop else "nodrop"), errs)
    assert errs["loss"] < TOL_LOSS and max(errs.values()) < TOL_GRAD, errs
    assert not np.any(g[n:])


def test_ae2wp_evaluate_loss_and_greedy_samples(pkg):
    dims = B, D, V, E, R, L, I = (6, 5, 13, 8, 8, 2, 16)
    rng = np.random.default_rng(5)
    lo = ref.layout(B, D, V, E, R, L)
    p = rng.uniform(-0.6, 0.6, lo["_total"]).astype(np.float32)  # wide weights: decisive argmaxes
    w = rng.uniform(-0.6, 0.6, (E, I)).astype(np.float32)
    bb = rng.uniform(-0.3, 0.3, E).astype(np.float32)
    tok = tokens(rng, B, D, V, tmax=4)
    f = features(rng, B, I)
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ctx.ae_wp_set_projection(w, bb)
        ev_loss, samples = ctx.ae_wp_evaluate(f, tok, enc_tokens=tok, samples=True)
        tr_loss = ctx.ae_wp_step(f, tok, enc_tokens=tok)
        null_loss, null_samples = ctx.ae_wp_evaluate(f, tok, samples=True)
        n_loss, n_samples = ctx.ae_wp_evaluate(f[:4], tok[:4], enc_tokens=tok[:4], samples=True)
    finally:
        ctx.close()
    assert ev_loss == tr_loss
    want = ref.greedy(dims, p.astype(np.float64), w, bb, f, tok)
    assert np.array_equal(samples, want), (samples, want)
    assert np.array_equal(null_samples, ref.greedy(dims, p.astype(np.float64), w, bb, f, None))
    pad_tok = np.zeros((B, D), np.int32)
    pad_tok[:4] = tok[:4]
    pad_f = np.zeros((B, I), np.float32)
    pad_f[:4] = f[:4]
    assert np.array_equal(n_samples, ref.greedy(dims, p.astype(np.float64), w, bb, pad_f, pad_tok, nvalid=4)[:4])
    full = ref.forward(dims, p.astype(np.float64), w, bb, f, tok, enc_tokens=tok, train=False, want_grads=False)
    null = ref.forward(dims, p.astype(np.float64), w, bb, f, tok, train=False, want_grads=False)
    sub = ref.forward(dims, p.astype(np.float64), w, bb, pad_f, pad_tok, enc_tokens=pad_tok, train=False, want_grads=False,
                      nvalid=4)
    errs = {"eval": abs(ev_loss - full["loss"]) / full["loss"], "eval_null": abs(null_loss - null["loss"]) / null["loss"],
            "eval_n4": abs(n_loss - sub["loss"]) / sub["loss"]}
    record("ae2wp_evaluate", errs)
    assert max(errs.values()) < TOL_LOSS, errs


def _np_adam(x, g, m, v, t, lr, b1, b2, eps):
    f = np.float32
    m = f(b1) * m + (f(1) - f(b1)) * g
    v = f(b2) * v + (f(1) - f(b2)) * g * g
    step = f(lr * np.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t))
    return x - step * (m / (np.sqrt(v) + f(eps))), m, v


def test_adam_update_leaves_the_frozen_lookup_alone(pkg):
    dims = B, D, V, E, R, L, I = (6, 5, 21, 8, 12, 1, 16)
    _, lo, p, w, bb, f, tok, _ = setup(pkg, dims, "adam_frozen")
    lr, b1, b2, eps, wd, clamp = 1e-3, 0.8, 0.999, 1e-8, 1e-3, 0.01
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ctx.ae_wp_set_projection(w, bb)
        ctx.ae_wp_step(f, tok, enc_tokens=tok)
        g = ctx.get_grads()
        norm, count = ctx.adam_update(lr, b1, b2, eps, wd, clamp, stats=True)
        x1 = ctx.get_params()
    finally:
        ctx.close()
    n = lo["_seg0"] + lo["_seg1"]
    assert np.array_equal(x1[n:], p[n:]), "W_lk moved"
    gc = np.clip(g[:n], -clamp, clamp) + np.float32(wd) * p[:n]
    want, _, _ = _np_adam(p[:n], gc, np.zeros(n, np.float32), np.zeros(n, np.float32), 1, lr, b1, b2, eps)
    assert np.abs(x1[:n] - want).max() <= 1e-6 * max(np.abs(want).max(), 1.0)
    assert abs(norm - np.sqrt((p[:n].astype(np.float64) ** 2).sum())) < 1e-5 * norm
    want_count = int((np.abs(gc * np.float32(lr)) >= np.abs(p[:n]) * np.float32(0.01)).sum())
    assert abs(count - want_count) <= 2, (count, want_count)


def test_projection_adam_matches_numpy_with_decay_then_clamp(pkg):
    dims = B, D, V, E, R, L, I = (6, 5, 21, 8, 12, 1, 16)
    _, _, p, w, bb, f, tok, _ = setup(pkg, dims, "proj_adam")
    lr, b1, b2, eps, wd, clamp = 1e-2, 0.8, 0.999, 1e-8, 0.5, 2e-3
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ctx.ae_wp_set_projection(w, bb)
        x = np.concatenate([w.ravel(), bb])
        m, v = np.zeros_like(x), np.zeros_like(x)
        for t in (1, 2):
            ctx.ae_wp_step(f, tok, enc_tokens=tok)
            gw, gb = ctx.ae_wp_get_projection_grads()
            ctx.adam_update(1e-3, b1, b2, eps, 0.0, 0.1)  # the AE parameters' counter runs on its own
            norm, count = ctx.ae_wp_projection_adam(lr, b1, b2, eps, wd, clamp, stats=True)
            g = np.clip(np.concatenate([gw.ravel(), gb]) + np.float32(wd) * x, -clamp, clamp)  # wd first, then clamp
            want_norm = float(np.sqrt((x[:E * I].astype(np.float64) ** 2).sum()))
            want_count = int((np.abs(g * np.float32(lr)) >= np.abs(x) * np.float32(0.01)).sum())
            x, m, v = _np_adam(x, g, m, v, t, lr, b1, b2, eps)
            w2, b2_ = ctx.ae_wp_get_projection()
            got = np.concatenate([w2.ravel(), b2_])
            assert np.abs(got - x).max() <= 1e-6 * max(np.abs(x).max(), 1.0), t
            assert abs(norm - want_norm) < 1e-5 * want_norm
            assert abs(count - want_count) <= 2, (count, want_count)
            x = got
    finally:
        ctx.close()


def test_ae2wp_step_is_deterministic(pkg):
    dims = B, D, V, E, R, L, I = (16, 6, 40, 16, 16, 2, 64)
    _, _, p, w, bb, f, tok, _ = setup(pkg, dims, "determinism")
    out = []
    for _ in range(2):
        ctx = make(pkg, *dims)
        try:
            ctx.set_params(p)
            ctx.ae_wp_set_projection(w, bb)
            loss = ctx.ae_wp_step(f, tok, enc_tokens=tok, dropout=pkg.binding.Dropout(1, 0.5, 5, 1))
            out.append((loss, ctx.get_grads(), *ctx.ae_wp_get_projection_grads()))
        finally:
            ctx.close()
    assert out[0][0] == out[1][0]
    for a, b in zip(out[0][1:], out[1][1:]):
        assert np.array_equal(a, b)


def test_ae2wp_init_params_draws_the_projection(pkg):
    dims = B, D, V, E, R, L, I = (4, 5, 9, 8, 8, 1, 16)
    ctx = make(pkg, *dims)
    try:
        ctx.init_params(7, -0.08, 0.08)
        w, b = ctx.ae_wp_get_projection()
        ctx.init_params(7, -0.08, 0.08)
        w2, _ = ctx.ae_wp_get_projection()
    finally:
        ctx.close()
    assert not np.any(b) and np.array_equal(w, w2)
    assert w.min() >= -0.08 and w.max() <= 0.08 and w.std() > 0.03


def test_ae2wp_refusals_and_other_archs_refuse_the_wp_calls(pkg):
    B, D, V, E, R, I = 4, 5, 9, 8, 8, 16
    b = pkg.binding
    Err = b.NvqaError
    tok = np.array([[1, 2, 0, 0, 0]] * B, np.int32)
    f = np.ones((B, I), np.float32)
    for bad_i in (0, 6):
        with pytest.raises(Err, match="multiple of 4"):
            b.Context(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, 1, bad_i, 0, 0), 0)
    ctx = make(pkg, B, D, V, E, R, 1, I)
    try:
        with pytest.raises(Err, match="before any"):
            ctx.ae_wp_projection_adam(1e-3)
        with pytest.raises(Err, match="weak-paired"):
            ctx.ae_step(tok)
        with pytest.raises(Err, match="weak-paired"):
            ctx.ae_evaluate(tok)
        with pytest.raises(Err, match="NVQA_ARCH_AE2"):
            ctx.ae_step(tok, images=np.zeros((B, E), np.float32))
        with pytest.raises(Err, match="NVQA_ARCH_AE2"):
            ctx.ae_evaluate(tok, images=np.zeros((B, E), np.float32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.step(tok, np.full(B, D, np.int32), np.zeros((B, I), np.float32), np.ones(B, np.int32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.forward(tok, np.full(B, D, np.int32), np.zeros((B, I), np.float32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.evaluate(tok, np.full(B, D, np.int32), np.zeros((B, I), np.float32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.set_ref_quirks(1)
        with pytest.raises(Err, match="auto-encoder"):
            ctx.dataset_load(tok, None, np.ones(B, np.int32), np.ones(B, np.int32), np.zeros((1, 4), np.float32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.step_indices(np.zeros(B, np.int64))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.comm_init(0, 1, bytes(128))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.set_precision(1)
        with pytest.raises(Err, match="outside"):
            ctx.ae_wp_step(f, tok, enc_tokens=np.full((B, D), V + 1, np.int32))
        ctx.init_params(1)
        loss = ctx.ae_wp_step(f, tok)
        assert np.isfinite(loss)
        with pytest.raises(Err, match="weak-paired"):
            ctx.rmsprop_update(1e-3)
        ctx.adam_update(1e-3, 0.8, 0.999, 1e-8, 1e-6, 0.1)
        ctx.ae_wp_projection_adam(1e-5)
        assert np.all(np.isfinite(ctx.param_norms()))
    finally:
        ctx.close()
    others = [b.Dims(b.ARCH_AE1, B, D, V, E, R, 1, 0, 0, 0), b.Dims(b.ARCH_AE2, B, D, V, E, R, 1, 0, 0, 0),
              b.Dims(b.ARCH2, B, D, V, E, R, 1, I, 0, 8)]
    for dims in others:
        c = b.Context(dims, 0)
        try:
            c.dims = b.Dims(dims.arch, B, D, V, E, R, 1, I, 0, 0)  # the binding's shapes for the calls below
            for call in (lambda: c.ae_wp_step(f, tok), lambda: c.ae_wp_evaluate(f, tok),
                         lambda: c.ae_wp_set_projection(np.zeros((E, I)), np.zeros(E)), c.ae_wp_get_projection,
                         c.ae_wp_get_projection_grads, lambda: c.ae_wp_projection_adam(1e-3)):
                with pytest.raises(Err, match="NVQA_ARCH_AE2_WP"):
                    call()
        finally:
            c.close()


def test_pipeline_ae2_export_weakpaired_training_into_arch2_vqa(pkg, tmp_path):
    B, D, V, E, R, L, I = 16, 6, 30, 16, 16, 1, 24
    rng = np.random.default_rng(1)
    sents = tokens(rng, 64, D, V, lo=2)
    feats = features(rng, 64, I)
    words = {str(i): f"w{i}" for i in range(1, V + 1)}
    b = pkg.binding
    ae = pkg.ae.AETrainer(b.Dims(b.ARCH_AE2, B, D, V, E, R, L, 0, 0, 0), learning_rate=1e-2)
    ae.train(pkg.ae.DataLoader(labels={"train": sents}, ix_to_word=words), 5, log=None)
    text_path = str(tmp_path / "ae2_text.t7")
    ae.export_params(text_path)
    x_text = ae.ctx.get_params()
    ae.ctx.close()

    loader = pkg.ae.WeakPairedDataLoader(labels={"train": sents, "val": sents[:32]}, feats={"train": feats, "val": feats[:32]},
                                         ix_to_word=words)
    tr = pkg.ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), learning_rate=1e-3,
                                    finetune_cnn_after=0)
    tr.init_from_text(text_path)
    assert np.array_equal(tr.ctx.get_params(), x_text)
    lines = []
    losses = tr.train(loader, 6, log=lines.append)
    assert all(np.isfinite(losses))
    assert "# cnn updates:" in lines[0] and "cnnParamsNorm:" in lines[0]
    val_loss, preds = tr.eval_split(loader, "val", val_sentences_use=20)
    assert np.isfinite(val_loss) and len(preds) == 32  # n = 16, 32: the loop ends once n >= 20
    x_ae = tr.ctx.get_params()
    seg = tr.ctx.segments()
    assert np.array_equal(x_ae[seg[0] + seg[1]:], x_text[seg[0] + seg[1]:])  # the lookup table stayed frozen
    w, bb = tr.ctx.ae_wp_get_projection()
    path = str(tmp_path / "ae2wp_vqa.t7")
    tr.export_for_vqa(path)
    tr.ctx.close()

    A = 8
    vt = pkg.trainer.VQATrainer(b.Dims(b.ARCH2, 8, D, V, E, R, L, I, 0, A))
    try:
        vt.init_from_autoencoder(path, with_cnn=True)
        xv = vt.ctx.get_params()
        sv = vt.ctx.segments()
        n_lstm = seg[0]
        assert np.array_equal(xv[:E * I], w.ravel()) and np.array_equal(xv[E * I:sv[0]], bb)           # cnn_w
        assert np.array_equal(xv[sv[0]:sv[0] + n_lstm], x_ae[:n_lstm])                                   # encoder
        assert np.array_equal(xv[sv[0] + n_lstm:sv[0] + sv[1]], x_ae[seg[0] + seg[1]:])                 # lookup_table
        r2 = np.random.default_rng(2)
        loss = vt.ctx.step(tokens(r2, 8, D, V), None, r2.uniform(0, 1, (8, I)).astype(np.float32),
                           r2.integers(1, A + 1, 8).astype(np.int32))
        assert np.isfinite(loss)
    finally:
        vt.ctx.close()
