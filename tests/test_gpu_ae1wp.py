"""arch1 weak-paired auto-encoder on the device (NVQA_ARCH_AE1_WP): loss, every gradient tensor of [encoder | decoder |
multimodal] and d(loss)/d(f^) against the float64 PyTorch model of tests/ae1wp_ref_torch.py, with the encoder run and skipped;
the frozen lookup; Adam over the whole vector against numpy; determinism; evaluate, greedy samples and the encoder's state;
the refusals in both directions; and the pipeline AE1 text steps -> export -> weak-paired training -> arch1 VQA with AskipB."""
import zlib

import numpy as np
import pytest

import ae1wp_ref_torch as ref
from ae_ref_torch import Adam
from util import record

pytestmark = pytest.mark.gpu

# test_gpu_ae2.py / test_gpu_ae2wp.py's tolerances (the same kernels and sums); the multimodal tensors and d(f^) are held to
# the gradients' bound
TOL_LOSS = 1e-6
TOL_GRAD = 2e-5
# the project's logit tolerance (relative to the largest logit): samples are compared where the float64 model's decision is
# wider than twice that
TOL_LOGIT = 1e-4


def make(pkg, B, D, V, E, R, I):
    b = pkg.binding
    return b.Context(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, 2 * R, 0), 0)


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
    return {k: rel_err(got[o:o + n], want[o:o + n]) for k, (o, n) in ((k, v) for k, v in lo.items() if not k.startswith("_"))}


def setup(dims, seed_name, tmax=None, enc="same", scale=0.08):
    B, D, V, E, R, I = dims
    rng = np.random.default_rng(zlib.crc32(seed_name.encode()))
    lo = ref.layout(D, V, E, R, I)
    p = rng.uniform(-scale, scale, lo["_total"]).astype(np.float32)
    # the bridge as the trainer draws it (nn.Linear's default), so that tanh is neither flat nor saturated at I = 4096
    for w, fan_in in (("w_q", 2 * R), ("b_q", 2 * R), ("w_v", I), ("b_v", I)):
        o, n = lo[w]
        p[o:o + n] = rng.uniform(-1, 1, n) / np.sqrt(fan_in)
    wlk = rng.uniform(-1.0, 1.0, (V + 1, E)).astype(np.float32)
    tok = tokens(rng, B, D, V, tmax=tmax)
    et = {"same": tok, "other": tokens(rng, B, D, V, tmax=max(1, (tmax or D) - 1)), "skip": None}[enc]
    es = rng.uniform(-0.5, 0.5, (B, 2 * R)).astype(np.float32) if enc == "skip" else None
    return rng, lo, p, wlk, features(rng, B, I), tok, et, es


CASES = [
    # name, (B, D, V, E, R, I), dropout, encoder input (same = tokens, other tokens, skip = enc_state), tmax (None: full length)
    ("tiny_same", (6, 5, 23, 8, 12, 16), False, "same", None),
    ("tiny_skip", (6, 5, 23, 8, 12, 16), False, "skip", None),
    ("ragged_other", (7, 6, 19, 8, 8, 12), False, "other", 4),
    ("ragged_skip", (7, 6, 19, 8, 8, 12), False, "skip", 3),
    ("drop_same", (5, 5, 17, 12, 8, 16), True, "same", None),
    ("drop_skip", (5, 5, 17, 12, 8, 16), True, "skip", None),
    ("drop_ragged_other", (6, 6, 21, 8, 12, 20), True, "other", 3),
    ("b16_r512_i4096_same", (16, 4, 30, 32, 512, 4096), False, "same", None),
    ("b16_r512_i4096_drop_skip", (16, 4, 30, 32, 512, 4096), True, "skip", None),
    ("b10_r512_i2048_same", (10, 4, 30, 32, 512, 2048), False, "same", None),
    ("b10_r512_i2048_drop_same", (10, 4, 30, 32, 512, 2048), True, "same", 3),
    ("b13_odd_other", (13, 6, 40, 16, 16, 24), False, "other", None),
    ("b1", (1, 4, 12, 8, 8, 8), False, "same", None),
    ("b20_wide_same", (20, 6, 50, 16, 16, 64), True, "same", 5),
    ("b130_wide_skip", (130, 4, 20, 8, 8, 40), False, "skip", None),
    ("full_vocab", (4, 5, 14773, 16, 16, 32), False, "same", None),
]


@pytest.mark.parametrize("name,dims,drop,enc,tmax", CASES, ids=[c[0] for c in CASES])
def test_ae1wp_step_matches_float64_model(pkg, name, dims, drop, enc, tmax):
    """Measured on the MI355X (profiles/ae1wp_measured_errors.jsonl): loss <= 1.6e-7; the worst case of the
    table is full_vocab with gradients 4.9e-6 (b_v) and d(f^) 3.2e-6; at B = 16, R = 512, I = 4096 gradients 6.4e-7 and
    d(f^) 1.4e-6 -- against the bounds 1e-6 / 2e-5."""
    _, lo, p, wlk, f, tok, et, es = setup(dims, name, tmax, enc)
    dr = pkg.binding.Dropout(1, 0.5, 77, 3) if drop else None
    ctx = make(pkg, *dims)
    try:
        assert ctx.param_count == lo["_total"]
        assert ctx.segments() == (lo["_seg0"], lo["_seg1"], lo["_seg2"])
        ctx.set_params(p)
        assert np.array_equal(ctx.get_params(), p)
        ctx.ae1_wp_set_lookup(wlk)
        loss, df = ctx.ae1_wp_step(f, tok, enc_tokens=et, enc_state=es, dropout=dr, want_dfeats=True)
        g = ctx.get_grads()
        loss2 = ctx.ae1_wp_step(f, tok, enc_tokens=et, enc_state=es, dropout=dr)  # without d(f^): the same step
        g2 = ctx.get_grads()
    finally:
        ctx.close()
    assert loss2 == loss and np.array_equal(g, g2)
    want = ref.forward(dims, p.astype(np.float64), wlk, f, tok, enc_tokens=et, enc_state=es, dr=dr)
    el = abs(loss - want["loss"]) / abs(want["loss"])
    eg = seg_errors(lo, g, want["grads"])
    ed = rel_err(df, want["dfhat"])
    record("ae1wp_" + name, {"loss_rel": el, "grad_rel_max": max(eg.values()), "worst": max(eg, key=eg.get),
                             "mm_rel_max": max(eg[k] for k in ("w_q", "b_q", "w_v", "b_v")), "dfeats_rel": ed})
    print(name, "loss_rel %.3g" % el, "dfeats_rel %.3g" % ed, {k: "%.3g" % v for k, v in eg.items()})
    if enc == "skip":
        assert not np.any(g[:lo["_seg0"]]), "the skipped encoder received a gradient"
        assert not np.any(want["grads"][:lo["_seg0"]])
    else:
        assert np.abs(g[:lo["_seg0"]]).max() > 0
    assert el < TOL_LOSS, (loss, want["loss"])
    assert max(eg.values()) < TOL_GRAD, eg
    assert ed < TOL_GRAD, ed


def test_adam_over_the_whole_vector_and_the_lookup_stays_bit_identical(pkg):
    """two steps, the second with the encoder skipped: its zero gradient still takes the weight decay"""
    dims = B, D, V, E, R, I = (6, 5, 21, 8, 12, 16)
    _, lo, p, wlk, f, tok, _, _ = setup(dims, "adam_whole")
    es = np.random.default_rng(3).uniform(-0.5, 0.5, (B, 2 * R)).astype(np.float32)
    lr, b1, b2, eps, wd, clamp = 1e-3, 0.8, 0.999, 1e-8, 1e-3, 0.01
    adam = Adam(lo["_total"])
    x = p.copy()
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ctx.ae1_wp_set_lookup(wlk)
        for t, kw in enumerate(({"enc_tokens": tok}, {"enc_state": es})):
            ctx.ae1_wp_step(f, tok, **kw)
            g = ctx.get_grads()
            if t == 1:
                assert not np.any(g[:lo["_seg0"]])
            norm, count = ctx.adam_update(lr, b1, b2, eps, wd, clamp, stats=True)
            want, want_norm, want_count = adam.update(x, g, lr, b1, b2, eps, wd, clamp)
            got = ctx.get_params()
            assert np.abs(got - want).max() <= 1e-6 * max(np.abs(want).max(), 1.0), t
            assert abs(norm - want_norm) < 1e-5 * want_norm
            assert abs(count - want_count) <= 2, (count, want_count)
            if t == 1:
                assert np.any(got[:lo["_seg0"]] != x[:lo["_seg0"]]), "the decay did not reach the skipped encoder"
            x = got
        assert np.array_equal(ctx.ae1_wp_get_lookup(), wlk), "W_lk moved"
        assert np.all(np.isfinite(ctx.param_norms()))
        n0, n1 = lo["_seg0"], lo["_seg0"] + lo["_seg1"]
        want_norms = [np.sqrt((x[a:b].astype(np.float64) ** 2).sum()) for a, b in ((0, n0), (n0, n1), (n1, x.size))]
        assert np.allclose(ctx.param_norms(), want_norms, rtol=1e-5)
    finally:
        ctx.close()


@pytest.mark.parametrize("dims", [(16, 6, 40, 16, 64, 256), (40, 5, 30, 16, 16, 64)], ids=["skinny", "wide"])
def test_ae1wp_step_is_deterministic(pkg, dims):
    _, _, p, wlk, f, tok, _, _ = setup(dims, "determinism")
    es = np.random.default_rng(4).uniform(-0.5, 0.5, (dims[0], 2 * dims[4])).astype(np.float32)
    out = []
    for _ in range(2):
        ctx = make(pkg, *dims)
        try:
            ctx.set_params(p)
            ctx.ae1_wp_set_lookup(wlk)
            row = []
            for kw in ({"enc_tokens": tok}, {"enc_state": es}):
                loss, df = ctx.ae1_wp_step(f, tok, dropout=pkg.binding.Dropout(1, 0.5, 5, 1), want_dfeats=True, **kw)
                row += [np.float32(loss), ctx.get_grads(), df]
            out.append(row)
        finally:
            ctx.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)


def _sample_setup():
    """wide weights for decisive argmaxes; the seed is the first for which the float64 model alone has at least 90 % of its
    rows decided by more than twice the logit tolerance at every step (tests/test_ae1wp_host.py checks that on the CPU)"""
    dims = B, D, V, E, R, I = (20, 5, 13, 8, 8, 16)
    rng = np.random.default_rng(11)
    lo = ref.layout(D, V, E, R, I)
    p = rng.uniform(-0.6, 0.6, lo["_total"]).astype(np.float32)
    wlk = rng.uniform(-1.0, 1.0, (V + 1, E)).astype(np.float32)
    return dims, p, wlk, tokens(rng, B, D, V, tmax=4), features(rng, B, I)


def decided_rows(logit_scale, gap):
    return (gap > 2 * TOL_LOGIT * logit_scale).all(axis=1)


def test_ae1wp_evaluate_loss_samples_and_encode(pkg):
    dims, p, wlk, tok, f = _sample_setup()
    B, D, V, E, R, I = dims
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ctx.ae1_wp_set_lookup(wlk)
        ev_loss, samples = ctx.ae1_wp_evaluate(f, tok, tok, samples=True)
        tr_loss = ctx.ae1_wp_step(f, tok, enc_tokens=tok)
        state = ctx.ae1_wp_encode(tok)
        n_loss, n_samples = ctx.ae1_wp_evaluate(f[:4], tok[:4], tok[:4], samples=True)
        n_state = ctx.ae1_wp_encode(tok[:4])
    finally:
        ctx.close()
    assert ev_loss == tr_loss  # no dropout given: the training forward is the evaluate-mode one
    p64 = p.astype(np.float64)
    full = ref.forward(dims, p64, wlk, f, tok, enc_tokens=tok, train=False, want_grads=False)
    want, gap = ref.greedy(dims, p64, wlk, f, tok)
    ok = decided_rows(np.abs(full["logits"]).max(), gap)
    assert ok.mean() >= 0.9, ok
    assert np.array_equal(samples[ok], want[ok]), (samples, want)
    pad_tok = np.zeros((B, D), np.int32)
    pad_tok[:4] = tok[:4]
    pad_f = np.zeros((B, I), np.float32)
    pad_f[:4] = f[:4]
    pad_et = pad_tok.copy()
    sub = ref.forward(dims, p64, wlk, pad_f, pad_tok, enc_tokens=pad_et, train=False, want_grads=False, nvalid=4)
    want4, gap4 = ref.greedy(dims, p64, wlk, pad_f, pad_et, nvalid=4)
    ok4 = decided_rows(np.abs(sub["logits"]).max(), gap4)[:4]
    assert np.array_equal(n_samples[ok4], want4[:4][ok4])
    errs = {"eval": abs(ev_loss - full["loss"]) / full["loss"], "eval_n4": abs(n_loss - sub["loss"]) / sub["loss"],
            "encode": rel_err(state, ref.encode(dims, p64, wlk, tok)), "encode_n4": rel_err(n_state, sub["state"][:4])}
    record("ae1wp_evaluate", errs)
    assert max(errs["eval"], errs["eval_n4"]) < TOL_LOSS, errs
    assert max(errs["encode"], errs["encode_n4"]) < TOL_GRAD, errs
    assert rel_err(state, full["state"]) < TOL_GRAD


def test_ae1wp_refusals_in_both_directions(pkg):
    B, D, V, E, R, I = 4, 5, 9, 8, 8, 16
    b = pkg.binding
    Err = b.NvqaError
    tok = np.array([[1, 2, 0, 0, 0]] * B, np.int32)
    f = np.ones((B, I), np.float32)
    es = np.zeros((B, 2 * R), np.float32)
    with pytest.raises(Err, match="L must be 1"):
        b.Context(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 2, I, 2 * R, 0), 0)
    with pytest.raises(Err, match="C must be 2R"):
        b.Context(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, R, 0), 0)
    for bad_i in (0, 6):
        with pytest.raises(Err, match="multiple of 4"):
            b.Context(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, bad_i, 2 * R, 0), 0)
    ctx = make(pkg, B, D, V, E, R, I)
    try:
        with pytest.raises(Err, match="arch1 weak-paired"):
            ctx.ae_step(tok)
        with pytest.raises(Err, match="arch1 weak-paired"):
            ctx.ae_evaluate(tok)
        with pytest.raises(Err, match="NVQA_ARCH_AE2 "):
            ctx.ae_step(tok, images=np.zeros((B, E), np.float32))
        with pytest.raises(Err, match="NVQA_ARCH_AE2 "):
            ctx.ae_evaluate(tok, images=np.zeros((B, E), np.float32))
        for call in (lambda: ctx.ae_wp_step(f, tok), lambda: ctx.ae_wp_evaluate(f, tok), ctx.ae_wp_get_projection,
                     lambda: ctx.ae_wp_set_projection(np.zeros((E, I)), np.zeros(E)), lambda: ctx.ae_wp_projection_adam(1e-3)):
            with pytest.raises(Err, match="NVQA_ARCH_AE2_WP"):
                call()
        with pytest.raises(Err, match="auto-encoder"):
            ctx.step(tok, np.full(B, D, np.int32), np.zeros((B, I), np.float32), np.ones(B, np.int32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.forward(tok, np.full(B, D, np.int32), np.zeros((B, I), np.float32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.evaluate(tok, np.full(B, D, np.int32), np.zeros((B, I), np.float32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.set_fusion(1)
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
        with pytest.raises(Err, match="per-segment"):
            ctx.set_grad_scales([1.0, 0.5, 1.0])
        ctx.set_grad_scales([1.0, 1.0, 1.0])
        with pytest.raises(Err, match="exactly one"):
            ctx.ae1_wp_step(f, tok)
        with pytest.raises(Err, match="exactly one"):
            ctx.ae1_wp_step(f, tok, enc_tokens=tok, enc_state=es)
        with pytest.raises(Err, match="outside"):
            ctx.ae1_wp_step(f, tok, enc_tokens=np.full((B, D), V + 1, np.int32))
        with pytest.raises(Err, match="no token"):
            ctx.ae1_wp_step(f, tok, enc_tokens=np.zeros((B, D), np.int32))
        with pytest.raises(Err, match="no token"):
            ctx.ae1_wp_encode(np.zeros((B, D), np.int32))
        with pytest.raises(Err, match="before any"):
            ctx.adam_update(1e-3)
        ctx.init_params(1)
        assert np.isfinite(ctx.ae1_wp_step(f, tok, enc_tokens=tok))
        assert np.isfinite(ctx.ae1_wp_step(f, tok, enc_state=es))
        with pytest.raises(Err, match="weak-paired"):
            ctx.rmsprop_update(1e-3)
        ctx.adam_update(1e-3, 0.8, 0.999, 1e-8, 1e-6, 0.1)
    finally:
        ctx.close()
    others = [b.Dims(b.ARCH_AE1, B, D, V, E, R, 1, 0, 0, 0), b.Dims(b.ARCH_AE2, B, D, V, E, R, 1, 0, 0, 0),
              b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, 1, I, 0, 0), b.Dims(b.ARCH2, B, D, V, E, R, 1, I, 0, 8),
              b.Dims(b.ARCH1, B, D, V, E, R, 1, I, 2 * R, 8)]
    for dims in others:
        c = b.Context(dims, 0)
        try:
            c.dims = b.Dims(dims.arch, B, D, V, E, R, 1, I, 2 * R, 0)  # the binding's shapes for the calls below
            for call in (lambda: c.ae1_wp_step(f, tok, enc_tokens=tok), lambda: c.ae1_wp_step(f, tok, enc_state=es),
                         lambda: c.ae1_wp_evaluate(f, tok, tok), lambda: c.ae1_wp_encode(tok),
                         lambda: c.ae1_wp_set_lookup(np.zeros((V + 1, E))), c.ae1_wp_get_lookup):
                with pytest.raises(Err, match="NVQA_ARCH_AE1_WP|auto-encoder context"):
                    call()
        finally:
            c.close()


def test_pipeline_ae1_text_weakpaired_training_into_arch1_vqa_askipb(pkg, tmp_path):
    B, D, V, E, R, I = 16, 6, 30, 16, 16, 24
    rng = np.random.default_rng(1)
    sents = tokens(rng, 64, D, V, lo=2)
    feats = features(rng, 64, I)
    words = {str(i): f"w{i}" for i in range(1, V + 1)}
    b = pkg.binding
    ae = pkg.ae.AETrainer(b.Dims(b.ARCH_AE1, B, D, V, E, R, 1, 0, 0, 0), learning_rate=1e-2)
    ae.train(pkg.ae.DataLoader(labels={"train": sents}, ix_to_word=words), 5, log=None)
    text_path = str(tmp_path / "ae1_text.t7")
    ae.export_params(text_path)
    x_text = ae.ctx.get_params()
    ae.ctx.close()

    loader = pkg.ae.WeakPairedDataLoader(labels={"train": sents, "val": sents[:32]}, feats={"train": feats, "val": feats[:32]},
                                         ix_to_word=words)
    tr = pkg.ae.WeakPairedAE1Trainer(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, 2 * R, 0), learning_rate=1e-3)
    try:
        tr.init_from_text(text_path)
        seg = tr.ctx.segments()
        n_ed = seg[0] + seg[1]
        assert np.array_equal(tr.ctx.get_params()[:n_ed], x_text[:n_ed])
        wlk = x_text[n_ed:].reshape(V + 1, E)
        assert np.array_equal(tr.ctx.ae1_wp_get_lookup(), wlk)
        mean = tr.mean_sentence_vector(loader, "train")
        want_mean = np.mean([tr.ctx.ae1_wp_encode(sents[i:i + B]) for i in range(0, 64, B)], axis=(0, 1))
        assert mean.shape == (2 * R,) and np.allclose(mean, want_mean, rtol=1e-5, atol=1e-7)
        lines, skipped = [], []
        for _ in range(8):
            labels, fb, _ = loader.get_batch("train", B)
            out = tr.train_step(labels, fb)
            assert np.isfinite(out[0])
            skipped.append(out[3])
            lines.append(out[-1])
        assert any(skipped) and not all(skipped), skipped  # both modes ran
        assert lines[0].startswith("iter 1: loss: ") and "# updates:" in lines[0] and "paramsNorm:" in lines[0]
        val_loss, preds = tr.eval_split(loader, "val", val_sentences_use=20)
        assert np.isfinite(val_loss) and len(preds) == 32
        assert np.array_equal(tr.ctx.ae1_wp_get_lookup(), wlk)  # the lookup table stayed frozen
        x_ae = tr.ctx.get_params()
        assert np.any(x_ae[n_ed:] != 0) and np.any(x_ae[:seg[0]] != x_text[:seg[0]])
        path = str(tmp_path / "ae1wp_vqa.t7")
        tr.export_for_vqa(path)
    finally:
        tr.ctx.close()

    A, C = 8, 2 * R
    vt = pkg.trainer.VQATrainer(b.Dims(b.ARCH1, 8, D, V, E, R, 1, I, C, A))
    try:
        vt.ctx.set_fusion(1)  # netdef.AskipB
        vt.init_from_autoencoder(path, with_multimodal=True)
        xv = vt.ctx.get_params()
        sv = vt.ctx.segments()
        assert np.array_equal(xv[:sv[0]], x_ae[:seg[0]])                                             # encoder
        assert np.array_equal(xv[sv[0]:sv[0] + E * V].reshape(E, V), wlk[:V].T)                      # embedding <- lookup
        assert np.array_equal(xv[sv[0] + sv[1]:sv[0] + sv[1] + seg[2]], x_ae[n_ed:])                 # W_q, b_q, W_v, b_v
        r2 = np.random.default_rng(2)
        left = tokens(r2, 8, D, V)
        lens = (left != 0).sum(1).astype(np.int32)
        tok = np.zeros_like(left)  # arch1 questions are right-aligned
        for i, n in enumerate(lens):
            tok[i, D - n:] = left[i, :n]
        loss = vt.ctx.step(tok, lens, r2.uniform(0, 1, (8, I)).astype(np.float32),
                           r2.integers(1, A + 1, 8).astype(np.int32))
        assert np.isfinite(loss)
    finally:
        vt.ctx.close()
