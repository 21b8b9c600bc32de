"""Text auto-encoder on the device (NVQA_ARCH_AE1): loss and every gradient segment against the float64 PyTorch model of
tests/ae_ref_torch.py, evaluate-mode loss and greedy decoding, the fused Adam update against its NumPy mirror,
determinism, the entry points an auto-encoder context refuses, and the pipeline into VQATrainer.init_from_autoencoder."""
import zlib

import numpy as np
import pytest

import ae_ref_torch as ref
from util import record

pytestmark = pytest.mark.gpu

# measured errors are recorded (util.record; first MI355X run: loss <= 7e-8 relative, gradients <= 1.6e-6 of the tensor's largest
# element, worst at the full vocabulary width); tolerances: the loss is a mean of f32 log-softmax terms, the gradients are
# f32 sums over (steps x rows) and, for W_proj / b_proj, over the vocabulary-wide softmax
TOL_LOSS = 1e-6
TOL_GRAD = 2e-5


def make(pkg, B, D, V, E, R, L):
    return pkg.binding.Context(pkg.binding.Dims(3, B, D, V, E, R, L, 0, 0, 0), 0)


def tokens(rng, B, D, V, lo=1, hi=None, tmax=None):
    hi = D if hi is None else hi
    lens = rng.integers(lo, hi + 1, B)
    if tmax is not None:
        lens = np.minimum(lens, tmax)
        lens[0] = tmax
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def seg_errors(lo, got, want):
    out = {}
    for k, v in lo.items():
        if k.startswith("_"):
            continue
        o, n = v
        a, b = np.asarray(got[o:o + n], np.float64), np.asarray(want[o:o + n], np.float64)
        out[k] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    return out


CASES = [
    # name, (B, D, V, E, R, L), dropout, tmax
    ("l1_full", (6, 5, 23, 8, 12, 1), False, None),
    ("l2_ragged_short", (7, 6, 19, 8, 8, 2), False, 4),
    ("l1_drop", (5, 5, 17, 12, 8, 1), True, None),
    ("l2_drop_ragged", (6, 6, 21, 8, 12, 2), True, 3),
    ("e512_r512", (8, 4, 30, 512, 512, 1), False, None),
    ("full_vocab", (4, 5, 14773, 16, 16, 1), False, None),
]


@pytest.mark.parametrize("name,dims,drop,tmax", CASES, ids=[c[0] for c in CASES])
def test_ae_step_matches_float64_model(pkg, name, dims, drop, tmax):
    B, D, V, E, R, L = dims
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lo = ref.layout(*dims)
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    tok = tokens(rng, B, D, V, tmax=tmax)
    dr = pkg.binding.Dropout(1, 0.5, 77, 3) if drop else None
    ctx = make(pkg, *dims)
    try:
        assert ctx.param_count == lo["_total"]
        assert ctx.segments() == (lo["_seg0"], lo["_seg1"], lo["_seg2"])
        ctx.set_params(p)
        loss = ctx.ae_step(tok, dr)
        g = ctx.get_grads()
    finally:
        ctx.close()
    want = ref.forward(dims, p.astype(np.float64), tok, dr=dr, train=True)
    el = abs(loss - want["loss"]) / abs(want["loss"])
    eg = seg_errors(lo, g, want["grads"])
    record("ae_" + name, {"loss_rel": el, "grad_rel_max": max(eg.values()), "worst": max(eg, key=eg.get)})
    assert el < TOL_LOSS, (loss, want["loss"])
    assert max(eg.values()) < TOL_GRAD, eg


def test_ae_evaluate_loss_and_greedy_samples(pkg):
    dims = B, D, V, E, R, L = (6, 5, 13, 8, 8, 2)
    rng = np.random.default_rng(5)
    lo = ref.layout(*dims)
    p = rng.uniform(-0.6, 0.6, lo["_total"]).astype(np.float32)  # wide weights: decisive argmaxes
    tok = tokens(rng, B, D, V, tmax=4)
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ev_loss, samples = ctx.ae_evaluate(tok, samples=True)
        tr_loss = ctx.ae_step(tok, None)
        n_loss, _ = ctx.ae_evaluate(tok[:4])
    finally:
        ctx.close()
    assert ev_loss == tr_loss
    want = ref.greedy(dims, p.astype(np.float64), tok)
    assert np.array_equal(samples, want), (samples, want)
    assert samples.min() >= 1 and samples.max() <= V + 1
    sub = ref.forward(dims, p.astype(np.float64), tok, train=False, want_grads=False, nvalid=4)
    assert abs(n_loss - sub["loss"]) / sub["loss"] < TOL_LOSS


def test_adam_update_matches_numpy_mirror(pkg):
    dims = (4, 4, 11, 8, 8, 1)
    rng = np.random.default_rng(9)
    lo = ref.layout(*dims)
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        mirror = ref.Adam(lo["_total"])
        x = p.copy()
        for it in range(3):
            tok = tokens(rng, *dims[:3])
            ctx.ae_step(tok, None)
            g = ctx.get_grads()
            # a large lr makes the update count non-trivial; the clamp (1e-3) and the weight decay (1e-2) both act
            norm, count = ctx.adam_update(2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3, stats=True)
            x, wnorm, wcount = mirror.update(x, g, 2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3)
            got = ctx.get_params()
            err = float(np.abs(got - x).max())
            record(f"ae_adam_step{it}", {"max_abs": err, "count": count, "count_ref": wcount})
            assert err < 1e-6, err
            assert abs(norm - wnorm) / wnorm < 1e-6
            assert abs(count - wcount) <= max(2, wcount // 1000)  # |lr g| vs 0.01 |x| ties at f32 rounding
            x = got  # continue from the device's values
    finally:
        ctx.close()


def test_adam_update_on_a_vqa_context(pkg, orc):
    d = orc.make_dims(arch=1, B=8, T=5, V=20, E=8, R=8, L=1, I=8, C=8, A=8)
    gd = pkg.binding.Dims(*[getattr(d, n) for n, _ in d._fields_])
    ctx = pkg.binding.Context(gd, 0)
    try:
        params = orc.synth_params(d)
        tok, lens, img, lab = orc.synth_batch(d, full_length=False)
        ctx.set_params(params)
        ctx.step(tok, lens, img, lab, None)
        g = ctx.get_grads()
        x, _, _ = ref.Adam(params.size).update(params, g, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
        ctx.adam_update(1e-3, 0.9, 0.999, 1e-8, 0.0, 0.0)
        assert float(np.abs(ctx.get_params() - x).max()) < 1e-6
    finally:
        ctx.close()


def test_ae_step_is_deterministic(pkg):
    dims = (16, 6, 40, 16, 16, 2)
    rng = np.random.default_rng(3)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"]).astype(np.float32)
    tok = tokens(rng, *dims[:3])
    out = []
    for _ in range(2):
        ctx = make(pkg, *dims)
        try:
            ctx.set_params(p)
            loss = ctx.ae_step(tok, pkg.binding.Dropout(1, 0.5, 5, 1))
            out.append((loss, ctx.get_grads()))
        finally:
            ctx.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1])


def test_vqa_entry_points_refuse_an_ae_context(pkg):
    B, D = 4, 5
    ctx = make(pkg, B, D, 9, 8, 8, 1)
    E = pkg.binding.NvqaError
    try:
        tok = np.ones((B, D), np.int32)
        with pytest.raises(E, match="auto-encoder"):
            ctx.step(tok, np.full(B, D, np.int32), np.zeros((B, 0), np.float32), np.ones(B, np.int32))
        with pytest.raises(E, match="auto-encoder"):
            ctx.evaluate(tok, np.full(B, D, np.int32), np.zeros((B, 0), np.float32))
        with pytest.raises(E, match="auto-encoder"):
            ctx.forward(tok, np.full(B, D, np.int32), np.zeros((B, 0), np.float32))
        with pytest.raises(E, match="auto-encoder"):
            ctx.set_fusion(1)
        with pytest.raises(E, match="auto-encoder"):
            ctx.set_ref_quirks(1)
        with pytest.raises(E, match="auto-encoder"):
            ctx.set_precision(1)
        with pytest.raises(E, match="auto-encoder"):
            ctx.dataset_load(tok, None, np.ones(B, np.int32), np.ones(B, np.int32), np.zeros((1, 4), np.float32))
        with pytest.raises(E, match="auto-encoder"):
            ctx.step_indices(np.zeros(B, np.int64))
        with pytest.raises(E, match="auto-encoder"):
            ctx.comm_init(0, 1, bytes(128))
        ctx.set_precision(0)
        with pytest.raises(E):
            ctx.ae_step(np.zeros((B, D), np.int32))  # an all-null batch has no tmax
        # ... and the context still works
        ctx.init_params(1)
        loss = ctx.ae_step(np.array([[1, 2, 0, 0, 0]] * B, np.int32))
        assert np.isfinite(loss)
        ctx.rmsprop_update(1e-3, 0.8, 1e-8, 1e-6, 0.1)
        assert np.all(np.isfinite(ctx.param_norms()))
    finally:
        ctx.close()
    vqa = pkg.binding.Context(pkg.binding.Dims(1, 4, 5, 9, 8, 8, 1, 8, 8, 8), 0)
    try:
        with pytest.raises(E, match="auto-encoder"):
            vqa.ae_step(np.ones((4, 5), np.int32))
    finally:
        vqa.close()


def test_train_export_and_init_vqa_encoder(pkg, tmp_path):
    B, D, V, E, R, L = 32, 6, 30, 16, 16, 2
    rng = np.random.default_rng(1)
    sents = tokens(rng, 96, D, V, lo=2)
    loader = pkg.ae.DataLoader(labels={"train": sents, "val": sents[:40]}, ix_to_word={str(i): f"w{i}" for i in range(1, V + 1)})
    tr = pkg.ae.AETrainer(pkg.binding.Dims(3, B, D, V, E, R, L, 0, 0, 0), learning_rate=1e-2, grad_clip=0.1)
    lines = []
    losses = tr.train(loader, 30, log=lines.append)
    assert lines[0].startswith("iter 1: loss: ") and "# updates:" in lines[0] and "paramsNorm:" in lines[0]
    assert np.mean(losses[-5:]) < np.mean(losses[:5]) - 0.1, losses
    val_loss, preds = tr.eval_split(loader, "val")
    assert np.isfinite(val_loss) and len(preds) >= 40 and "prediction" in preds[0]
    path = str(tmp_path / "ae_vqa.t7")
    tr.export_for_vqa(path)
    x_ae = tr.ctx.get_params()
    seg = tr.ctx.segments()
    tr.ctx.close()

    vt = pkg.trainer.VQATrainer(pkg.binding.Dims(1, 8, D, V, E, R, L, 8, 8, 8))
    try:
        vt.init_from_autoencoder(path)
        xv = vt.ctx.get_params()
        sv = vt.ctx.segments()
        assert sv[0] == seg[0]
        assert np.array_equal(xv[:sv[0]], x_ae[:seg[0]])  # encoder: the same LSTM layers, same order
        w_lk = x_ae[seg[0] + seg[1]:].reshape(V + 1, E)
        assert np.array_equal(xv[sv[0]:sv[0] + E * V].reshape(E, V), w_lk[:V].T)  # embedding = lookup rows 1..V
    finally:
        vt.ctx.close()
