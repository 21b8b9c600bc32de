"""Image-first-token text auto-encoder on the device (NVQA_ARCH_AE2): loss, every gradient segment and d(images) against the
float64 PyTorch model of tests/ae2_ref_torch.py, the NULL / zero image equivalences, evaluate-mode loss and greedy
decoding, determinism, the entry points an AE2 context refuses, and the pipeline into an arch2 VQATrainer."""
import ctypes
import zlib

import numpy as np
import pytest

import ae2_ref_torch as ref
from util import record

pytestmark = pytest.mark.gpu

# the tolerances of test_gpu_ae.py (same kernels, same sums); d(images) is held to the gradients' bound
TOL_LOSS = 1e-6
TOL_GRAD = 2e-5


def make(pkg, B, D, V, E, R, L, arch=4):
    return pkg.binding.Context(pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0), 0)


def tokens(rng, B, D, V, lo=1, hi=None, tmax=None):
    hi = D if hi is None else hi
    lens = rng.integers(lo, hi + 1, B)
    if tmax is not None:
        lens = np.minimum(lens, tmax)
        lens[0] = tmax
    else:
        lens[0] = D  # a full-length row
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


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


CASES = [
    # name, (B, D, V, E, R, L), dropout, random images, tmax (None: a full-length batch)
    ("l1_full_zero_img", (6, 5, 23, 8, 12, 1), False, False, None),
    ("l2_ragged_img", (7, 6, 19, 8, 8, 2), False, True, 4),
    ("l1_drop_img", (5, 5, 17, 12, 8, 1), True, True, None),
    ("l2_drop_ragged_zero_img", (6, 6, 21, 8, 12, 2), True, False, 3),
    ("e512_r512_img", (8, 4, 30, 512, 512, 1), False, True, None),
    ("full_vocab_img", (4, 5, 14773, 16, 16, 1), False, True, None),
]


@pytest.mark.parametrize("name,dims,drop,with_img,tmax", CASES, ids=[c[0] for c in CASES])
def test_ae2_step_matches_float64_model(pkg, name, dims, drop, with_img, tmax):
    B, D, V, E, R, L = dims
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lo = ref.layout(*dims)
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    tok = tokens(rng, B, D, V, tmax=tmax)
    img = rng.uniform(-1, 1, (B, E)).astype(np.float32) if with_img else None
    dr = pkg.binding.Dropout(1, 0.5, 77, 3) if drop else None
    ctx = make(pkg, *dims)
    try:
        assert ctx.param_count == lo["_total"]
        assert ctx.segments() == (lo["_seg0"], lo["_seg1"], lo["_seg2"])
        ctx.set_params(p)
        loss, dimg = ctx.ae_step(tok, dr, images=img, want_dimages=True)
        g = ctx.get_grads()
    finally:
        ctx.close()
    want = ref.forward(dims, p.astype(np.float64), tok, images=None if img is None else img.astype(np.float64), dr=dr)
    el = abs(loss - want["loss"]) / abs(want["loss"])
    eg = seg_errors(lo, g, want["grads"])
    ei = rel_err(dimg, want["dimages"])
    record("ae2_" + name, {"loss_rel": el, "grad_rel_max": max(eg.values()), "worst": max(eg, key=eg.get), "dimages_rel": ei})
    assert el < TOL_LOSS, (loss, want["loss"])
    assert max(eg.values()) < TOL_GRAD, eg
    assert ei < TOL_GRAD, ei


def test_null_images_equal_zero_images_bit_for_bit(pkg):
    dims = B, D, V, E, R, L = (8, 6, 25, 16, 16, 2)
    rng = np.random.default_rng(11)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"]).astype(np.float32)
    tok = tokens(rng, B, D, V, tmax=5)
    dr = pkg.binding.Dropout(1, 0.5, 9, 2)
    ctx = make(pkg, *dims)
    lib = ctx.lib
    try:
        ctx.set_params(p)
        out = []
        l0 = ctx.ae_step(tok, dr)  # nvqa_ae_step: images = NULL on an AE2 context
        out.append((l0, ctx.get_grads()))
        loss = ctypes.c_float(0)
        ti = np.ascontiguousarray(tok, np.int32)
        rc = lib.nvqa_ae_step_images(ctx._h, None, ti.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(dr),
                                     ctypes.byref(loss), None)
        assert rc == 0
        out.append((float(loss.value), ctx.get_grads()))
        l2 = ctx.ae_step(tok, dr, images=np.zeros((B, E), np.float32))
        out.append((l2, ctx.get_grads()))
    finally:
        ctx.close()
    for loss_k, g_k in out[1:]:
        assert loss_k == out[0][0]
        assert np.array_equal(g_k, out[0][1])


def test_ae2_evaluate_loss_and_greedy_samples(pkg):
    dims = B, D, V, E, R, L = (6, 5, 13, 8, 8, 2)
    rng = np.random.default_rng(5)
    lo = ref.layout(*dims)
    p = rng.uniform(-0.6, 0.6, lo["_total"]).astype(np.float32)  # wide weights: decisive argmaxes
    tok = tokens(rng, B, D, V, tmax=4)
    img = rng.uniform(-1, 1, (B, E)).astype(np.float32)
    ctx = make(pkg, *dims)
    try:
        ctx.set_params(p)
        ev_loss, samples = ctx.ae_evaluate(tok, samples=True, images=img)
        tr_loss = ctx.ae_step(tok, None, images=img)
        z_loss, z_samples = ctx.ae_evaluate(tok, samples=True)
        n_loss, _ = ctx.ae_evaluate(tok[:4], images=img[:4])
    finally:
        ctx.close()
    assert ev_loss == tr_loss
    want = ref.greedy(dims, p.astype(np.float64), tok, images=img.astype(np.float64))
    assert np.array_equal(samples, want), (samples, want)
    assert samples.min() >= 1 and samples.max() <= V + 1
    want0 = ref.greedy(dims, p.astype(np.float64), tok)
    assert np.array_equal(z_samples, want0), (z_samples, want0)
    full = ref.forward(dims, p.astype(np.float64), tok, images=img.astype(np.float64), train=False, want_grads=False)
    zero = ref.forward(dims, p.astype(np.float64), tok, train=False, want_grads=False)
    img4 = np.zeros((B, E))
    img4[:4] = img[:4]
    sub = ref.forward(dims, p.astype(np.float64), tok[:4].tolist() + [[0] * D] * (B - 4), images=img4, train=False,
                      want_grads=False, nvalid=4)
    errs = {"eval": abs(ev_loss - full["loss"]) / full["loss"], "eval_zero": abs(z_loss - zero["loss"]) / zero["loss"],
            "eval_n4": abs(n_loss - sub["loss"]) / sub["loss"]}
    record("ae2_evaluate", errs)
    assert max(errs.values()) < TOL_LOSS, errs


def test_ae2_step_is_deterministic(pkg):
    dims = B, D, V, E, R, L = (16, 6, 40, 16, 16, 2)
    rng = np.random.default_rng(3)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"]).astype(np.float32)
    tok = tokens(rng, B, D, V)
    img = rng.uniform(-1, 1, (B, E)).astype(np.float32)
    out = []
    for _ in range(2):
        ctx = make(pkg, *dims)
        try:
            ctx.set_params(p)
            loss, dimg = ctx.ae_step(tok, pkg.binding.Dropout(1, 0.5, 5, 1), images=img, want_dimages=True)
            out.append((loss, ctx.get_grads(), dimg))
        finally:
            ctx.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1])
    assert np.array_equal(out[0][2], out[1][2])


def test_ae2_refusals_and_ae1_refuses_the_image_calls(pkg):
    B, D, E = 4, 5, 8
    ctx = make(pkg, B, D, 9, E, 8, 1)
    Err = pkg.binding.NvqaError
    try:
        tok = np.ones((B, D), np.int32)
        with pytest.raises(Err, match="auto-encoder"):
            ctx.step(tok, np.full(B, D, np.int32), np.zeros((B, 0), np.float32), np.ones(B, np.int32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.evaluate(tok, np.full(B, D, np.int32), np.zeros((B, 0), np.float32))
        with pytest.raises(Err, match="auto-encoder"):
            ctx.forward(tok, np.full(B, D, np.int32), np.zeros((B, 0), np.float32))
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
        ctx.set_precision(0)
        # ... and the context still works
        ctx.init_params(1)
        loss = ctx.ae_step(np.array([[1, 2, 0, 0, 0]] * B, np.int32), images=np.ones((B, E), np.float32))
        assert np.isfinite(loss)
        ctx.adam_update(1e-3, 0.8, 0.999, 1e-8, 1e-6, 0.1)
        assert np.all(np.isfinite(ctx.param_norms()))
    finally:
        ctx.close()
    ae1 = make(pkg, B, D, 9, E, 8, 1, arch=3)
    try:
        tok = np.array([[1, 2, 0, 0, 0]] * B, np.int32)
        with pytest.raises(Err, match="NVQA_ARCH_AE2"):
            ae1.ae_step(tok, images=np.zeros((B, E), np.float32))
        with pytest.raises(Err, match="NVQA_ARCH_AE2"):
            ae1.ae_step(tok, want_dimages=True)
        with pytest.raises(Err, match="NVQA_ARCH_AE2"):
            ae1.ae_evaluate(tok, images=np.zeros((B, E), np.float32))
        assert np.isfinite(ae1.ae_step(tok))
    finally:
        ae1.close()


def test_ae2_train_export_and_init_arch2_vqa(pkg, tmp_path):
    B, D, V, E, R, L = 32, 6, 30, 16, 16, 1
    rng = np.random.default_rng(1)
    sents = tokens(rng, 96, D, V, lo=2)
    loader = pkg.ae.DataLoader(labels={"train": sents, "val": sents[:40]}, ix_to_word={str(i): f"w{i}" for i in range(1, V + 1)})
    b = pkg.binding
    tr = pkg.ae.AETrainer(b.Dims(b.ARCH_AE2, B, D, V, E, R, L, 0, 0, 0), learning_rate=1e-2, grad_clip=0.1)
    lines = []
    losses = tr.train(loader, 30, log=lines.append)
    assert lines[0].startswith("iter 1: loss: ") and "# updates:" in lines[0] and "paramsNorm:" in lines[0]
    assert np.mean(losses[-5:]) < np.mean(losses[:5]) - 0.1, losses
    val_loss, preds = tr.eval_split(loader, "val", val_sentences_use=64)
    assert np.isfinite(val_loss) and len(preds) == 64 and "prediction" in preds[0]
    path = str(tmp_path / "ae2_vqa.t7")
    tr.export_for_vqa(path)
    x_ae = tr.ctx.get_params()
    seg = tr.ctx.segments()
    tr.ctx.close()

    I, A = 8, 8
    vt = pkg.trainer.VQATrainer(b.Dims(b.ARCH2, 8, D, V, E, R, L, I, 0, A))
    try:
        vt.init_from_autoencoder(path)  # no encoder_perm: the table carries layout = 'nvqa'
        xv = vt.ctx.get_params()
        sv = vt.ctx.segments()
        n_lstm = seg[0]
        assert sv[1] == n_lstm + (V + 1) * E
        assert np.array_equal(xv[sv[0]:sv[0] + n_lstm], x_ae[:n_lstm])                          # encoder
        assert np.array_equal(xv[sv[0] + n_lstm:sv[0] + sv[1]], x_ae[seg[0] + seg[1]:])       # lookup_table
        r2 = np.random.default_rng(2)
        tok = tokens(r2, 8, D, V)
        loss = vt.ctx.step(tok, None, r2.uniform(0, 1, (8, I)).astype(np.float32), r2.integers(1, A + 1, 8).astype(np.int32))
        assert np.isfinite(loss)
    finally:
        vt.ctx.close()
