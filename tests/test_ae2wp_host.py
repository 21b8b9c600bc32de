"""Weak-paired auto-encoder (NVQA_ARCH_AE2_WP), CPU side: the float64 yardstick of tests/ae2wp_ref_torch.py against finite
differences and against the image-first-token model, the null sentence, WeakPairedAETrainer's draw, loader, log line and
export, and VQATrainer.init_from_autoencoder(..., with_cnn=True)."""
import os
import subprocess

import numpy as np
import pytest

import ae2_ref_torch as ref2
import ae2wp_ref_torch as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(dims, seed, scale=0.5):
    B, D, V, E, R, L, I = dims
    rng = np.random.default_rng(seed)
    p = rng.uniform(-scale, scale, ref.layout(B, D, V, E, R, L)["_total"])
    w = rng.uniform(-scale, scale, (E, I))
    b = rng.uniform(-scale, scale, E)
    f = rng.uniform(0, 1, (B, I))
    return p, w, b, f


def test_model_gradients_match_finite_differences():
    dims = B, D, V, E, R, L, I = (2, 3, 5, 4, 4, 2, 6)
    p, w, b, f = _case(dims, 4)
    tok = np.array([[1, 4, 2], [5, 0, 0]], np.int32)
    et = np.array([[3, 0, 0], [2, 2, 0]], np.int32)
    out = ref.forward(dims, p, w, b, f, tok, enc_tokens=et)
    h = 1e-6

    def loss(pp=p, ww=w, bb=b):
        return ref.forward(dims, pp, ww, bb, f, tok, enc_tokens=et, want_grads=False)["loss"]

    lo = ref.layout(B, D, V, E, R, L)
    rng = np.random.default_rng(0)
    idx = [int(i) for i in rng.choice(lo["w_lk"][0], 12, replace=False)]  # LSTM and vocabulary projection entries
    for i in idx:
        up, dn = p.copy(), p.copy()
        up[i] += h
        dn[i] -= h
        fd = (loss(pp=up) - loss(pp=dn)) / (2 * h)
        assert abs(fd - out["grads"][i]) < 1e-7 + 1e-6 * abs(fd), (i, fd, out["grads"][i])
    for e, k in [(0, 0), (1, 5), (3, 2)]:
        up, dn = w.copy(), w.copy()
        up[e, k] += h
        dn[e, k] -= h
        fd = (loss(ww=up) - loss(ww=dn)) / (2 * h)
        assert abs(fd - out["dw_p"][e, k]) < 1e-7 + 1e-6 * abs(fd)
    for e in range(E):
        up, dn = b.copy(), b.copy()
        up[e] += h
        dn[e] -= h
        fd = (loss(bb=up) - loss(bb=dn)) / (2 * h)
        assert abs(fd - out["db_p"][e]) < 1e-7 + 1e-6 * abs(fd)
    # the frozen lookup: no gradient at all, although the loss depends on it
    o, n = lo["w_lk"]
    assert not np.any(out["grads"][o:o + n])
    # dW_p = dx0^T f^ and db_p = colsum(dx0)
    assert np.allclose(out["dw_p"], out["dx0"].T @ out["fhat"], rtol=1e-12, atol=1e-15)
    assert np.allclose(out["db_p"], out["dx0"].sum(0), rtol=1e-12, atol=1e-15)


def test_null_sentence_runs_two_encoder_steps():
    dims = B, D, V, E, R, L, I = (3, 5, 9, 4, 4, 1, 8)
    p, w, b, f = _case(dims, 1, 0.2)
    tok = np.array([[3, 4, 0, 0, 0], [7, 0, 0, 0, 0], [2, 8, 5, 0, 0]], np.int32)
    assert ref.encoder_steps(None) == 2 and ref.encoder_steps(np.zeros_like(tok)) == 2 and ref.encoder_steps(tok) == 5
    null = ref.forward(dims, p, w, b, f, tok, enc_tokens=None, want_grads=False)
    zero = ref.forward(dims, p, w, b, f, tok, enc_tokens=np.zeros_like(tok), want_grads=False)
    same = ref.forward(dims, p, w, b, f, tok, enc_tokens=tok, want_grads=False)
    assert null["te"] == zero["te"] == 2 and same["te"] == 5
    assert null["loss"] == zero["loss"] != same["loss"]
    assert null["tmax"] == same["tmax"] == 3 and null["n"] == same["n"]  # the decoder and the criterion read tokens


def test_same_tokens_equal_ae2_model_fed_the_projected_row():
    dims = B, D, V, E, R, L, I = (3, 4, 7, 4, 6, 2, 8)
    p, w, b, f = _case(dims, 2)
    tok = np.array([[1, 4, 2, 0], [5, 0, 0, 0], [3, 3, 3, 3]], np.int32)
    out = ref.forward(dims, p, w, b, f, tok, enc_tokens=tok)
    x0 = ref.l2_normalize(f) @ w.T + b
    assert np.allclose(out["x0"], x0, rtol=1e-13, atol=1e-15)
    a2 = ref2.forward((B, D, V, E, R, L), p, tok, images=x0)
    lo = ref.layout(B, D, V, E, R, L)
    o, n = lo["w_lk"]
    g2 = a2["grads"].copy()
    assert np.any(g2[o:o + n])
    g2[o:o + n] = 0.0  # AutoEncoderNull drops the lookup's backward
    assert abs(out["loss"] - a2["loss"]) < 1e-13
    assert np.allclose(out["grads"], g2, rtol=1e-11, atol=1e-15)
    assert np.allclose(out["dx0"], a2["dimages"], rtol=1e-11, atol=1e-15)


def test_l2_normalize_rows_and_padding():
    f = np.array([[3.0, 4.0], [0.0, 2.0], [0.0, 0.0]])
    g = ref.l2_normalize(f, nvalid=2)
    assert np.allclose(g[:2], [[0.6, 0.8], [0.0, 1.0]]) and not np.any(g[2])


def test_header_declares_the_weak_paired_arch_with_ae2_layout(tmp_path):
    src = tmp_path / "lo.c"
    src.write_text(r'''
#include <stdio.h>
#include "nvqa.h"
#include "nvqa_layout.h"
int main(void) {
    nvqa_dims d = {NVQA_ARCH_AE2_WP, 3, 5, 11, 8, 12, 2, 16, 0, 0};
    nvqa_layout lo, l2;
    if (nvqa_layout_init(&d, &lo)) return 1;
    d.arch = NVQA_ARCH_AE2; d.I = 0;
    if (nvqa_layout_init(&d, &l2)) return 2;
    printf("%d %d %zu %zu %zu %zu\n", NVQA_ARCH_AE2_WP, lo.total == l2.total && lo.w_lk == l2.w_lk && lo.seg[0] == l2.seg[0] &&
           lo.seg[1] == l2.seg[1] && lo.w_proj == l2.w_proj && lo.d_w_i2h[1] == l2.d_w_i2h[1], lo.total, lo.seg[0], lo.seg[1], lo.seg[2]);
    return 0;
}
''')
    exe = tmp_path / "lo"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    v = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    lo = ref.layout(3, 5, 11, 8, 12, 2)
    assert v == [5, 1, lo["_total"], lo["_seg0"], lo["_seg1"], lo["_seg2"]]


class _FakeCtx:
    """a parameter vector, its segments and a projection, no device"""

    def __init__(self, x, seg, E=0, I=0):
        self.x, self.seg = np.asarray(x, np.float32).copy(), seg
        self.w, self.b = np.zeros((E, I), np.float32), np.zeros(E, np.float32)
        self.param_count = self.x.size

    def init_params(self, seed, lo=-0.08, hi=0.08):
        self.x = np.random.default_rng(seed).uniform(lo, hi, self.x.size).astype(np.float32)
        self.w = np.random.default_rng(seed + 1).uniform(lo, hi, self.w.shape).astype(np.float32)
        self.b[:] = 0

    def get_params(self):
        return self.x.copy()

    def set_params(self, x):
        self.x = np.asarray(x, np.float32).copy()

    def segments(self):
        return self.seg

    def ae_wp_get_projection(self):
        return self.w.copy(), self.b.copy()


def _trainer(pkg, monkeypatch, B=4, D=5, V=9, E=8, R=8, L=1, I=16, **kw):
    lo = ref.layout(B, D, V, E, R, L)

    class Ctx(_FakeCtx):
        def __init__(self, dims, device):
            super().__init__(np.zeros(lo["_total"]), (lo["_seg0"], lo["_seg1"], lo["_seg2"]), dims.E, dims.I)

    monkeypatch.setattr(pkg.binding, "Context", Ctx)
    b = pkg.binding
    return pkg.ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2_WP, B, D, V, E, R, L, I, 0, 0), **kw), lo


def test_trainer_defaults_and_deterministic_null_draw(pkg, monkeypatch):
    b = pkg.binding
    assert b.ARCH_AE2_WP == 5
    tr, _ = _trainer(pkg, monkeypatch)
    assert (tr.learning_rate, tr.grad_clip, tr.weight_decay, tr.alpha, tr.beta) == (1e-5, 0.1, 1e-6, 0.8, 0.999)
    assert (tr.cnn_learning_rate, tr.cnn_weight_decay, tr.rand_val, tr.finetune_cnn_after) == (1e-5, 0.0, 0.5, -1)
    assert not tr.finetuning()
    inc, _ = _trainer(pkg, monkeypatch, variant="inc")
    assert inc.learning_rate == 3e-5
    draws = [tr.null_sentence(i) for i in range(1, 401)]
    assert draws == [tr.null_sentence(i) for i in range(1, 401)]       # keyed by (seed, iter) only
    assert 0.4 < np.mean(draws) < 0.6                                    # rand_val = 0.5
    other, _ = _trainer(pkg, monkeypatch, seed=124)
    assert draws != [other.null_sentence(i) for i in range(1, 401)]
    never, _ = _trainer(pkg, monkeypatch, rand_val=0.0)
    assert not any(never.null_sentence(i) for i in range(1, 50))
    with pytest.raises(ValueError):
        pkg.ae.WeakPairedAETrainer(b.Dims(b.ARCH_AE2, 4, 5, 9, 8, 8, 1, 0, 0, 0))


def test_train_step_feeds_the_draw_and_logs_both_counts(pkg, monkeypatch):
    tr, lo = _trainer(pkg, monkeypatch)
    seen = []
    tr.ctx.ae_wp_step = lambda feats, tokens, enc_tokens=None, dropout=None: seen.append(enc_tokens) or 2.5
    tr.ctx.adam_update = lambda *a, **k: (1.25, 7)
    tok = np.ones((4, 5), np.int32)
    for _ in range(6):
        out = tr.train_step(tok, np.ones((4, 16), np.float32))
    for i, et in enumerate(seen, start=1):
        assert (et is None) == tr.null_sentence(i)
    assert out[-1].startswith("iter 6: loss: 2.500 | # updates:    7 | paramsNorm: 1.2500 | # cnn updates: ")
    assert out[3] == 8 + 8 * 16 - np.count_nonzero(tr.ctx.w)  # frozen: the zero gradient counts the zero entries


def test_weak_paired_loader_walks_features_with_the_captions(pkg):
    labels = np.arange(1, 8, dtype=np.int32).reshape(7, 1).repeat(2, 1)
    feats = np.arange(7, dtype=np.float32).reshape(7, 1).repeat(4, 1)
    ld = pkg.ae.WeakPairedDataLoader(labels={"train": labels}, feats={"train": feats})
    for _ in range(5):
        lab, f, bounds = ld.get_batch("train", 3)
        assert np.array_equal(lab[:, 0] - 1, f[:, 0].astype(np.int32))
    with pytest.raises(ValueError):
        pkg.ae.WeakPairedDataLoader(labels={"train": labels}, feats={"train": feats[:5]})


def test_export_table_keys_shapes_and_vqa_init_with_cnn(pkg, monkeypatch, tmp_path):
    B, D, V, E, R, L, I = 4, 5, 9, 8, 8, 1, 16
    tr, lo = _trainer(pkg, monkeypatch, B, D, V, E, R, L, I)
    x = np.arange(lo["_total"], dtype=np.float32) * 1e-3
    tr.ctx.set_params(x)
    tr.ctx.w = np.arange(E * I, dtype=np.float32).reshape(E, I) * 1e-2
    tr.ctx.b = np.arange(E, dtype=np.float32) + 0.5
    path = str(tmp_path / "wp.t7")
    tr.export_for_vqa(path)
    t = pkg.t7.load(path)
    assert set(t) == {"encoder", "lookup_table", "cnn_w", "layout"} and t["layout"] == pkg.t7.LAYOUT_MARK
    assert np.asarray(t["lookup_table"]).shape == (V + 1, E)
    assert np.array_equal(np.asarray(t["lookup_table"]).ravel(), x[lo["w_lk"][0]:])
    assert np.array_equal(np.asarray(t["encoder"]), x[:lo["_seg0"]])
    cw = np.asarray(t["cnn_w"])
    assert cw.shape == (E * I + E,) and np.array_equal(cw[:E * I], tr.ctx.w.ravel()) and np.array_equal(cw[E * I:], tr.ctx.b)

    A = 4
    s0, s1, s2 = E * I + E, lo["_seg0"] + (V + 1) * E, A * R + A
    b = pkg.binding

    def vqa(I_=I, E_=E):
        vt = pkg.trainer.VQATrainer.__new__(pkg.trainer.VQATrainer)
        vt.dims, vt.seed = b.Dims(b.ARCH2, 8, D, V, E_, R, L, I_, 0, A), 123
        vt.ctx = _FakeCtx(np.zeros(E_ * I_ + E_ + s1 + s2), (E_ * I_ + E_, s1, s2))
        return vt

    vt = vqa()
    vt.init_from_autoencoder(path, with_cnn=True)
    xv = vt.ctx.get_params()
    assert np.array_equal(xv[:s0], cw)
    assert np.array_equal(xv[s0:s0 + lo["_seg0"]], x[:lo["_seg0"]])
    assert np.array_equal(xv[s0 + lo["_seg0"]:s0 + s1], x[lo["w_lk"][0]:])
    vt = vqa()
    vt.init_from_autoencoder(path)  # the default leaves cnn_w to the uniform draw
    assert not np.array_equal(vt.ctx.get_params()[:s0], cw)
    with pytest.raises(ValueError, match="cnn_w has"):
        vqa(I_=8).init_from_autoencoder(path, with_cnn=True)
    tr2 = pkg.ae.AETrainer.__new__(pkg.ae.AETrainer)
    tr2.dims, tr2.ctx = b.Dims(b.ARCH_AE2, B, D, V, E, R, L, 0, 0, 0), _FakeCtx(x, (lo["_seg0"], lo["_seg1"], lo["_seg2"]))
    tr2.export_for_vqa(path)  # an AE2 export: no cnn_w
    with pytest.raises(ValueError, match="no cnn_w"):
        vqa().init_from_autoencoder(path, with_cnn=True)


def test_init_from_text_takes_an_ae2_export(pkg, monkeypatch, tmp_path):
    B, D, V, E, R, L, I = 4, 5, 9, 8, 8, 1, 16
    lo = ref.layout(B, D, V, E, R, L)
    x = np.random.default_rng(3).uniform(-1, 1, lo["_total"]).astype(np.float32)
    b = pkg.binding
    ae = pkg.ae.AETrainer.__new__(pkg.ae.AETrainer)
    ae.dims, ae.ctx = b.Dims(b.ARCH_AE2, B, D, V, E, R, L, 0, 0, 0), _FakeCtx(x, (lo["_seg0"], lo["_seg1"], lo["_seg2"]))
    path = str(tmp_path / "text.t7")
    ae.export_params(path)
    tr, _ = _trainer(pkg, monkeypatch, B, D, V, E, R, L, I)
    tr.init_from_text(path)
    assert np.array_equal(tr.ctx.get_params(), x)
    small, _ = _trainer(pkg, monkeypatch, B, D, V, E, R, L, I)
    small.ctx.param_count -= 1
    with pytest.raises(ValueError, match="values"):
        small.init_from_text(path)
