"""Image-first-token text auto-encoder (NVQA_ARCH_AE2), CPU side: the header's layout, the tmax rule with the image and
START steps, d(images) of the float64 yardstick, AETrainer's arch2 defaults and eval_split stop rule, and the export table
against VQATrainer.init_from_autoencoder's arch2 checks."""
import os
import subprocess

import numpy as np
import pytest

import ae2_ref_torch as ref2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_layout_of_ae2_matches_the_reference_order(tmp_path):
    """include/nvqa_layout.h with arch NVQA_ARCH_AE2: [encoder | decoder | lookup] as AutoEncoder.lua:86-107, the
    same offsets as NVQA_ARCH_AE1 of the same dims"""
    src = tmp_path / "lo.c"
    src.write_text(r'''
#include <stdio.h>
#include "nvqa.h"
#include "nvqa_layout.h"
int main(void) {
    for (int L = 1; L <= 2; ++L) {
        nvqa_dims d = {NVQA_ARCH_AE2, 3, 5, 11, 8, 12, L, 0, 0, 0};
        nvqa_layout lo;
        if (nvqa_layout_init(&d, &lo)) return 1;
        printf("%zu %zu %zu %zu %zu %zu %zu", lo.total, lo.seg[0], lo.seg[1], lo.seg[2], lo.w_proj, lo.b_proj, lo.w_lk);
        for (int l = 0; l < L; ++l) printf(" %zu %zu %zu %zu", lo.w_i2h[l], lo.w_h2h[l], lo.d_w_i2h[l], lo.d_w_h2h[l]);
        d.arch = NVQA_ARCH_AE1;
        nvqa_layout l1;
        if (nvqa_layout_init(&d, &l1) || l1.total != lo.total || l1.w_lk != lo.w_lk || l1.w_proj != lo.w_proj) return 2;
        printf("\n");
    }
    return 0;
}
''')
    exe = tmp_path / "lo"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).strip().split("\n")
    for L, line in zip((1, 2), lines):
        v = [int(x) for x in line.split()]
        lo = ref2.layout(3, 5, 11, 8, 12, L)
        assert v[:7] == [lo["_total"], lo["_seg0"], lo["_seg1"], lo["_seg2"], lo["w_proj"][0], lo["b_proj"][0], lo["w_lk"][0]]
        for l in range(L):
            assert v[7 + 4 * l:11 + 4 * l] == [lo[f"enc{l}_w_i2h"][0], lo[f"enc{l}_w_h2h"][0], lo[f"dec{l}_w_i2h"][0],
                                             lo[f"dec{l}_w_h2h"][0]]
        # sizes: LSTM(E -> R) x L per side, Linear(R, V+1), LookupTable(V+1, E)
        lstm = sum(4 * 12 * ((8 if l == 0 else 12) + 12 + 2) for l in range(L))
        assert lo["_seg0"] == lstm and lo["_seg1"] == lstm + 12 * 12 + 12 and lo["_seg2"] == 12 * 8


def test_tmax_rule_with_image_and_start_steps():
    V = 9
    tok = np.array([[3, 4, 0, 0, 0],
                    [7, 0, 0, 0, 0],     # length 1
                    [2, 8, 5, 0, 0]], np.int32)
    assert ref2.tmax_of(tok) == 3 and ref2.encoder_steps(tok) == 5  # image, START, three token columns
    one = np.array([[6, 0, 0], [0, 0, 0]], np.int32)                 # every row at most one word
    assert ref2.encoder_steps(one) == 3
    dims = (3, 5, V, 4, 4, 1)
    p = np.random.default_rng(0).uniform(-0.1, 0.1, ref2.layout(*dims)["_total"])
    out = ref2.forward(dims, p, tok, want_grads=False)
    assert out["tmax"] == 3 and out["logits"].shape == (4, 3, V + 1)  # the decoder: START + tmax tokens
    tg, n = ref2.criterion_targets(tok, V)
    assert out["n"] == n == (2 + 1) + (1 + 1) + (3 + 1)
    assert max(s for s, _ in tg) == 3
    out1 = ref2.forward((2, 3, V, 4, 4, 1), p[:ref2.layout(2, 3, V, 4, 4, 1)["_total"]], one, want_grads=False)
    assert out1["logits"].shape[0] == 2 and out1["n"] == 3  # row 0: word + END; row 1 (all null): END at s = 0


def test_image_gradient_is_the_encoder_step1_input_gradient():
    """on a hand-sized batch the image rows are the encoder's step-1 input x (AutoEncoder.lua:262-264), so dimgs (:405-414)
    is d(loss)/dx there: the model's d(images) equals central differences of the loss in every image entry"""
    dims = B, D, V, E, R, L = (2, 3, 5, 4, 4, 2)
    rng = np.random.default_rng(4)
    p = rng.uniform(-0.5, 0.5, ref2.layout(*dims)["_total"])
    img = rng.uniform(-1, 1, (B, E))
    tok = np.array([[1, 4, 2], [5, 0, 0]], np.int32)
    out = ref2.forward(dims, p, tok, images=img)
    g = out["dimages"]
    assert g.shape == (B, E) and np.abs(g).max() > 1e-4
    h = 1e-6
    for b in range(B):
        for e in range(E):
            up, dn = img.copy(), img.copy()
            up[b, e] += h
            dn[b, e] -= h
            fd = (ref2.forward(dims, p, tok, images=up, want_grads=False)["loss"]
                  - ref2.forward(dims, p, tok, images=dn, want_grads=False)["loss"]) / (2 * h)
            assert abs(fd - g[b, e]) < 1e-7 + 1e-6 * abs(fd), (b, e, fd, g[b, e])
    # the image moves the loss, and zero images (the text script) still receive a gradient
    zero = ref2.forward(dims, p, tok)
    assert zero["loss"] != out["loss"] and np.abs(zero["dimages"]).max() > 0


class _FakeCtx:
    """a parameter vector and its segments, no device"""

    def __init__(self, x, seg):
        self.x, self.seg = np.asarray(x, np.float32).copy(), seg

    def init_params(self, seed, lo=-0.08, hi=0.08):
        self.x = np.random.default_rng(seed).uniform(lo, hi, self.x.size).astype(np.float32)

    def get_params(self):
        return self.x.copy()

    def set_params(self, x):
        self.x = np.asarray(x, np.float32).copy()

    def segments(self):
        return self.seg


def test_ae_trainer_accepts_ae2_with_the_arch2_script_defaults(pkg, monkeypatch):
    made = []

    class Ctx(_FakeCtx):
        def __init__(self, dims, device):
            lo = ref2.layout(dims.B, dims.T, dims.V, dims.E, dims.R, dims.L)
            super().__init__(np.zeros(lo["_total"]), (lo["_seg0"], lo["_seg1"], lo["_seg2"]))
            made.append(dims.arch)

    monkeypatch.setattr(pkg.binding, "Context", Ctx)
    b = pkg.binding
    assert b.ARCH_AE2 == 4
    tr = pkg.ae.AETrainer(b.Dims(b.ARCH_AE2, 4, 5, 9, 8, 8, 1, 0, 0, 0))
    assert made == [4] and tr.learning_rate == 5e-5
    assert pkg.ae.ARCH_DEFAULTS[b.ARCH_AE2]["max_iters"] == 40001
    assert pkg.ae.AETrainer(b.Dims(b.ARCH_AE1, 4, 5, 9, 8, 8, 1, 0, 0, 0)).learning_rate == 1e-5
    assert pkg.ae.AETrainer(b.Dims(b.ARCH_AE2, 4, 5, 9, 8, 8, 1, 0, 0, 0), learning_rate=1e-3).learning_rate == 1e-3


def test_ae2_eval_split_stops_after_val_sentences_use(pkg):
    """001_train_arch2_text_autoencoder.lua:192-195: n += batch_size, stop at n >= val_sentences_use (arch1: only a wrap
    or a positive budget)"""
    calls = []

    class Ctx:
        def ae_evaluate(self, batch, samples=False):
            calls.append(batch.shape[0])
            return 1.0, np.ones_like(batch)

    D, V = 3, 7
    sents = np.ones((20, D), np.int32)
    loader = pkg.ae.DataLoader(labels={"val": sents})
    b = pkg.binding
    tr = pkg.ae.AETrainer.__new__(pkg.ae.AETrainer)
    tr.ctx = Ctx()
    tr.dims = b.Dims(b.ARCH_AE2, 4, D, V, 8, 8, 1, 0, 0, 0)
    loss, preds = tr.eval_split(loader, "val", val_sentences_use=8)
    assert len(calls) == 2 and len(preds) == 8 and loss == 1.0
    calls.clear()
    tr.eval_split(loader, "val", val_sentences_use=-1)  # the reference's loop: one batch
    assert len(calls) == 1
    calls.clear()
    tr.dims = b.Dims(b.ARCH_AE1, 4, D, V, 8, 8, 1, 0, 0, 0)
    tr.eval_split(loader, "val", val_sentences_use=-1)  # arch1: to the wrap (20 rows / 4 = 5 batches, the 6th wraps)
    assert len(calls) == 6


def test_ae2_export_table_feeds_an_arch2_vqa_trainer(pkg, tmp_path):
    """the table export_for_vqa writes on AE2 has lua/convert_ae_arch2.lua's keys and shapes plus the layout mark, and
    init_from_autoencoder on an arch2 VQATrainer (no encoder_perm) places the encoder and lookup_table in its segment 1"""
    B, D, V, E, R, L = 2, 3, 7, 8, 12, 1
    lo = ref2.layout(B, D, V, E, R, L)
    x = np.arange(lo["_total"], dtype=np.float32) * 1e-3
    b = pkg.binding
    tr = pkg.ae.AETrainer.__new__(pkg.ae.AETrainer)
    tr.dims, tr.ctx = b.Dims(b.ARCH_AE2, B, D, V, E, R, L, 0, 0, 0), _FakeCtx(x, (lo["_seg0"], lo["_seg1"], lo["_seg2"]))
    path = str(tmp_path / "ae2.t7")
    tr.export_for_vqa(path)
    t = pkg.t7.load(path)
    assert set(t) == {"encoder", "lookup_table", "layout"} and t["layout"] == pkg.t7.LAYOUT_MARK
    lk = np.asarray(t["lookup_table"])
    assert lk.shape == (V + 1, E) and np.array_equal(lk.ravel(), x[lo["w_lk"][0]:])
    assert np.array_equal(np.asarray(t["encoder"]), x[:lo["_seg0"]])

    # an arch2 VQA model of the same V, E, R, L (include/nvqa_layout.h): [W_p, b_p | LSTM, W_lk | W_o, b_o]
    I, A = 16, 4
    s0 = E * I + E
    s1 = lo["_seg0"] + (V + 1) * E
    s2 = A * R + A
    vt = pkg.trainer.VQATrainer.__new__(pkg.trainer.VQATrainer)
    vt.dims, vt.seed = b.Dims(b.ARCH2, 8, D, V, E, R, L, I, 0, A), 123
    vt.ctx = _FakeCtx(np.zeros(s0 + s1 + s2), (s0, s1, s2))
    vt.init_from_autoencoder(path)
    xv = vt.ctx.get_params()
    assert np.array_equal(xv[s0:s0 + lo["_seg0"]], x[:lo["_seg0"]])
    assert np.array_equal(xv[s0 + lo["_seg0"]:s0 + s1], x[lo["w_lk"][0]:])
    # the AE1 export is unchanged: it still writes the arch1 converter's keys
    tr.dims = b.Dims(b.ARCH_AE1, B, D, V, E, R, L, 0, 0, 0)
    tr.export_for_vqa(path)
    assert set(pkg.t7.load(path)) == {"lookup", "encoder", "layout"}


def test_ae_trainer_still_rejects_vqa_archs(pkg):
    with pytest.raises(ValueError):
        pkg.ae.AETrainer(pkg.binding.Dims(2, 2, 3, 4, 4, 4, 1, 4, 0, 4))
