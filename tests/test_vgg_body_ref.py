"""CPU side of the body-in-the-loop route: the float64 body model of tests/vgg_body_ref.py anchored to the direct-convolution
oracle, h5.File.read_rows, the trainers' window draws and WeakPairedImageLoader."""
import os

import numpy as np
import pytest

import vgg_body_ref as vref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Dr:
    def __init__(self, mode, p, seed, step):
        self.mode, self.p, self.seed, self.step = mode, p, seed, step


def test_body_model_agrees_with_the_oracle(orc):
    """No dropout, a host-made crop: the float64 model against the oracle's f32 sums, to 1e-5 of the largest feature."""
    div, hw, S, n = 16, 32, 40, 5
    o = orc.VggOracle(div, hw)
    w = o.synth_weights()
    x = vref.host_crop(vref.raw_images(n, S, 5), 7, 3, hw)
    want = o.fc7(w, x)
    got, m6, m7 = vref.body_fc7(div, hw, w, x)
    assert m6 is None and m7 is None
    assert (want > 0).mean() > 0.05, "degenerate test: almost every feature is clipped by the ReLU"
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()
    # the raw route of the model is the same crop in float64
    got2, _, _ = vref.body_fc7_raw(div, hw, w, vref.raw_images(n, S, 5), 7, 3)
    assert np.abs(got2 - want).max() <= 1e-5 * np.abs(want).max()


def test_body_model_masks():
    """The two sites draw different masks, each keeps about half, and module 38's output is zero where mask 7 is."""
    div, hw, n = 16, 32, 3
    dr = _Dr(1, 0.5, 77, 3)
    m6, m7 = vref.dropout_mask(dr, vref.SITE_VGG_FC6, n, 256), vref.dropout_mask(dr, vref.SITE_VGG_FC7, n, 256)
    assert set(np.unique(m6)) == {0.0, 2.0} and set(np.unique(m7)) == {0.0, 2.0}
    assert 0.4 < (m6 > 0).mean() < 0.6 and 0.4 < (m7 > 0).mean() < 0.6
    assert not np.array_equal(m6, m7)
    assert not np.array_equal(m6, vref.dropout_mask(_Dr(1, 0.5, 77, 4), vref.SITE_VGG_FC6, n, 256))
    rng = np.random.default_rng(0)
    chans, parts, cin = vref.CONV_COUT, [], 3
    for c in chans:
        co = c // div
        parts += [rng.standard_normal(co * cin * 9) * np.sqrt(2.0 / (cin * 9)), rng.uniform(0, 0.1, co)]
        cin = co
    for k in (cin, 256):
        parts += [rng.standard_normal(256 * k) * np.sqrt(2.0 / k), rng.uniform(0, 0.1, 256)]
    f, a6, a7 = vref.body_fc7_raw(div, hw, np.concatenate(parts), vref.raw_images(n, 40, 1), 8, 8, dr)
    assert np.array_equal(a6, m6) and np.array_equal(a7, m7)
    assert not np.any(f[m7 == 0]) and np.any(f[m7 > 0])


# ---- h5.File.read_rows ---------------------------------------------------------------------------------------------
def _ranges(N):
    return [(0, N), (0, 0), (N, N), (0, 1), (N - 1, N), (1, max(1, N - 1)), (N // 3, N // 3 + min(5, N - N // 3))]


def test_read_rows_equals_full_reads_of_written_files(pkg, tmp_path):
    h5 = pkg.h5
    rng = np.random.default_rng(2)
    data = {"images_train": rng.integers(0, 256, (9, 3, 6, 6), dtype=np.uint8),
            "labels_train": rng.integers(0, 50, (9, 7)).astype(np.int32),
            "feats": rng.standard_normal((5, 11)).astype(np.float32),
            "vec": rng.standard_normal(13)}
    path = str(tmp_path / "rows.h5")
    h5.write(path, data)
    with h5.File(path) as f:
        for name, a in data.items():
            full = f.read(name)
            assert np.array_equal(full, a)
            for lo, hi in _ranges(a.shape[0]):
                got = f.read_rows(name, lo, hi)
                assert got.dtype == full.dtype and got.shape == full[lo:hi].shape and np.array_equal(got, full[lo:hi]), (name, lo, hi)
        for lo, hi in [(-1, 2), (3, 2), (0, 10)]:
            with pytest.raises(IndexError):
                f.read_rows("images_train", lo, hi)


def test_read_rows_of_the_golden_variants(pkg):
    """libhdf5's own files: the chunked, filtered, big-endian and never-written datasets of tests/golden/h5/variants.h5"""
    h5 = pkg.h5
    exp = np.load(os.path.join(ROOT, "tests", "golden", "h5", "expected.npz"))
    seen_chunked = 0
    with h5.File(os.path.join(ROOT, "tests", "golden", "h5", "variants.h5")) as f:
        for name in f.keys():
            if "v_" + name not in exp.files:
                continue
            want = exp["v_" + name]
            if want.ndim == 0 or f.shape(name) == ():
                continue
            kind = f._dataset(name).layout[0]
            seen_chunked += kind == "chunked"
            for lo, hi in _ranges(want.shape[0]):
                got = f.read_rows(name, lo, hi)
                assert got.shape == want[lo:hi].shape and np.array_equal(got, want[lo:hi]), (name, kind, lo, hi)
        want = exp["v_many_chunks"]  # rows that straddle chunk borders, and a second call served by the kept chunk index
        assert f._dataset("many_chunks").layout[0] == "chunked"
        step = f._dataset("many_chunks").layout[2][0]
        for lo, hi in [(step - 1, step + 1), (step, 2 * step), (1, want.shape[0] - 1), (want.shape[0] - 2, want.shape[0])]:
            assert np.array_equal(f.read_rows("many_chunks", lo, hi), want[lo:hi]), (lo, hi)
    assert seen_chunked >= 2


# ---- the trainers' window draws and the image loader ----------------------------------------------------------------
def test_window_draws(pkg):
    ae = pkg.ae
    for S, hw in [(40, 32), (256, 224), (33, 32)]:
        seen = set()
        for it in range(1, 400):
            x, y = ae.crop_origin_train(123, it, S, hw)
            assert 0 <= x <= S - hw - 1 and 0 <= y <= S - hw - 1  # torch.random(w - 224) never gives the last origin
            seen.add((x, y))
        assert ae.crop_origin_train(123, 7, S, hw) == ae.crop_origin_train(123, 7, S, hw)
        if S - hw > 1:
            assert {p[0] for p in seen} == set(range(S - hw)) and {p[1] for p in seen} == set(range(S - hw))
            assert len(seen) > (S - hw)  # x and y are drawn separately
            assert ae.crop_origin_train(124, 7, S, hw) != ae.crop_origin_train(123, 7, S, hw) or \
                ae.crop_origin_train(124, 8, S, hw) != ae.crop_origin_train(123, 8, S, hw)
    assert ae.crop_origin_eval(256, 224) == (15, 15)  # math.ceil(32 / 2) = 16, 1-based
    assert ae.crop_origin_eval(40, 32) == (3, 3)
    assert ae.crop_origin_eval(37, 32) == (2, 2)      # ceil(2.5) - 1
    assert ae.crop_origin_eval(33, 32) == (0, 0)
    assert ae.crop_origin_eval(32, 32) == (0, 0) and ae.crop_origin_train(123, 5, 32, 32) == (0, 0)
    with pytest.raises(ValueError):
        ae.crop_origin_eval(31, 32)
    with pytest.raises(ValueError):
        ae.crop_origin_train(1, 1, 31, 32)


def test_image_loader_walks_linearly_and_wraps(pkg, tmp_path):
    ae = pkg.ae
    h5 = pkg.h5
    rng = np.random.default_rng(3)
    N, D, S = 8, 4, 6
    labels = rng.integers(1, 9, (N, D)).astype(np.int32)
    images = rng.integers(0, 256, (N, 3, S, S), dtype=np.uint8)
    path = str(tmp_path / "img.h5")
    h5.write(path, {"images_train": images})
    for src in (images, (path, "images_train")):
        ld = ae.WeakPairedImageLoader({"train": labels}, {"train": src})
        rows = [[0, 1, 2], [3, 4, 5], [6, 7, 0], [0, 1, 2]]  # a wrap restarts at the first rows, as DataLoader does
        for want in rows:
            lab, img, bounds = ld.get_batch("train", 3)
            assert img.dtype == np.uint8 and img.shape == (3, 3, S, S)
            assert np.array_equal(lab, labels[want]) and np.array_equal(img, images[want])
            assert bounds["wrapped"] == (want == [6, 7, 0])
        ld.close()
    with pytest.raises(ValueError):
        ae.WeakPairedImageLoader({"train": labels}, {"train": images[:5]})
    with pytest.raises(ValueError):
        ae.WeakPairedImageLoader({"train": labels}, {"train": images.astype(np.float32)})


class _FakeBody:
    hw, feature_dim = 32, 256


class _FakeCtx:
    """records the in-loop calls of a trainer; no device"""

    def __init__(self):
        self.calls = []

    def ae_wp_step_images(self, body, images, xoff, yoff, tokens, enc_tokens=None, body_dropout=None, dropout=None, want_loss=True):
        self.calls.append(("step", xoff, yoff, enc_tokens is None, body_dropout, dropout))
        return 2.5

    def ae_wp_evaluate_images(self, body, images, xoff, yoff, tokens, enc_tokens=None, body_dropout=None, samples=False):
        self.calls.append(("eval", xoff, yoff, enc_tokens is None, body_dropout, None))
        return 2.0, np.zeros_like(tokens)

    def adam_update(self, *a, **kw):
        return (1.0, 0)

    def ae_wp_get_projection(self):
        return np.ones((2, 2), np.float32), np.zeros(2, np.float32)


def test_trainer_passes_the_window_and_the_body_dropout(pkg):
    """train_step_images: the iteration's random window, body dropout p = 0.5 keyed by (seed, iter); eval_split: the centre,
    no body dropout unless body_dropout_in_eval"""
    ae, b = pkg.ae, pkg.binding
    B, D, V, S = 4, 5, 9, 40
    tr = ae.WeakPairedAETrainer.__new__(ae.WeakPairedAETrainer)
    tr.__dict__.update(dims=b.Dims(b.ARCH_AE2_WP, B, D, V, 8, 8, 1, 256, 0, 0), ctx=_FakeCtx(), body=_FakeBody(), seed=11, iter=1,
                       drop_prob=0.5, rand_val=0.5, optim="adam", learning_rate=1e-3, decay_start=-1, decay_every=1, alpha=0.8,
                       beta=0.999, eps=1e-8, weight_decay=0.0, grad_clip=0.1, finetune_cnn_after=-1, cnn_learning_rate=1e-5,
                       _frozen_cnn_stats=None, body_dropout_in_eval=False)
    rng = np.random.default_rng(4)
    labels = rng.integers(1, V + 1, (B, D)).astype(np.int32)
    loader = ae.WeakPairedImageLoader({"train": labels, "val": labels},
                                      {"train": vref.raw_images(B, S, 1), "val": vref.raw_images(B, S, 2)})
    tr.train(loader, 3, log=None)
    assert tr.iter == 4 and len(tr.ctx.calls) == 3
    for it, (kind, xoff, yoff, null, bdr, dr) in enumerate(tr.ctx.calls, start=1):
        assert kind == "step" and (xoff, yoff) == ae.crop_origin_train(11, it, S, 32)
        assert null == tr.null_sentence(it)
        assert (bdr.mode, bdr.p, bdr.seed, bdr.step) == (1, 0.5, 11, it)
        assert (dr.mode, dr.p, dr.seed, dr.step) == (1, 0.5, 11, it)
    tr.eval_split(loader, "val")
    assert tr.ctx.calls[-1][:5] == ("eval", 3, 3, False, None)
    tr.body_dropout_in_eval = True
    tr.eval_split(loader, "val")
    bdr = tr.ctx.calls[-1][4]
    assert tr.ctx.calls[-1][1:3] == (3, 3) and (bdr.mode, bdr.p, bdr.seed) == (1, 0.5, 11)
    tr.body = None
    with pytest.raises(ValueError):
        tr.train_step_images(labels, vref.raw_images(B, S, 1))
