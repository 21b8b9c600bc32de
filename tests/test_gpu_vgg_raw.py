"""The extractor's raw-image route (nvqa_vgg16_fc7_raw): the fused uint8 front end against nvqa_vgg16_fc7 on the same crop
prepared on the host, bit for bit, in f32 and both bf16 forms; the training-mode head (drop6 / drop7) against the float64
body model of tests/vgg_body_ref.py; the refusals."""
import functools

import numpy as np
import pytest

import vgg_body_ref as vref

pytestmark = pytest.mark.gpu

DIV, HW, S, N = 16, 32, 40, 5
ORIGINS = [(0, 0), (7, 3), (8, 8), (3, 3)]  # (8, 8) is the last valid origin, (3, 3) eval_split's centre


@functools.lru_cache(maxsize=None)
def _weights(orc, div, hw):
    return orc.VggOracle(div, hw).synth_weights()


def _body(pkg, orc, div=DIV, hw=HW, max_batch=N, bf16=False):
    v = pkg.binding.Vgg16(0, div, hw, max_batch=max_batch)
    if bf16:
        v.set_precision(1)
    v.set_weights(_weights(orc, div, hw))
    return v


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_raw_front_end_equals_host_crop_bit_for_bit(pkg, orc, bf16):
    img = vref.raw_images(N, S, 21)
    v = _body(pkg, orc, bf16=bf16)
    try:
        for xoff, yoff in ORIGINS:
            want = v.fc7(vref.host_crop(img, xoff, yoff, HW))
            got = v.fc7_raw(img, xoff, yoff)
            assert (want > 0).mean() > 0.05
            assert np.array_equal(got, want), (xoff, yoff, float(np.abs(got - want).max()))
            off = pkg.binding.Dropout(0, 0.5, 1, 1)  # mode 0 is the evaluate path
            assert np.array_equal(v.fc7_raw(img, xoff, yoff, dropout=off), want)
        # an off-centre window differs from the centre one (the origin is used), and rows are independent of the batch
        assert not np.array_equal(v.fc7_raw(img, 7, 3), v.fc7_raw(img, 3, 7))
        assert np.array_equal(v.fc7_raw(img[1:3], 7, 3), v.fc7_raw(img, 7, 3)[1:3])
        # S == hw: no crop
        same = vref.raw_images(3, HW, 22)
        assert np.array_equal(v.fc7_raw(same, 0, 0), v.fc7(vref.host_crop(same, 0, 0, HW)))
    finally:
        v.close()


def test_raw_front_end_bf16_gfx950_form(pkg, orc):
    """full width: bf16 mode runs its gfx950 form (bf16 activations from conv1_1's epilogue on)"""
    div, hw, n, s = 1, 64, 2, 70
    img = vref.raw_images(n, s, 23)
    v = _body(pkg, orc, div, hw, n, bf16=True)
    try:
        want = v.fc7(vref.host_crop(img, 5, 6, hw))
        assert np.array_equal(v.fc7_raw(img, 5, 6), want)
        dr = pkg.binding.Dropout(1, 0.5, 77, 3)
        got = v.fc7_raw(img, 5, 6, dropout=dr)
        m7 = vref.dropout_mask(dr, vref.SITE_VGG_FC7, n, v.feature_dim)
        assert not np.any(got[m7 == 0]) and np.any(got[m7 > 0])
        assert np.array_equal(got, v.fc7_raw(img, 5, 6, dropout=dr))
    finally:
        v.close()


@pytest.mark.parametrize("seed", [77, 123456789012])
@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
def test_training_mode_head(pkg, orc, seed, bf16):
    """drop6 / drop7 live (p = 0.5).  f32: within 1e-4 of the float64 model's largest feature, the bound test_gpu_vgg.py holds
    the same sums to.  bf16 mode has no float64 yardstick of that size (its operands are rounded): there the masks' structure
    and the f32-before-rounding order are what is checked -- module 38's output is fc7's ReLU times mask 7 exactly."""
    img = vref.raw_images(N, S, 31)
    dr = pkg.binding.Dropout(1, 0.5, seed, 3)
    v = _body(pkg, orc, bf16=bf16)
    try:
        got = v.fc7_raw(img, 7, 3, dropout=dr)
        again = v.fc7_raw(img, 7, 3, dropout=dr)
        other = v.fc7_raw(img, 7, 3, dropout=pkg.binding.Dropout(1, 0.5, seed, 4))
        plain = v.fc7_raw(img, 7, 3)
    finally:
        v.close()
    want, m6, m7 = vref.body_fc7_raw(DIV, HW, _weights(orc, DIV, HW), img, 7, 3, dr)
    for m in (m6, m7):
        assert 0.4 < (m > 0).mean() < 0.6
    assert np.array_equal(got, again)
    assert not np.array_equal(got, other) and not np.array_equal(got, plain)
    assert not np.any(got[m7 == 0]), "module 38's output must be exactly zero where drop7's mask is"
    assert np.any(got[m7 > 0]) and (want > 0).mean() > 0.02
    if not bf16:
        err = np.abs(got - want).max() / np.abs(want).max()
        print("training-mode head: rel-max err", err)
        assert err < 1e-4, err


def test_refusals_leave_the_extractor_usable(pkg, orc, monkeypatch):
    b = pkg.binding
    img = vref.raw_images(N, S, 41)
    v = b.Vgg16(0, DIV, HW, max_batch=N)
    with pytest.raises(b.NvqaError, match="set_weights"):
        v.fc7_raw(img, 0, 0)                                   # no weights loaded
    v.set_weights(_weights(orc, DIV, HW))
    want = v.fc7_raw(img, 7, 3)
    bad = [
        (vref.raw_images(N, HW - 8, 1), 0, 0, None),           # S < hw
        (img, -1, 0, None), (img, 0, -1, None),                # an origin outside 0..S-hw
        (img, S - HW + 1, 0, None), (img, 0, S - HW + 1, None),
        (img[:0], 0, 0, None),                                 # n outside 1..max_batch
        (vref.raw_images(N + 1, S, 2), 0, 0, None),
        (img, 0, 0, b.Dropout(1, 1.0, 1, 1)),                  # p outside [0, 1)
        (img, 0, 0, b.Dropout(1, -0.25, 1, 1)),
        (img, 0, 0, b.Dropout(1, float("nan"), 1, 1)),
    ]
    for x, xoff, yoff, dr in bad:
        with pytest.raises(b.NvqaError):
            v.fc7_raw(x, xoff, yoff, dropout=dr)
        assert np.array_equal(v.fc7_raw(img, 7, 3), want)
    with pytest.raises(ValueError):
        v.fc7_raw(img.astype(np.float32), 0, 0)                # the binding converts nothing silently
    v.close()
    # n above the extractor's chunk size: the raw route runs one pass
    monkeypatch.setenv("NVQA_VGG_CHUNK", "3")
    v = b.Vgg16(0, DIV, HW, max_batch=N)
    v.set_weights(_weights(orc, DIV, HW))
    try:
        with pytest.raises(b.NvqaError, match="chunk"):
            v.fc7_raw(img, 7, 3)
        assert np.array_equal(v.fc7_raw(img[:3], 7, 3), want[:3])
    finally:
        v.close()
