"""The yardstick of the auto-encoder bf16 operand mode (tests/ae_bf16_ref_torch.py) and the preconditions of
tests/test_gpu_ae_bf16.py, on the CPU: with the rounding off the model is ae_ref_torch / ae2_ref_torch; its rounding is
round-to-nearest-even bit for bit; on every GPU case the reference alone -- its f32-arithmetic twin against its f64 version --
meets the conditions the device is held to; and the greedy-decoding input has decisive argmaxes at every row and step."""
import numpy as np
import pytest
import torch

import ae2_ref_torch
import ae_bf16_cases as cases
import ae_bf16_ref_torch as ref
import ae_ref_torch


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "dropout"])
def test_unrounded_model_is_the_ae1_reference(drop):
    dims = (5, 4, 17, 8, 12, 2)
    rng = np.random.default_rng(1)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"])
    tok = cases.tokens(rng, 5, 4, 17, 3)
    dr = cases.DROPOUT if drop else None
    a = ref.forward(dims, p, tok, dr=dr, rounded=False)
    b = ae_ref_torch.forward(dims, p, tok, dr=dr)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(b["loss"])
    assert np.abs(a["grads"] - b["grads"]).max() <= 1e-12
    ev = ref.forward(dims, p, tok, train=False, want_grads=False, nvalid=3, rounded=False)
    ev0 = ae_ref_torch.forward(dims, p, tok, train=False, want_grads=False, nvalid=3)
    assert abs(ev["loss"] - ev0["loss"]) <= 1e-12 * abs(ev0["loss"])
    assert np.array_equal(ref.greedy(dims, p, tok, rounded=False)[0], ae_ref_torch.greedy(dims, p, tok))


@pytest.mark.parametrize("drop,with_img", [(False, True), (True, True), (False, False)], ids=["image", "image_dropout", "null_image"])
def test_unrounded_model_is_the_ae2_reference(drop, with_img):
    dims = B, D, V, E, R, L = (5, 4, 17, 8, 12, 2)
    rng = np.random.default_rng(2)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"])
    tok = cases.tokens(rng, B, D, V, 3)
    img = rng.uniform(-1, 1, (B, E)) if with_img else None
    dr = cases.DROPOUT if drop else None
    a = ref.forward(dims, p, tok, images=img, ae2=True, dr=dr, rounded=False)
    b = ae2_ref_torch.forward(dims, p, tok, images=img, dr=dr)
    assert abs(a["loss"] - b["loss"]) <= 1e-12 * abs(b["loss"])
    assert np.abs(a["grads"] - b["grads"]).max() <= 1e-12
    assert np.abs(a["dimages"] - b["dimages"]).max() <= 1e-12
    assert np.array_equal(ref.greedy(dims, p, tok, images=img, ae2=True, rounded=False)[0],
                          ae2_ref_torch.greedy(dims, p, tok, images=img))


def rne_bf16(x):
    """f32 -> bf16 -> f32 on the bits: add 0x7fff plus the lowest kept bit, drop the low half"""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def test_rounding_is_nearest_even_bit_for_bit():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.standard_normal(20000).astype(np.float32) * np.float32(10.0) ** rng.integers(-6, 6, 20000).astype(np.float32),
                        np.array([0.0, -0.0, 1.0, -1.0, 0.08, 3.0e-5], np.float32)])
    # ties: the dropped half is exactly 0x8000, above an even and above an odd kept mantissa, both signs; and their neighbours
    hi = rng.integers(0x3000, 0x4800, 4000).astype(np.uint32)
    for low in (0x8000, 0x7FFF, 0x8001):
        bits = (hi << 16) | np.uint32(low)
        x = np.concatenate([x, bits.view(np.float32), (bits | np.uint32(0x80000000)).view(np.float32)])
    assert (((x.view(np.uint32) & 0xFFFF) == 0x8000).sum()) >= 8000
    for dt in (torch.float32, torch.float64):
        got = ref.r(torch.tensor(x).to(dt)).to(torch.float32).numpy()
        assert np.array_equal(got.view(np.uint32), rne_bf16(x).view(np.uint32))


@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_reference_alone_meets_the_gpu_conditions(case):
    """What tests/test_gpu_ae_bf16.py asks of the device, asked of the reference's f32-arithmetic twin: the loss within 1e-4,
    every gradient tensor within 5e-3 of its largest entry, and -- the precondition of the 0.5 x condition -- per weight tensor an
    L2 distance between the twin and the f64 version below 0.25 x the tensor's bf16-to-f32 distance, with the twin more than
    5e-4 away from the unrounded model wherever that distance exceeds 1e-4."""
    refs = cases.references(case)
    r64, r32 = refs["ref"], refs["ref32"]
    assert np.all(np.isfinite(r64["grads"])) and np.isfinite(r64["loss"])
    assert abs(r32["loss"] - r64["loss"]) <= 1e-4 * abs(r64["loss"])
    for k, v in refs["layout"].items():
        if not k.startswith("_"):
            o, n = v
            assert cases.relmax(r32["grads"][o:o + n], r64["grads"][o:o + n]) <= 5e-3 or np.abs(r64["grads"][o:o + n]).max() == 0, k
    dist = cases.distances(refs)
    print(case.name, {k: {m: float("%.3g" % x) for m, x in v.items()} for k, v in dist.items()})
    assert any(v["dist"] > 1e-4 for v in dist.values())
    for k, v in dist.items():
        assert v["self"] < 0.25 * v["dist"], (k, v)
        if v["dist"] > 1e-4:
            assert v["self_to_f32"] > 5e-4, (k, v)


def test_greedy_input_has_decisive_argmaxes():
    """The reference's top-two logit gap exceeds 1e-3 x max |logit| at every row and step of the greedy-decoding input, in f64 and
    in f32 arithmetic: the GPU test may then ask for the reference's samples exactly, no row left out."""
    p, tok = cases.greedy_inputs()
    out = {}
    for dt in (torch.float64, torch.float32):
        samples, logits = ref.greedy(cases.GREEDY_DIMS, p, tok, dtype=dt)
        top = np.sort(logits, axis=2)
        gap = top[:, :, -1] - top[:, :, -2]
        assert gap.min() > 1e-3 * np.abs(logits).max(), (gap.min(), np.abs(logits).max())
        out[dt] = samples
    assert np.array_equal(out[torch.float64], out[torch.float32])
    assert out[torch.float64].min() >= 1 and out[torch.float64].max() <= cases.GREEDY_DIMS[2] + 1
