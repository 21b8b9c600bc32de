"""The text auto-encoders' data-parallel exchange (nvqa_ae_comm_init) with world > 1 on ONE GPU.

NVQA_RCCL_LIB points libnvqa at tests/shim/libnccl_shim.so, whose ncclAllReduce(sum) returns world x send: what `world`
ranks holding identical batches produce.  Their criterion counts are then equal too, so the rank weight n_r world / N the
step forms on the device is exactly 1, and world x g x 1/world is exact for a power-of-two world: a context with a
communicator must end every step with the loss, the gradient, the clamped gradient, the updated parameters and the Adam
statistics BIT-IDENTICAL to a context without one.  A bucket exchanged zero or two times, a missing event edge around the
early W_proj bucket (NCCL_SHIM_DELAY_US stretches every exchange past the kernels around it), a softmax that does not wait
for the count's exchange, or a clamp before the mean would all show."""
import ctypes
import os

import numpy as np
import pytest

import ae_ref_torch as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim", "libnccl_shim.so")

CLAMP = 1e-4   # small enough to bite on > 1 % of the gradient entries of the tiny models (asserted)
# full vocabulary: a non-target entry of d(logits) is p / n ~ (1 / 14774) / 20, and W_proj's gradient sums 20 rows of it times
# |h| <~ 0.1, i.e. ~ 1e-6 and below, while the lookup rows of the ~ 14750 unseen words are exactly zero
CLAMP_FULL_VOCAB = 1e-7
WD = 1e-2


@pytest.fixture()
def shim_env(monkeypatch):
    assert os.path.exists(SHIM), "tests/shim/libnccl_shim.so missing: run __graft_entry__.build()"
    monkeypatch.setenv("NVQA_RCCL_LIB", SHIM)
    monkeypatch.setenv("NCCL_SHIM_DELAY_US", "300")  # every exchange outlasts the kernels around it
    yield ctypes.CDLL(SHIM)


def _tokens(rng, B, D, V):
    lens = rng.integers(1, D + 1, B)
    lens[0] = D
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def _inputs(arch, dims, seed=11):
    B, D, V, E, R, L = dims
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"]).astype(np.float32)
    tok = [_tokens(rng, B, D, V) for _ in range(3)]
    img = rng.standard_normal((B, E)).astype(np.float32) if arch == 4 else None
    return p, tok, img


def _run(pkg, arch, dims, inputs, world, bf16=False, steps=3, optim="adam", clamp=CLAMP):
    B, D, V, E, R, L = dims
    p, toks, img = inputs
    ctx = pkg.binding.Context(pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0), 0)
    out = []
    try:
        ctx.set_params(p)
        if bf16:
            ctx.ae_set_precision(1)
        if world > 1:
            ctx.ae_comm_init(0, world, ctx.comm_unique_id())
        for it in range(steps):
            dr = pkg.binding.Dropout(1, 0.5, 77, it + 1)
            if arch == 4:
                loss, dimg = ctx.ae_step(toks[it], dr, images=img, want_dimages=True)
            else:
                loss, dimg = ctx.ae_step(toks[it], dr), None
            assert ctx.get_loss() == loss
            g = ctx.get_grads()            # unclamped mean
            gc = ctx.get_grads(clamp)      # the clamp on the way out acts on the mean
            if optim == "adam":
                stats = ctx.adam_update(2e-2, 0.8, 0.999, 1e-8, WD, clamp, stats=True)
            else:
                stats = ctx.rmsprop_update(1e-3, 0.8, 1e-8, WD, clamp)
            out.append((loss, g, gc, ctx.get_params(), stats, dimg))
    finally:
        ctx.close()
    return out


def _assert_identical(base, got, tag):
    for it, (a, b) in enumerate(zip(base, got)):
        assert a[0] == b[0], (tag, it, "loss", a[0], b[0])
        assert np.array_equal(a[1], b[1]), (tag, it, "mean gradient")
        assert np.array_equal(a[2], b[2]), (tag, it, "clamped gradient")
        assert np.array_equal(a[3], b[3]), (tag, it, "parameters after the update")
        assert a[4] == b[4], (tag, it, "Adam statistics", a[4], b[4])
        if a[5] is not None:
            assert np.array_equal(a[5], b[5]), (tag, it, "d(images)")


SMALL = (6, 5, 23, 8, 12)
CASES = [  # id, (B, D, V, E, R, L)
    ("l1", SMALL + (1,)),
    ("l2", SMALL + (2,)),
    ("e512_r512", (8, 4, 30, 512, 512, 1)),       # the GEMM configurations the real shape uses
    ("full_vocab", (4, 5, 14773, 16, 16, 1)),     # the full-vocabulary projection bucket, ld16 padding in the bf16 mode
]


@pytest.mark.parametrize("bf16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("name,dims", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("arch", [3, 4])
def test_shim_world_equals_no_communicator_bitwise(pkg, shim_env, arch, name, dims, bf16):
    inputs = _inputs(arch, dims)
    clamp = CLAMP_FULL_VOCAB if name == "full_vocab" else CLAMP
    base = _run(pkg, arch, dims, inputs, 1, bf16, clamp=clamp)
    assert float(np.mean(np.abs(base[0][1]) > clamp)) > 0.01, "the test clamp must bite"
    for world in (2, 4, 8):
        _assert_identical(base, _run(pkg, arch, dims, inputs, world, bf16, clamp=clamp), (arch, name, bf16, world))


def test_shim_world_rmsprop_bitwise(pkg, shim_env):
    dims = SMALL + (2,)
    inputs = _inputs(3, dims)
    base = _run(pkg, 3, dims, inputs, 1, optim="rmsprop")
    _assert_identical(base, _run(pkg, 3, dims, inputs, 4, optim="rmsprop"), "rmsprop")


def test_every_gradient_element_is_exchanged_exactly_once(pkg, shim_env, monkeypatch):
    """world = 3 is not a power of two, so the identity is no longer exact, but the device sum must be 3 x g everywhere to
    rounding (rank weight 3 n / 3 n = 1): bucket coverage independently of the scale (zero or two exchanges give g/3 or 3 g)."""
    monkeypatch.setenv("NCCL_SHIM_DELAY_US", "0")
    for arch, dims in ((3, SMALL + (2,)), (4, SMALL + (2,))):
        inputs = _inputs(arch, dims)
        base = _run(pkg, arch, dims, inputs, 1, steps=1)[0][1]
        got = _run(pkg, arch, dims, inputs, 3, steps=1)[0][1]   # = (3 g) / 3
        assert np.allclose(got, base, rtol=3e-7, atol=0), float(np.abs(got - base).max())


def test_refusals(pkg, shim_env):
    E = pkg.binding.NvqaError
    D = pkg.binding.Dims
    cid = bytes(128)
    vqa = pkg.binding.Context(D(1, 4, 5, 9, 8, 8, 1, 8, 8, 8), 0)
    try:
        with pytest.raises(E, match="nvqa_ae_comm_init"):
            vqa.ae_comm_init(0, 2, cid)
    finally:
        vqa.close()
    for dims in (D(5, 4, 5, 9, 8, 8, 1, 8, 0, 0), D(6, 4, 5, 9, 8, 8, 1, 8, 16, 0)):  # AE2_WP, AE1_WP
        wp = pkg.binding.Context(dims, 0)
        try:
            with pytest.raises(E, match="weak-paired"):
                wp.ae_comm_init(0, 2, cid)
        finally:
            wp.close()
    for arch in (3, 4):
        ctx = pkg.binding.Context(D(arch, 4, 5, 9, 8, 8, 1, 0, 0, 0), 0)
        try:
            for rank, world in ((0, 0), (-1, 2), (2, 2), (3, 2)):
                with pytest.raises(E, match="rank/world"):
                    ctx.ae_comm_init(rank, world, cid)
            with pytest.raises(E, match="auto-encoder"):   # the VQA call stays refused, before and after
                ctx.comm_init(0, 1, cid)
            ctx.ae_comm_init(0, 2, cid)
            with pytest.raises(E, match="already has a communicator"):
                ctx.ae_comm_init(0, 2, cid)
            with pytest.raises(E, match="auto-encoder"):
                ctx.comm_init(0, 1, cid)
            ctx.init_params(1)
            assert np.isfinite(ctx.ae_step(np.array([[1, 2, 0, 0, 0]] * 4, np.int32)))
        finally:
            ctx.close()


@pytest.mark.parametrize("arch", [3, 4])
def test_evaluate_is_rank_local(pkg, shim_env, arch):
    """nvqa_ae_evaluate* issue no collective and apply no rank weight: the same loss and greedy samples with and without a
    communicator, before and after a data-parallel step (which leaves a rank weight behind)."""
    dims = B, D, V, E, R, L = (6, 5, 13, 8, 8, 2)
    rng = np.random.default_rng(5)
    p = rng.uniform(-0.6, 0.6, ref.layout(*dims)["_total"]).astype(np.float32)  # wide weights: decisive argmaxes
    tok = _tokens(rng, B, D, V)
    img = rng.standard_normal((B, E)).astype(np.float32) if arch == 4 else None
    out = []
    for world in (1, 4):
        ctx = pkg.binding.Context(pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0), 0)
        try:
            ctx.set_params(p)
            if world > 1:
                ctx.ae_comm_init(0, world, ctx.comm_unique_id())
            first = ctx.ae_evaluate(tok, samples=True, images=img)
            ctx.ae_step(tok, None, images=img) if arch == 4 else ctx.ae_step(tok, None)
            second = ctx.ae_evaluate(tok[:4], samples=True, images=None if img is None else img[:4])
            assert ctx.get_loss() == second[0]
            out.append((first, second))
        finally:
            ctx.close()
    for a, b in zip(out[0], out[1]):
        assert a[0] == b[0]
        assert np.array_equal(a[1], b[1])
