"""nvqa_optim_update under the text auto-encoders' data-parallel exchange with world > 1 on ONE GPU, after
tests/test_gpu_ae_dp_shim.py's test_shim_world_rmsprop_bitwise: NVQA_RCCL_LIB points libnvqa at tests/shim/libnccl_shim.so,
whose all-reduce returns world x send, so with identical batches on every rank a context with a communicator of world 4 must end
every step with the loss, the mean gradient, the clamped gradient, the updated parameters and the statistics BIT-IDENTICAL to
a context without one.  An update kernel that does not clear the next step's status word (the second step would read the
first one's and skip), or that scales by 1 / world after the clamp (the test clamp bites), fails here."""
import ctypes
import os

import numpy as np
import pytest

import ae_ref_torch as ref
import optim_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "tests", "shim", "libnccl_shim.so")

CLAMP = 1e-4   # small enough to bite on > 1 % of the gradient entries of the tiny models (asserted)
WD = 1e-2
DIMS = (6, 5, 23, 8, 12, 2)


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


def _inputs(dims, seed=11):
    B, D, V, E, R, L = dims
    rng = np.random.default_rng(seed)
    p = rng.uniform(-0.08, 0.08, ref.layout(*dims)["_total"]).astype(np.float32)
    return p, [_tokens(rng, B, D, V) for _ in range(3)]


def _run(pkg, dims, inputs, world, rule, steps=3):
    B, D, V, E, R, L = dims
    p, toks = inputs
    ctx = pkg.binding.Context(pkg.binding.Dims(3, B, D, V, E, R, L, 0, 0, 0), 0)
    out = []
    try:
        ctx.set_params(p)
        if world > 1:
            ctx.ae_comm_init(0, world, ctx.comm_unique_id())
        for it in range(steps):
            loss = ctx.ae_step(toks[it], pkg.binding.Dropout(1, 0.5, 77, it + 1))
            assert ctx.get_loss() == loss
            g = ctx.get_grads()            # unclamped mean
            gc = ctx.get_grads(CLAMP)      # the clamp on the way out acts on the mean
            stats = ctx.optim_update(rule, 1e-3, 0.8, 0.999, 1e-8, WD, CLAMP, stats=True)
            out.append((loss, g, gc, ctx.get_params(), stats))
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("rule", [optim_ref.SGDMOM, optim_ref.ADAGRAD], ids=["sgdmom", "adagrad"])
def test_shim_world_optim_update_bitwise(pkg, shim_env, rule):
    inputs = _inputs(DIMS)
    base = _run(pkg, DIMS, inputs, 1, rule)
    assert float(np.mean(np.abs(base[0][1]) > CLAMP)) > 0.01, "the test clamp must bite"
    assert not np.array_equal(base[0][3], base[1][3]) and not np.array_equal(base[1][3], base[2][3])  # every step applies
    got = _run(pkg, DIMS, inputs, 4, rule)
    for it, (a, b) in enumerate(zip(base, got)):
        assert a[0] == b[0], (it, "loss", a[0], b[0])
        assert np.array_equal(a[1], b[1]), (it, "mean gradient")
        assert np.array_equal(a[2], b[2]), (it, "clamped gradient")
        assert np.array_equal(a[3], b[3]), (it, "parameters after the update")
        assert a[4] == b[4], (it, "statistics", a[4], b[4])
