"""nvqa_ae_step_rows on a context with a communicator (nvqa_ae_comm_init), world > 1 on ONE GPU through the all-reduce
stand-in of tests/test_gpu_ae_dp_shim.py: ncclAllReduce(sum) returns world x send, what `world` ranks holding identical
batches produce, so for a power-of-two world every resident step must end with the loss, the gradient, the clamped gradient,
the updated parameters and the Adam statistics BIT-IDENTICAL to the same resident steps without a communicator.

The resident step does not drain the compute stream, so the order between the previous step's kernels and the count that the
communication stream writes at the start of the next one rests on an event edge alone; NCCL_SHIM_DELAY_US stretches every
exchange past the kernels around it, so a missing edge there, or around any bucket, shows as different bits."""

import numpy as np
import pytest

import ae_ref_torch as ref
import test_gpu_ae_dp_shim as shim

pytestmark = pytest.mark.gpu

shim_env = shim.shim_env
DIMS = shim.SMALL + (2,)


def _run(pkg, arch, world, steps=3):
    B, D, V, E, R, L = DIMS
    rng = np.random.default_rng(29 + arch)
    p = rng.uniform(-0.08, 0.08, ref.layout(*DIMS)["_total"]).astype(np.float32)
    corpus = shim._tokens(rng, 3 * B + 5, D, V)
    N = corpus.shape[0]
    short = np.flatnonzero((corpus != 0).sum(axis=1) < D)
    batches = [np.concatenate([[0, N - 1], rng.integers(0, N, B - 2)]), np.sort(rng.choice(short, B))[::-1], np.arange(N - 1, N - 1 - B, -1)]
    batches[2][-1] = 0  # tmax = D, below D, D again
    ctx = pkg.binding.Context(pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0), 0)
    out = []
    try:
        ctx.set_params(p)
        ctx.ae_corpus_load(corpus)
        if world > 1:
            ctx.ae_comm_init(0, world, ctx.comm_unique_id())
        for it in range(steps):
            dr = pkg.binding.Dropout(1, 0.5, 77, it + 1)
            loss = ctx.ae_step_rows(batches[it], dr, want_loss=it != 1)  # the second step only enqueues
            if loss is None:
                loss = ctx.get_loss()
            assert ctx.get_loss() == loss
            g = ctx.get_grads()
            gc = ctx.get_grads(shim.CLAMP)
            stats = ctx.adam_update(2e-2, 0.8, 0.999, 1e-8, shim.WD, shim.CLAMP, stats=True)
            out.append((loss, g, gc, ctx.get_params(), stats, None))
        assert ctx.ae_step_routes() == {"host": 0, "resident": steps}
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("arch", [3, 4])
def test_resident_steps_with_a_communicator_bitwise(pkg, shim_env, arch):
    base = _run(pkg, arch, 1)
    assert float(np.mean(np.abs(base[0][1]) > shim.CLAMP)) > 0.01, "the test clamp must bite"
    for world in (2, 4):
        shim._assert_identical(base, _run(pkg, arch, world), ("resident", arch, world))


@pytest.mark.parametrize("arch", [3, 4])
def test_back_to_back_resident_steps_with_a_communicator(pkg, shim_env, arch):
    """three steps and updates enqueued without a single read in between: the next step's count is written while the last
    step's kernels may still be running, held apart by the event edge alone"""
    B, D, V, E, R, L = DIMS
    rng = np.random.default_rng(31 + arch)
    p = rng.uniform(-0.08, 0.08, ref.layout(*DIMS)["_total"]).astype(np.float32)
    corpus = shim._tokens(rng, 3 * B + 5, D, V)
    batches = [rng.integers(0, corpus.shape[0], B) for _ in range(3)]
    out = []
    for world in (1, 4):
        ctx = pkg.binding.Context(pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0), 0)
        try:
            ctx.set_params(p)
            ctx.ae_corpus_load(corpus)
            if world > 1:
                ctx.ae_comm_init(0, world, ctx.comm_unique_id())
            for it in range(3):
                ctx.ae_step_rows(batches[it], pkg.binding.Dropout(1, 0.5, 77, it + 1), want_loss=False)
                ctx.adam_update(2e-2, 0.8, 0.999, 1e-8, shim.WD, shim.CLAMP)
            out.append((ctx.get_loss(), ctx.get_grads(), ctx.get_params()))
        finally:
            ctx.close()
    assert out[0][0] == out[1][0]
    assert np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][2], out[1][2])
