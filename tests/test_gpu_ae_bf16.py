"""The bf16 operand mode of the text auto-encoders on the device (Context.ae_set_precision, NVQA_ARCH_AE1 / NVQA_ARCH_AE2) against
the PyTorch model of tests/ae_bf16_ref_torch.py in f64 arithmetic: loss and every gradient tensor on short, wide and long
cascades, bit-reproducibility, switching the mode off again, evaluate-mode loss and greedy decoding, the trainer, and the
contexts and values the switch refuses.  tests/test_ae_bf16_ref.py holds the reference alone to the same conditions on the CPU.

Measured on the MI355X (util.record keeps every figure; e = L2 distance of a gradient tensor to the reference, dist = the
reference's own bf16-to-f32 distance, self = the reference's f32-arithmetic twin against its f64 version; per case the worst
tensor):
    case                 loss_rel  max-norm  e / dist  e / max(self, 1e-6)
    l1_t2                4.9e-8    1.2e-7    5.2e-5    0.09
    l2_drop_t3           2.2e-8    1.8e-7    5.1e-5    0.03
    l2_drop_t6           9.1e-9    4.4e-4    0.026     102 (w_lk: one flipped rounding against self = 7e-7; not a wide case)
    ae2_img_t3           9.8e-8    1.5e-7    5.6e-5    0.14
    wide_l1_t1           1.1e-7    3.1e-4    0.064     1.04
    wide_l2_t2           2.4e-9    1.6e-4    0.052     1.34
    wide_fullvocab_t3    2.9e-8    3.3e-4    0.049     1.06
    r12_t3               1.6e-7    2.3e-7    7.0e-5    -
The 6 x bound on the wide cases (measured <= 1.34 x) held on the first run and stands as the issue sets it."""
import numpy as np
import pytest

import ae_bf16_cases as cases
import ae_bf16_ref_torch as ref
from util import record

pytestmark = pytest.mark.gpu

TOL_LOSS = 1e-4            # the loss bound of tests/test_gpu_bf16.py
TOL_BF16_SHORT_MAX = 5e-3  # every gradient tensor, relative to its largest entry
TOL_BF16_SHORT_SELF = 6.0  # wide short cascades: e <= 6 x max(self, 1e-6), as tests/test_gpu_bf16.py holds the VQA kernels
TOL_DIST = 0.5             # e <= 0.5 x dist wherever dist > 1e-4 ...
TOL_AWAY = 5e-4            # ... and the result is more than this away from the unrounded model: the mode is on
TOL_DIST_LONG = 0.75       # the long cascade (the project's full-size bf16 bound)


def make(pkg, dims, arch=3):
    B, D, V, E, R, L = dims
    return pkg.binding.Context(pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0), 0)


def gdrop(pkg, dr):
    return None if dr is None else pkg.binding.Dropout(dr.mode, dr.p, dr.seed, dr.step)


def device_step(pkg, case, bf16=1):
    p, tok, img, dr = cases.inputs(case)
    ctx = make(pkg, case.dims, 4 if case.ae2 else 3)
    try:
        ctx.set_params(p)
        ctx.ae_set_precision(bf16)
        loss = ctx.ae_step(tok, gdrop(pkg, dr), images=img)
        return loss, ctx.get_grads()
    finally:
        ctx.close()


def check_case(pkg, case, tol_dist, with_self):
    loss, g = device_step(pkg, case)
    refs = cases.references(case, with_self=with_self)
    want = refs["ref"]
    assert np.isfinite(loss) and np.all(np.isfinite(g))
    e_loss = abs(loss - want["loss"]) / abs(want["loss"])
    e_max = {k: cases.relmax(g[v[0]:v[0] + v[1]], want["grads"][v[0]:v[0] + v[1]]) for k, v in refs["layout"].items()
             if not k.startswith("_") and np.abs(want["grads"][v[0]:v[0] + v[1]]).max() > 0}
    dist = cases.distances(refs, g)
    ratio = {k: v["e"] / max(v["self"], 1e-6) for k, v in dist.items()} if with_self else {}
    record("ae_bf16_" + case.name, dict(loss_rel=float(e_loss), grad_relmax=e_max, e_l2={k: v["e"] for k, v in dist.items()},
                                        self_l2={k: v.get("self") for k, v in dist.items()}, ratio_to_self=ratio,
                                        dist_to_f32={k: v["dist"] for k, v in dist.items()},
                                        e_over_dist={k: v["e"] / v["dist"] for k, v in dist.items()}))
    print(case.name, "loss_rel %.3g" % e_loss, "worst relmax %.3g" % max(e_max.values()),
          "worst e/dist %.3g" % max(v["e"] / v["dist"] for v in dist.values()),
          "worst e/self %.3g" % max(ratio.values()) if ratio else "")
    assert e_loss <= TOL_LOSS, (loss, want["loss"])
    assert max(e_max.values()) <= TOL_BF16_SHORT_MAX, e_max
    assert any(v["dist"] > 1e-4 for v in dist.values())
    for k, v in dist.items():
        if v["dist"] > 1e-4:
            assert v["e"] <= tol_dist * v["dist"], (k, v)
            assert v["to_f32"] > TOL_AWAY, (k, v)
    return dist, ratio


@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_ae_bf16_step_matches_bf16_model(pkg, case):
    """Loss within 1e-4, every gradient tensor within 5e-3 of its largest entry, every weight tensor within 0.5 x its bf16-to-f32
    distance of the reference and away from the unrounded model; on the wide short cascades also within 6 x the reference's own
    f32-vs-f64 distance (floor 1e-6)."""
    dist, ratio = check_case(pkg, case, TOL_DIST, with_self=True)
    if case.wide:
        for k, v in dist.items():
            assert v["e"] <= TOL_BF16_SHORT_SELF * max(v["self"], 1e-6), (k, v, ratio[k])


def test_ae_bf16_width_not_a_multiple_of_8(pkg):
    """R = 12: the projection group cannot read 16-byte pieces of bf16 images and rounds its f32 operands as they are read, like
    the LSTM products; the same contract, the same conditions."""
    check_case(pkg, cases.Case("r12_t3", (6, 5, 23, 8, 12, 1), 3, True, False, False), TOL_DIST, with_self=False)


def test_ae_bf16_long_cascade(pkg):
    """D = 16 at the full vocabulary width, E = R = 512, B = 256: every weight tensor within 0.75 x its bf16-to-f32 distance, the
    loss within 1e-4, everything finite."""
    check_case(pkg, cases.LONG, TOL_DIST_LONG, with_self=False)


def test_ae_bf16_step_is_bit_reproducible(pkg):
    case = cases.CASES[2]
    a, b = device_step(pkg, case), device_step(pkg, case)
    assert a[0] == b[0] and np.array_equal(a[1], b[1])
    p, tok, img, dr = cases.inputs(case)
    ctx = make(pkg, case.dims)
    try:  # ... and on one context, step after step
        ctx.set_params(p)
        ctx.ae_set_precision(1)
        out = [(ctx.ae_step(tok, gdrop(pkg, dr)), ctx.get_grads()) for _ in range(2)]
    finally:
        ctx.close()
    assert out[0][0] == out[1][0] == a[0] and np.array_equal(out[0][1], out[1][1]) and np.array_equal(out[0][1], a[1])


@pytest.mark.parametrize("case", [cases.CASES[1], cases.CASES[3], cases.CASES[5]], ids=lambda c: c.name)
def test_switching_off_gives_back_the_f32_step_bit_for_bit(pkg, case):
    p, tok, img, dr = cases.inputs(case)
    fresh = device_step(pkg, case, bf16=0)
    ctx = make(pkg, case.dims, 4 if case.ae2 else 3)
    try:
        ctx.set_params(p)
        ctx.ae_set_precision(1)
        on = ctx.ae_step(tok, gdrop(pkg, dr), images=img), ctx.get_grads()
        ctx.ae_set_precision(0)
        off = ctx.ae_step(tok, gdrop(pkg, dr), images=img), ctx.get_grads()
    finally:
        ctx.close()
    assert off[0] == fresh[0] and np.array_equal(off[1], fresh[1])
    assert not np.array_equal(on[1], fresh[1])  # the mode was on in between


def test_ae_bf16_evaluate_loss_and_greedy_samples(pkg):
    p, tok = cases.greedy_inputs()
    ctx = make(pkg, cases.GREEDY_DIMS)
    try:
        ctx.set_params(p)
        ctx.ae_set_precision(1)
        ev_loss, samples = ctx.ae_evaluate(tok, samples=True)
        tr_loss = ctx.ae_step(tok, None)
    finally:
        ctx.close()
    assert ev_loss == tr_loss
    want, _ = ref.greedy(cases.GREEDY_DIMS, p, tok)
    assert np.array_equal(samples, want), (samples, want)
    ev = ref.forward(cases.GREEDY_DIMS, p, tok, train=False, want_grads=False)
    assert abs(ev_loss - ev["loss"]) <= TOL_LOSS * abs(ev["loss"])


def test_ae_bf16_trainer_learns(pkg):
    B, D, V, E, R, L = 32, 6, 30, 16, 16, 2
    rng = np.random.default_rng(1)
    lens = rng.integers(2, D + 1, 96)  # the toy loader of tests/test_gpu_ae.py
    sents = np.zeros((96, D), np.int32)
    for b, n in enumerate(lens):
        sents[b, :n] = rng.integers(1, V + 1, n)
    loader = pkg.ae.DataLoader(labels={"train": sents, "val": sents[:40]}, ix_to_word={str(i): f"w{i}" for i in range(1, V + 1)})
    tr = pkg.ae.AETrainer(pkg.binding.Dims(3, B, D, V, E, R, L, 0, 0, 0), learning_rate=1e-2, grad_clip=0.1, bf16=True)
    try:
        losses = tr.train(loader, 30, log=None)
        assert np.mean(losses[-5:]) < np.mean(losses[:5]) - 0.1, losses
        val_loss, preds = tr.eval_split(loader, "val")
        assert np.isfinite(val_loss) and len(preds) >= 40
    finally:
        tr.ctx.close()


def test_ae_set_precision_refusals(pkg):
    E = pkg.binding.NvqaError
    D = pkg.binding.Dims
    for dims in (D(5, 4, 5, 9, 8, 8, 1, 16, 0, 0), D(6, 4, 5, 9, 8, 8, 1, 16, 16, 0)):  # ARCH_AE2_WP, ARCH_AE1_WP
        ctx = pkg.binding.Context(dims, 0)
        try:
            with pytest.raises(E, match="weak-paired"):
                ctx.ae_set_precision(1)
            with pytest.raises(E, match="weak-paired"):
                ctx.ae_set_precision(0)
        finally:
            ctx.close()
    vqa = pkg.binding.Context(D(1, 4, 5, 9, 8, 8, 1, 8, 8, 8), 0)
    try:
        with pytest.raises(E, match="nvqa_set_precision"):
            vqa.ae_set_precision(1)
    finally:
        vqa.close()
    for arch in (3, 4):
        ctx = make(pkg, (4, 5, 9, 8, 8, 1), arch)
        try:
            for bad in (2, -1):
                with pytest.raises(E, match="0 .* or 1"):
                    ctx.ae_set_precision(bad)
            with pytest.raises(E, match="auto-encoder"):
                ctx.set_precision(1)  # the VQA step's switch stays refused here
            with pytest.raises(E, match="auto-encoder"):
                ctx.comm_init(0, 1, bytes(128))
            ctx.ae_set_precision(1)
            ctx.ae_set_precision(0)
            ctx.ae_set_precision(1)
            ctx.init_params(1)
            assert np.isfinite(ctx.ae_step(np.array([[1, 2, 0, 0, 0]] * 4, np.int32)))
        finally:
            ctx.close()
    with pytest.raises(ValueError, match="bf16"):
        pkg.ae.WeakPairedAETrainer(D(5, 4, 5, 9, 8, 8, 1, 16, 0, 0), bf16=True)
    with pytest.raises(ValueError, match="bf16"):
        pkg.ae.WeakPairedAE1Trainer(D(6, 4, 5, 9, 8, 8, 1, 16, 16, 0), bf16=True)
