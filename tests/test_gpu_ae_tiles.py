"""The f32 auto-encoder steps past one tile, one slab and one chunk (NVQA_ARCH_AE1, AE2, AE2_WP, AE1_WP): the cases of
tests/ae_tile_cases.py against the float64 model of their arch, checked as the arch's own module checks its small cases and
held to the same bounds; evaluate with a short batch on a multi-tile shape; bit reproducibility of the fixed-order slab and
chunk sums at Z = 13 and 17 chunks; the fused Adam update over 274 k parameters; and k_ae_argmax's ties across lanes, waves
and stride iterations.  tests/test_ae_tile_cases.py holds the CPU side: which boundary each case crosses, and that f32
arithmetic reaches a quarter of these bounds.

Measured on the MI355X (util.record, cases "aetile_*") against the existing modules' bounds
TOL_LOSS = 1e-6 and TOL_GRAD = 2e-5: the worst loss is 1.51e-7 relative (b136_l2_drop), the worst gradient tensor 4.97e-7 of its
largest element (d(f^) of ae1wp_b136_skip; among the parameter tensors 4.20e-7, w_lk of b136_l2_drop; d(images) of
ae2_b136_l2_drop_img 4.84e-7); evaluate with 99 rows 1.0e-8; Adam over 274 k parameters 1.4e-7 absolute, the update counts
(111, 197) equal to the mirror's.  That is 6.6 x and 40 x under the bounds, and level with the f32 CPU evaluation of the same
model (1.13e-7 and 4.65e-7, tests/test_ae_tile_cases.py)."""
import numpy as np
import pytest

import ae_ref_torch
import ae_tile_cases as cases
from util import record

pytestmark = pytest.mark.gpu

# the bounds of tests/test_gpu_ae.py, test_gpu_ae2.py, test_gpu_ae2wp.py and test_gpu_ae1wp.py, unchanged
TOL_LOSS = 1e-6
TOL_GRAD = 2e-5


def rel_err(got, want):
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30))


def make(pkg, case):
    b = pkg.binding
    if case.arch == "ae1wp":
        B, D, V, E, R, I = case.dims
        return b.Context(b.Dims(b.ARCH_AE1_WP, B, D, V, E, R, 1, I, 2 * R, 0), 0)
    B, D, V, E, R, L = case.dims[:6]
    arch = {"ae1": b.ARCH_AE1, "ae2": b.ARCH_AE2, "ae2wp": b.ARCH_AE2_WP}[case.arch]
    return b.Context(b.Dims(arch, B, D, V, E, R, L, case.dims[6] if case.arch == "ae2wp" else 0, 0, 0), 0)


def device_step(pkg, case):
    """one training step of the case in a fresh context: dict(loss, grads, and per arch dimages / dw_p, db_p / dfeats)"""
    x = cases.inputs(case.name)
    lo = cases.layout(case)
    dr = pkg.binding.Dropout(*x["dr"]) if x["dr"] else None
    ctx = make(pkg, case)
    out = {}
    try:
        assert ctx.param_count == lo["_total"]
        assert ctx.segments() == (lo["_seg0"], lo["_seg1"], lo["_seg2"])
        ctx.set_params(x["p"])
        if case.arch == "ae1":
            out["loss"] = ctx.ae_step(x["tok"], dr)
        elif case.arch == "ae2":
            out["loss"], out["dimages"] = ctx.ae_step(x["tok"], dr, images=x["img"], want_dimages=True)
        elif case.arch == "ae2wp":
            ctx.ae_wp_set_projection(x["w"], x["b"])
            out["loss"] = ctx.ae_wp_step(x["f"], x["tok"], enc_tokens=x["et"], dropout=dr)
            out["dw_p"], out["db_p"] = ctx.ae_wp_get_projection_grads()
            w2, b2 = ctx.ae_wp_get_projection()
            assert np.array_equal(w2, x["w"]) and np.array_equal(b2, x["b"])  # the step does not move the projection
        else:
            ctx.ae1_wp_set_lookup(x["wlk"])
            kw = dict(enc_tokens=x["et"], enc_state=x["es"], dropout=dr)
            out["loss"], out["dfeats"] = ctx.ae1_wp_step(x["f"], x["tok"], want_dfeats=True, **kw)
        out["grads"] = ctx.get_grads()
        if case.arch == "ae1wp":
            loss2 = ctx.ae1_wp_step(x["f"], x["tok"], **kw)  # without d(f^): the same step
            assert loss2 == out["loss"] and np.array_equal(ctx.get_grads(), out["grads"])
    finally:
        ctx.close()
    return out


@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_step_matches_float64_model(pkg, case):
    got = device_step(pkg, case)
    want = cases.reference(case.name)
    lo = cases.layout(case)
    g = got["grads"]
    el = abs(got["loss"] - want["loss"]) / abs(want["loss"])
    frozen = "w_lk" if case.arch == "ae2wp" else None
    eg = {k: rel_err(g[o:o + n], want["grads"][o:o + n]) for k, (o, n) in
          ((k, v) for k, v in lo.items() if not k.startswith("_") and k != frozen)}
    if case.arch == "ae2":
        eg["dimages"] = rel_err(got["dimages"], want["dimages"])
    elif case.arch == "ae2wp":
        eg["dw_p"], eg["db_p"] = rel_err(got["dw_p"], want["dw_p"]), rel_err(got["db_p"], want["db_p"])
        o, n = lo["w_lk"]
        assert not np.any(g[o:o + n]), "the frozen lookup table received a gradient"
    elif case.arch == "ae1wp":
        eg["dfeats"] = rel_err(got["dfeats"], want["dfhat"])
        if case.variant == "skip":
            assert not np.any(g[:lo["_seg0"]]), "the skipped encoder received a gradient"
            assert not np.any(want["grads"][:lo["_seg0"]])
        else:
            assert np.abs(g[:lo["_seg0"]]).max() > 0
    worst = max(eg, key=eg.get)
    record("aetile_" + case.name, {"loss_rel": el, "grad_rel_max": eg[worst], "worst": worst})
    print(case.name, "loss_rel %.3g" % el, "worst %s %.3g" % (worst, eg[worst]))
    assert el < TOL_LOSS, (got["loss"], want["loss"])
    assert eg[worst] < TOL_GRAD, (worst, eg[worst], {k: "%.3g" % v for k, v in eg.items()})


@pytest.mark.parametrize("name", ["b136_l2_drop", "ae2_b136_l2_drop_img"])
def test_step_is_bit_reproducible_in_a_fresh_context(pkg, name):
    """the fixed-order slab sums (13 slices) and chunk sums (START: 9 and 17 chunks) give the same bits in two contexts"""
    case = cases.BY_NAME[name]
    a, b = device_step(pkg, case), device_step(pkg, case)
    assert a.keys() == b.keys()
    assert a["loss"] == b["loss"]
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_evaluate_short_batch_on_a_multi_tile_shape(pkg):
    """nvalid = 99 < B = 136: rows 99.. sit in the second and third row tile and carry no loss; and evaluate on the whole batch
    is the training loss of a dropout-free step bit for bit"""
    case = cases.BY_NAME["b136_l2_drop"]
    x = cases.inputs(case.name)
    ctx = make(pkg, case)
    try:
        ctx.set_params(x["p"])
        ev_loss, _ = ctx.ae_evaluate(x["tok"])
        tr_loss = ctx.ae_step(x["tok"], None)
        n_loss, _ = ctx.ae_evaluate(x["tok"][:99])
    finally:
        ctx.close()
    assert ev_loss == tr_loss
    sub = ae_ref_torch.forward(case.dims, x["p"].astype(np.float64), x["tok"], train=False, want_grads=False, nvalid=99)
    assert sub["n"] < cases.reference(case.name)["n"]
    el = abs(n_loss - sub["loss"]) / sub["loss"]
    record("aetile_evaluate_n99", {"loss_rel": el})
    assert el < TOL_LOSS, (n_loss, sub["loss"])


def test_adam_update_at_size_matches_numpy_mirror(pkg):
    """two updates over b200_l1's 274 k parameters (k_adam's per-block statistics over hundreds of blocks), the clamp (1e-3) and the
    weight decay (1e-2) active; the bounds of tests/test_gpu_ae.py's test_adam_update_matches_numpy_mirror"""
    case = cases.BY_NAME["b200_l1"]
    x0 = cases.inputs(case.name)
    n = cases.layout(case)["_total"]
    assert n > 250000
    ctx = make(pkg, case)
    try:
        ctx.set_params(x0["p"])
        ctx.ae_step(x0["tok"], None)
        g = ctx.get_grads()
        mirror = ae_ref_torch.Adam(n)
        x = x0["p"].copy()
        for it in range(2):
            norm, count = ctx.adam_update(2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3, stats=True)
            x, wnorm, wcount = mirror.update(x, g, 2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3)
            got = ctx.get_params()
            err = float(np.abs(got - x).max())
            record(f"aetile_adam_step{it}", {"max_abs": err, "count": count, "count_ref": wcount, "norm_rel": abs(norm - wnorm) / wnorm})
            assert 0 < wcount < n
            assert err < 1e-6, err
            assert abs(norm - wnorm) / wnorm < 1e-6
            assert abs(count - wcount) <= max(2, wcount // 1000)  # |lr g| vs 0.01 |x| ties at f32 rounding
            x = got  # continue from the device's values
    finally:
        ctx.close()


@pytest.mark.parametrize("lo_col,hi_col", cases.TIE_PAIRS, ids=["%d_%d" % p for p in cases.TIE_PAIRS])
def test_greedy_tie_returns_the_lower_index(pkg, lo_col, hi_col):
    """two identical logit columns beat every other one at every step: the first maximum wins, as torch.max on the CPU"""
    B, D, V, E, R, L = cases.TIE_DIMS
    p, tok = cases.tie_inputs(lo_col, hi_col)
    b = pkg.binding
    ctx = b.Context(b.Dims(b.ARCH_AE1, B, D, V, E, R, L, 0, 0, 0), 0)
    try:
        ctx.set_params(p)
        _, samples = ctx.ae_evaluate(tok, samples=True)
    finally:
        ctx.close()
    want = ae_ref_torch.greedy(cases.TIE_DIMS, p.astype(np.float64), tok)
    assert set(np.unique(want)) <= {lo_col + 1, hi_col + 1}  # the pair wins everywhere (the float64 BLAS may pick either)
    want = np.where(want == hi_col + 1, lo_col + 1, want)
    assert np.array_equal(samples, want), (samples, want)
