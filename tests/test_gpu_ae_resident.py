"""The resident corpus of the text auto-encoders (nvqa_ae_corpus_load / nvqa_ae_step_rows / nvqa_ae_evaluate_rows) on the device.

The yardstick is nvqa_ae_step on the gathered rows: the resident path runs the same kernels on a lookup index that the device
builds, entry for entry the host's, so loss, gradients and the parameters after the Adam update must be np.array_equal.  Two of
the cases are also held against the float64 models of tests/ae_ref_torch.py / ae2_ref_torch.py under the existing bounds
(TOL_LOSS = 1e-6, TOL_GRAD = 2e-5), so that the pair of paths cannot be wrong together.

Each case's corpus is 3 B + 5 rows: the case's own batch (tests/ae_tile_cases.py, tests/test_gpu_ae.py) followed by rows drawn
the same way.  A run is three steps whose batches have tmax = D, then a batch capped below D, then D again (stale bins of the
longer chain must not survive), named by row ids that include row 0, row N - 1, repeats and descending order."""
import functools
import zlib

import numpy as np
import pytest

import ae_ref_torch
import ae_tile_cases as cases
import test_gpu_ae as tga
from util import record

pytestmark = pytest.mark.gpu

TOL_LOSS, TOL_GRAD = tga.TOL_LOSS, tga.TOL_GRAD
ADAM = (2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3)  # a large rate, the clamp and the weight decay all act

FULL_VOCAB = next(c for c in tga.CASES if c[0] == "full_vocab")
assert FULL_VOCAB[1] == (4, 5, 14773, 16, 16, 1)

# name -> (arch, tile case or None, dropout)
RUNS = {
    "b70_v3_drop": (3, "b70_v3_drop", True),           # three real tokens, hundreds of rows each; partial last chunks; 0 -> 1 into token 1
    "b264_v1100_drop": (3, "b264_v1100_drop", True),   # more bins than one workgroup's threads, two row blocks per chain step
    "b136_l2_drop": (3, "b136_l2_drop", True),
    "ae2_b200_null_img": (4, "ae2_b200_null_img", False),      # AE2: the image step's rows are not in the index
    "ae2_b136_l2_drop_zero_img": (4, "ae2_b136_l2_drop_img", True),  # its dims and tokens with the text script's zero images
    "full_vocab": (3, None, False),                    # 14 774 bins, almost all empty
}


@functools.lru_cache(maxsize=None)
def setup(name):
    """(arch, dims, params, corpus [3B + 5 x D], three row-id batches, dropout on?) -- read-only, shared"""
    arch, tile, drop = RUNS[name]
    rng = np.random.default_rng(zlib.crc32(("resident_" + name).encode()))
    if tile:
        dims = cases.BY_NAME[tile].dims[:6]
        x = cases.inputs(tile)
        p, tok = x["p"], x["tok"]
        B, D, V = dims[:3]
        extra = cases.tokens(rng, 2 * B + 5, D, V, D)
    else:
        dims = FULL_VOCAB[1]
        B, D, V = dims[:3]
        r0 = np.random.default_rng(zlib.crc32(b"full_vocab"))
        p = r0.uniform(-0.08, 0.08, ae_ref_torch.layout(*dims)["_total"]).astype(np.float32)
        tok = tga.tokens(r0, B, D, V, tmax=D)
        extra = tga.tokens(rng, 2 * B + 5, D, V)
    corpus = np.concatenate([tok, extra]).astype(np.int32)
    N = corpus.shape[0]
    assert N == 3 * B + 5
    lens = (corpus != 0).sum(axis=1)
    short = np.flatnonzero(lens < D)
    assert lens[0] == D and short.size > 0
    r1 = np.concatenate([[0, N - 1], rng.integers(0, N, B - 2)])              # row 0 (full length), row N - 1
    r2 = np.sort(rng.choice(short, B))[::-1].copy()                            # capped below D; descending, repeats
    r3 = np.sort(rng.integers(0, N, B))[::-1].copy()
    r3[:2], r3[-1] = N - 1, 0                                                  # N - 1 twice, down to row 0
    batches = [r.astype(np.int64) for r in (r1, r2, r3)]
    tm = [ae_ref_torch.tmax_of(corpus[r]) for r in batches]
    assert tm[0] == D and tm[1] < D and tm[2] == D, tm
    for a in (p, corpus, *batches):
        a.setflags(write=False)
    return arch, dims, p, corpus, batches, drop


def make(pkg, arch, dims):
    B, D, V, E, R, L = dims
    return pkg.binding.Context(pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0), 0)


def run(pkg, name, modes, bf16=False, want_loss=True, grads=True):
    """steps over the case's batches (cycled), step i fed by modes[i] ('rows' / 'host'), Adam in between;
    returns [(loss, grads, params)] per step, or with want_loss=False the final (get_loss(), params) alone"""
    arch, dims, p, corpus, batches, drop = setup(name)
    ctx = make(pkg, arch, dims)
    out = []
    try:
        ctx.set_params(p)
        if bf16:
            ctx.ae_set_precision(1)
        ctx.ae_corpus_load(corpus)
        for it, mode in enumerate(modes):
            rows = batches[it % len(batches)]
            dr = pkg.binding.Dropout(1, 0.5, 77, it + 1) if drop else None
            if mode == "rows":
                loss = ctx.ae_step_rows(rows, dr, want_loss=want_loss)
            else:
                loss = ctx.ae_step(corpus[rows], dr, want_loss=want_loss)
            if want_loss:
                g = ctx.get_grads() if grads else None
                ctx.adam_update(*ADAM)
                out.append((loss, g, ctx.get_params()))
            else:
                ctx.adam_update(*ADAM)
        if not want_loss:
            return ctx.get_loss(), ctx.get_params()
        assert ctx.ae_step_routes() == {"host": modes.count("host"), "resident": modes.count("rows")}
    finally:
        ctx.close()
    return out


@functools.lru_cache(maxsize=None)
def host_run(pkg, name, steps=3, bf16=False):
    """the yardstick: `steps` host-fed steps (computed once per case, shared)"""
    return run(pkg, name, ["host"] * steps, bf16)


def assert_identical(want, got, tag):
    assert len(want) == len(got)
    for it, (a, b) in enumerate(zip(want, got)):
        assert a[0] == b[0], (tag, it, "loss", a[0], b[0])
        if a[1] is not None and b[1] is not None:
            assert np.array_equal(a[1], b[1]), (tag, it, "gradient", float(np.abs(a[1] - b[1]).max()))
        assert np.array_equal(a[2], b[2]), (tag, it, "parameters after adam_update")


@pytest.mark.parametrize("name", list(RUNS))
def test_step_rows_equals_step_on_the_gathered_rows_bitwise(pkg, name):
    want = host_run(pkg, name)
    assert len({w[0] for w in want}) == 3 and np.isfinite([w[0] for w in want]).all()
    assert_identical(want, run(pkg, name, ["rows"] * 3), name)


def test_step_rows_bf16_bitwise(pkg):
    name = "b136_l2_drop"
    want = host_run(pkg, name, 3, True)
    assert want[0][0] != host_run(pkg, name)[0][0]  # the operand mode is on
    assert_identical(want, run(pkg, name, ["rows"] * 3, bf16=True), "bf16")


@pytest.mark.parametrize("name", ["b264_v1100_drop", "ae2_b200_null_img"])
def test_step_rows_matches_float64_model(pkg, name):
    """rows 0 .. B-1 of the corpus are the tile case's batch: the resident step against the case's float64 model"""
    arch, dims, p, corpus, _, drop = setup(name)
    B = dims[0]
    want = cases.reference(name)
    lo = ae_ref_torch.layout(*dims)
    ctx = make(pkg, arch, dims)
    try:
        ctx.set_params(p)
        ctx.ae_corpus_load(corpus)
        loss = ctx.ae_step_rows(np.arange(B), pkg.binding.Dropout(*cases.DROPOUT) if drop else None)
        g = ctx.get_grads()
    finally:
        ctx.close()
    el = abs(loss - want["loss"]) / abs(want["loss"])
    eg = tga.seg_errors(lo, g, want["grads"])
    worst = max(eg, key=eg.get)
    record("ae_resident_" + name, {"loss_rel": el, "grad_rel_max": eg[worst], "worst": worst})
    print(name, "loss_rel %.3g" % el, "worst %s %.3g" % (worst, eg[worst]))
    assert el < TOL_LOSS, (loss, want["loss"])
    assert eg[worst] < TOL_GRAD, eg


def test_mixing_both_routes_on_one_context(pkg):
    name = "b70_v3_drop"
    want = host_run(pkg, name, 4)
    assert_identical(want, run(pkg, name, ["rows", "host", "rows", "host"]), "mixed")
    assert_identical(want, run(pkg, name, ["host", "rows", "rows", "host"]), "mixed2")


@pytest.mark.parametrize("name", ["b70_v3_drop", "ae2_b200_null_img"])
def test_evaluate_rows(pkg, name):
    arch, dims, p, corpus, batches, drop = setup(name)
    B = dims[0]
    rows = batches[2]
    ctx = make(pkg, arch, dims)
    try:
        ctx.set_params(p)
        ctx.ae_corpus_load(corpus)
        for n in (B - 3, B):
            want_loss, want_s = ctx.ae_evaluate(corpus[rows[:n]], samples=True)
            got_loss, got_s = ctx.ae_evaluate_rows(rows[:n], samples=True)
            assert got_loss == want_loss and np.array_equal(got_s, want_s), n
            assert ctx.ae_evaluate_rows(rows[:n])[0] == want_loss
        short = ctx.ae_evaluate_rows(batches[1][:5])[0]   # tmax below D, rows 5 .. B-1 zero
        assert short == ctx.ae_evaluate(corpus[batches[1][:5]])[0]
        # a step behind the short evaluation: the rows past n were zero, the step sees all B again
        dr = pkg.binding.Dropout(1, 0.5, 77, 1) if drop else None
        loss = ctx.ae_step_rows(batches[0], dr)
        g = ctx.get_grads()
        assert ctx.ae_step_routes() == {"host": 0, "resident": 1}  # evaluations are not training steps
    finally:
        ctx.close()
    want = host_run(pkg, name)[0]
    assert loss == want[0] and np.array_equal(g, want[1])


def test_enqueue_only_steps(pkg):
    """want_loss=False: five steps and updates are only enqueued; what they leave behind is the blocking run's"""
    name = "b264_v1100_drop"
    blocking = run(pkg, name, ["rows"] * 5, grads=False)
    loss, params = run(pkg, name, ["rows"] * 5, want_loss=False)
    assert loss == blocking[-1][0]
    assert np.array_equal(params, blocking[-1][2])
    assert_identical(host_run(pkg, name), blocking[:3], "blocking")


def test_errors_name_their_cause_and_leave_the_context_usable(pkg):
    name = "b70_v3_drop"
    arch, dims, p, corpus, batches, drop = setup(name)
    B, D, V = dims[:3]
    N = corpus.shape[0]
    E = pkg.binding.NvqaError
    ctx = make(pkg, arch, dims)
    try:
        ctx.set_params(p)
        with pytest.raises(E, match="no corpus is loaded"):
            ctx.ae_step_rows(batches[0])
        with pytest.raises(E, match="no corpus is loaded"):
            ctx.ae_evaluate_rows(batches[0])
        ctx.ae_corpus_load(corpus)
        for bad in (-1, N):
            rows = batches[0].copy()
            rows[7] = bad
            with pytest.raises(E, match=r"rows\[7\] = %d outside 0\.\.%d" % (bad, N - 1)):
                ctx.ae_step_rows(rows)
            with pytest.raises(E, match=r"rows\[7\]"):
                ctx.ae_evaluate_rows(rows)
        for n in (0, B + 1):
            with pytest.raises(E, match=r"outside 1\.\.B"):
                ctx.ae_evaluate_rows(np.zeros(n, np.int64))
        for bad in (V + 1, -1):  # a bad load names the place and leaves the old corpus in place
            other = np.ones((9, D), np.int32)
            other[4, 2] = bad
            with pytest.raises(E, match=r"token %d at \(row 4, column 2\) outside 0\.\.%d" % (bad, V)):
                ctx.ae_corpus_load(other)
            assert ctx.ae_evaluate_rows(batches[2])[0] == ctx.ae_evaluate(corpus[batches[2]])[0]  # row N - 1 is still there
        # an all-null batch: a corpus with a null row, stepped on that row alone
        nulls = np.concatenate([corpus, np.zeros((1, D), np.int32)])
        ctx.ae_corpus_load(nulls)
        with pytest.raises(E, match="every row is null"):
            ctx.ae_step_rows(np.full(B, N, np.int64))
        with pytest.raises(E, match="every row is null"):
            ctx.ae_evaluate_rows(np.full(3, N, np.int64))
        assert ctx.ae_step_routes() == {"host": 0, "resident": 0}
        # ... and the context still steps correctly, on the corpus that replaced the first
        dr = pkg.binding.Dropout(1, 0.5, 77, 1)
        loss = ctx.ae_step_rows(batches[0], dr)
        g = ctx.get_grads()
    finally:
        ctx.close()
    want = host_run(pkg, name)[0]
    assert loss == want[0] and np.array_equal(g, want[1])
    D_ = pkg.binding.Dims
    vqa = pkg.binding.Context(D_(1, 4, 5, 9, 8, 8, 1, 8, 8, 8), 0)
    try:
        with pytest.raises(E, match="not an auto-encoder context"):
            vqa.ae_corpus_load(np.ones((6, 5), np.int32))
        with pytest.raises(E, match="not an auto-encoder context"):
            vqa.ae_step_rows(np.zeros(4, np.int64))
        with pytest.raises(E, match="not an auto-encoder context"):
            vqa.ae_evaluate_rows(np.zeros(4, np.int64))
        with pytest.raises(E, match="NVQA_ARCH_AE1 / NVQA_ARCH_AE2 context expected"):
            vqa.ae_step_routes()
    finally:
        vqa.close()
    for wd in (D_(5, 4, 5, 9, 8, 8, 1, 8, 0, 0), D_(6, 4, 5, 9, 8, 8, 1, 8, 16, 0)):  # AE2_WP, AE1_WP
        wp = pkg.binding.Context(wd, 0)
        try:
            with pytest.raises(E, match="weak-paired"):
                wp.ae_corpus_load(np.ones((6, 5), np.int32))
            with pytest.raises(E, match="weak-paired"):
                wp.ae_step_rows(np.zeros(4, np.int64))
            with pytest.raises(E, match="weak-paired"):
                wp.ae_evaluate_rows(np.zeros(4, np.int64))
            with pytest.raises(E, match="NVQA_ARCH_AE1 / NVQA_ARCH_AE2 context expected"):
                wp.ae_step_routes()
        finally:
            wp.close()


def test_trainer_with_a_resident_corpus(pkg):
    """AETrainer after load_corpus against one without: four iterations (the fourth wraps the 101-row split), eval_split, and
    log_every = 2"""
    B, D, V, E, R, L = 32, 6, 30, 16, 16, 2
    rng = np.random.default_rng(1)
    sents = tga.tokens(rng, 3 * B + 5, D, V, lo=2)
    labels = {"train": sents, "val": sents[:40]}
    words = {str(i): f"w{i}" for i in range(1, V + 1)}
    out = []
    for resident, log_every in ((False, 1), (True, 1), (True, 2)):
        tr = pkg.ae.AETrainer(pkg.binding.Dims(3, B, D, V, E, R, L, 0, 0, 0), learning_rate=1e-2, grad_clip=0.1)
        try:
            loader = pkg.ae.DataLoader(labels=labels, ix_to_word=words)
            if resident:
                tr.load_corpus(loader)
            lines = []
            losses = tr.train(loader, 4, log=lines.append, log_every=log_every)
            assert loader.iterators["train"] == 1  # the fourth batch wrapped
            params = tr.ctx.get_params()
            routes = tr.ctx.ae_step_routes()
            ev = tr.eval_split(loader, "val")
            assert tr.ctx.ae_step_routes() == routes
            assert routes == ({"host": 0, "resident": 4} if resident else {"host": 4, "resident": 0})
            out.append((lines, losses, params, ev))
        finally:
            tr.ctx.close()
    host, res, res2 = out
    assert len(host[0]) == 4 and host[0] == res[0] and host[1] == res[1]
    assert np.array_equal(host[2], res[2])
    assert host[3][0] == res[3][0] and host[3][1] == res[3][1] and len(host[3][1]) >= 40
    assert res2[0] == [res[0][1], res[0][3]] and res2[1] == [res[1][1], res[1][3]]
    assert np.array_equal(res2[2], res[2])
