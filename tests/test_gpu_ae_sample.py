"""nvqa_ae_sample / nvqa_ae_sample_rows on the device against the float64 decoders of
tests/ae_sample_ref.py: argmax with log-probabilities, multinomial draws at three temperatures, the beam search, the resident
corpus, every refusal, and the paths that must not notice a decode call.  The inputs and the seeds that make them decisive are
tests/ae_sample_cases.py's; tests/test_ae_sample_ref.py asserts their preconditions without a device.

Measured on the first MI355X run (util.record): mode 1 worst band excess -2.1 delta (every pick at least
2.1 delta inside its float64 bin), equal picks 100 % in all twelve cases; log-probabilities within 0.0013 (mode 0), 0.0096
(mode 1) and 0.0026 (mode 2) of their tolerance."""
import ctypes

import numpy as np
import pytest

import ae_sample_cases as C
import ae_sample_ref as sref
from util import record

pytestmark = pytest.mark.gpu


def make_ctx(pkg, case):
    B, D, V, E, R, L = case["dims"]
    ctx = pkg.binding.Context(pkg.binding.Dims(case["arch"], B, D, V, E, R, L, 0, 0, 0), 0)
    ctx.set_params(case["p"])
    return ctx


@pytest.fixture(scope="module")
def ctx_of(pkg):
    """one context per shape for the whole module; every use sets the case's parameters and the f32 mode"""
    live = {}

    def get(case):
        if case["name"] not in live:
            live[case["name"]] = make_ctx(pkg, case)
        ctx = live[case["name"]]
        ctx.set_params(case["p"])
        ctx.ae_set_precision(0)
        return ctx
    yield get
    for ctx in live.values():
        ctx.close()


def opts_of(pkg, mode, K=1, T=1.0, seed=0, step=0):
    return pkg.binding.SampleOpts(mode, K, T, 0, seed, step)


def p64(case):
    return case["p"].astype(np.float64)


def upto_end(seq, end):
    out = np.zeros_like(seq)
    for b, row in enumerate(seq):
        e = np.nonzero(row == end)[0]
        n = e[0] + 1 if e.size else len(row)
        out[b, :n] = row[:n]
    return out


MAIN = ["w14", "w301", "full", "w14_ae2"]


@pytest.mark.parametrize("name", MAIN)
def test_mode0_is_evaluates_greedy_decode_with_logprobs(pkg, ctx_of, name):
    case = C.make(name)
    ctx = ctx_of(case)
    _, want = ctx.ae_evaluate(case["tok"], samples=True, images=case["img"])
    seq, lp = ctx.ae_sample(case["tok"], None, images=case["img"], logprobs=True)
    assert np.array_equal(seq, want)
    assert np.array_equal(ctx.ae_sample(case["tok"], opts_of(pkg, 0, K=99, T=-1.0), images=case["img"]), want)  # ignored fields
    chk = sref.greedy_check(case["dims"], p64(case), case["tok"], seq, images=case["img"], arch=case["arch"])
    err = np.abs(lp - chk["l"]) / C.lp_tol(chk["z"], seq)
    record("ae_sample_mode0_" + name, {"logprob_x_tol": float(err.max())})
    assert err.max() <= 1, err.max()
    n = case["dims"][0] - 1  # fewer rows than B
    img = None if case["img"] is None else case["img"][:n]
    _, want_n = ctx.ae_evaluate(case["tok"][:n], samples=True, images=img)
    assert np.array_equal(ctx.ae_sample(case["tok"][:n], None, images=img), want_n)
    ctx.ae_set_precision(1)  # the bf16 operand mode: the products are evaluate's, the selection reads f32 logits
    _, want16 = ctx.ae_evaluate(case["tok"], samples=True, images=case["img"])
    seq16, lp16 = ctx.ae_sample(case["tok"], None, images=case["img"], logprobs=True)
    assert np.array_equal(seq16, want16) and np.all(lp16 < 0)


@pytest.mark.parametrize("T", [1.0, 0.7, 1.5])
@pytest.mark.parametrize("name", MAIN)
def test_mode1_picks_lie_in_the_float64_cdf_band(pkg, ctx_of, name, T):
    case = C.make(name)
    B, D = case["dims"][:2]
    seed = C.SAMPLE_SEEDS[(name, T)]
    ctx = ctx_of(case)
    o = opts_of(pkg, 1, T=T, seed=seed, step=0)  # the keys whose draws test_ae_sample_ref.py found decisive
    seq, lp = ctx.ae_sample(case["tok"], o, images=case["img"], logprobs=True)
    u = sref.uniforms(seed, 0, B, D)
    chk = sref.sample_check(case["dims"], p64(case), case["tok"], u, T, seq, images=case["img"], arch=case["arch"])
    d = C.delta(chk["z"], T)
    excess = np.maximum(chk["cdf_lo"] - u, u - chk["cdf_hi"]) / d  # <= 0 inside the float64 bin, <= 1 inside the band
    equal = float((seq == chk["pick"]).mean())
    lerr = np.abs(lp - chk["l"]) / C.lp_tol(chk["z"], seq)
    record("ae_sample_mode1_%s_T%g" % (name, T), {"band_excess_x_delta": float(excess.max()), "equal_picks": equal,
                                                  "logprob_x_tol": float(lerr.max())})
    assert np.all(chk["cdf_lo"] - d <= u) and np.all(u < chk["cdf_hi"] + d), float(excess.max())
    assert equal >= 0.95, equal
    assert lerr.max() <= 1, lerr.max()
    seq2, lp2 = ctx.ae_sample(case["tok"], o, images=case["img"], logprobs=True)
    assert np.array_equal(seq, seq2) and np.array_equal(lp.view(np.int32), lp2.view(np.int32))  # same keys, same bits
    other = ctx.ae_sample(case["tok"], opts_of(pkg, 1, T=T, seed=seed, step=1), images=case["img"])
    assert not np.array_equal(seq, other)
    ctx.ae_set_precision(1)
    a, b = (ctx.ae_sample(case["tok"], o, images=case["img"], logprobs=True) for _ in range(2))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    assert a[0].min() >= 1 and a[0].max() <= case["dims"][2] + 1


BEAMS = sorted(C.BEAM_SEEDS)


@pytest.mark.parametrize("name,K,n", BEAMS, ids=["%s-K%d-n%d" % b for b in BEAMS])
def test_mode2_beam_matches_the_float64_beam(pkg, ctx_of, name, K, n):
    case = C.make(name, C.BEAM_SEEDS[(name, K, n)])
    B, D, V = case["dims"][:3]
    margin, want, wlp, z = C.beam_reference(case, K, n)
    assert margin > 0, "the input must be decisive: the smallest gap exceeds 2 D max _logit_tol"
    ctx = ctx_of(case)
    img = None if case["img"] is None else np.ascontiguousarray(case["img"][:n])
    tok = np.ascontiguousarray(case["tok"][:n])
    # through the raw ABI, into buffers of B rows: the rows behind n must come back untouched
    seq = np.full((B, D), -7, np.int32)
    lp = np.full((B, D), -7.0, np.float32)
    f32p, i32p = ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    ctx._check(ctx.lib.nvqa_ae_sample(ctx._h, n, None if img is None else img.ctypes.data_as(f32p), tok.ctypes.data_as(i32p),
                                      ctypes.byref(opts_of(pkg, 2, K=K)), seq.ctypes.data_as(i32p), lp.ctypes.data_as(f32p)))
    assert np.all(seq[n:] == -7) and np.all(lp[n:] == -7.0)
    seq, lp = seq[:n], lp[:n]
    assert np.array_equal(seq, want), (seq, want)
    err = np.abs(lp - wlp)[seq != 0] / C.lp_tol(z, seq)[seq != 0]
    record("ae_sample_beam_%s_K%d_n%d" % (name, K, n), {"logprob_x_tol": float(err.max()), "gap_margin": margin})
    assert err.max() <= 1, err.max()
    assert np.all(lp[seq == 0] == 0)
    assert n * K <= B
    if K == 1:  # mode 0 up to and including the first END, zeros behind
        greedy = ctx.ae_sample(tok, None, images=img)
        assert np.array_equal(seq, upto_end(greedy, V + 1))
        assert (greedy == V + 1).any()
    again = ctx.ae_sample(tok, opts_of(pkg, 2, K=K), images=img, logprobs=True)
    assert np.array_equal(again[0], seq) and np.array_equal(again[1].view(np.int32), lp.view(np.int32))


def test_sample_rows_equals_sample_on_the_gathered_rows(pkg, ctx_of):
    for name in ("w14", "w14_ae2"):
        case = C.make(name)
        B, D, V = case["dims"][:3]
        rng = np.random.default_rng(8)
        corpus = np.concatenate([case["tok"], C.make(name, 1)["tok"], C.make(name, 2)["tok"]])
        ctx = ctx_of(case)
        ctx.ae_corpus_load(corpus)
        for o, n in ((opts_of(pkg, 1, T=0.9, seed=3, step=2), B), (opts_of(pkg, 1, T=1.2, seed=3, step=2), B - 2),
                     (opts_of(pkg, 2, K=2), B // 2), (opts_of(pkg, 2, K=3), 1), (None, B)):
            rows = rng.integers(0, corpus.shape[0], n)
            a = ctx.ae_sample_rows(rows, o, logprobs=True)
            b = ctx.ae_sample(corpus[rows], o, logprobs=True)  # (AE2: zero image rows, as the resident step feeds)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
        with pytest.raises(pkg.binding.NvqaError, match="outside"):
            ctx.ae_sample_rows([corpus.shape[0]], None)


def _loss_and_grads(pkg, ctx, case):
    loss = ctx.ae_step(case["tok"], pkg.binding.Dropout(1, 0.5, 9, 2), images=case["img"])
    return loss, ctx.get_grads()


def test_refusals_leave_the_context_usable(pkg):
    E = pkg.binding.NvqaError
    b = pkg.binding
    for name in ("w14", "w14_ae2"):
        case = C.make(name)
        B, D, V, Ew, R, L = case["dims"]
        tok, img = case["tok"], case["img"]
        fresh = make_ctx(pkg, case)
        ctx = make_ctx(pkg, case)
        try:
            want = _loss_and_grads(pkg, fresh, case)
            for mode in (-1, 3):
                with pytest.raises(E, match="mode"):
                    ctx.ae_sample(tok, opts_of(pkg, mode), images=img)
            for T in (0.0, -1.0, float("nan"), float("inf")):
                with pytest.raises(E, match="temperature"):
                    ctx.ae_sample(tok, opts_of(pkg, 1, T=T), images=img)
            for K in (0, 9, -2):
                with pytest.raises(E, match="beam_size"):
                    ctx.ae_sample(tok[:1], opts_of(pkg, 2, K=K), images=None if img is None else img[:1])
            with pytest.raises(E, match="exceed B"):
                ctx.ae_sample(tok[:B // 2 + 1], opts_of(pkg, 2, K=2), images=None if img is None else img[:B // 2 + 1])
            with pytest.raises(E, match="outside 1..B"):
                ctx.ae_sample(np.zeros((0, D), np.int32), None)
            with pytest.raises(E, match="outside 1..B"):
                ctx.ae_sample(np.ones((B + 1, D), np.int32), None)
            with pytest.raises(E, match="no corpus"):
                ctx.ae_sample_rows([0], None)
            if case["arch"] == 3:
                with pytest.raises(E, match="images"):
                    ctx.ae_sample(tok, None, images=np.zeros((B, Ew), np.float32))
            got = _loss_and_grads(pkg, ctx, case)
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
        finally:
            fresh.close()
            ctx.close()
    B, D, V, Ew, R, I = 4, 5, 9, 8, 8, 16
    for dims in (b.Dims(b.ARCH_AE2_WP, B, D, V, Ew, R, 1, I, 0, 0), b.Dims(b.ARCH_AE1_WP, B, D, V, Ew, R, 1, I, 2 * R, 0)):
        wp = b.Context(dims, 0)
        try:
            with pytest.raises(E, match="weak-paired"):
                wp.ae_sample(np.ones((B, D), np.int32), None)
            with pytest.raises(E, match="weak-paired"):
                wp.ae_sample_rows([0], opts_of(pkg, 2, K=2))
        finally:
            wp.close()
    vqa = b.Context(b.Dims(1, 4, 5, 9, 8, 8, 1, 8, 8, 8), 0)
    try:
        with pytest.raises(E, match="auto-encoder"):
            vqa.ae_sample(np.ones((4, 5), np.int32), None)
    finally:
        vqa.close()


@pytest.mark.parametrize("bf16", [0, 1])
def test_a_step_after_decoding_is_the_step_without_it(pkg, bf16):
    for name in ("w14", "w14_ae2"):
        case = C.make(name)
        B = case["dims"][0]
        plain, ctx = make_ctx(pkg, case), make_ctx(pkg, case)
        try:
            plain.ae_set_precision(bf16)
            ctx.ae_set_precision(bf16)
            want = _loss_and_grads(pkg, plain, case)
            ev = plain.ae_evaluate(case["tok"], samples=True, images=case["img"])
            ctx.ae_sample(case["tok"], None, images=case["img"])
            ctx.ae_sample(case["tok"], opts_of(pkg, 1, T=0.8, seed=1), images=case["img"])
            n = B // 3
            ctx.ae_sample(case["tok"][:n], opts_of(pkg, 2, K=3), images=None if case["img"] is None else case["img"][:n])
            got = _loss_and_grads(pkg, ctx, case)
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
            ev2 = ctx.ae_evaluate(case["tok"], samples=True, images=case["img"])
            assert ev2[0] == ev[0] and np.array_equal(ev2[1], ev[1])
        finally:
            plain.close()
            ctx.close()


def test_trainer_sample_maps_the_references_options(pkg):
    case = C.make("w14")
    B, D, V, E, R, L = case["dims"]
    b = pkg.binding
    tr = pkg.ae.AETrainer(b.Dims(3, B, D, V, E, R, L, 0, 0, 0))
    try:
        tr.ctx.set_params(case["p"])
        tok = case["tok"]
        assert np.array_equal(tr.sample(tok), tr.ctx.ae_evaluate(tok, samples=True)[1])
        seq, lp = tr.sample(tok, sample_max=0, temperature=0.7, seed=5, logprobs=True)
        want = tr.ctx.ae_sample(tok, b.SampleOpts(1, 1, 0.7, 0, 5, 0), logprobs=True)
        assert np.array_equal(seq, want[0]) and np.array_equal(lp, want[1])
        beam = tr.sample(tok, beam_size=2)  # sample_max = 1 with beam_size > 1: B // 2 sentences per call
        want = np.concatenate([tr.ctx.ae_sample(tok[i:i + B // 2], b.SampleOpts(2, 2, 1.0, 0, 0, 0)) for i in range(0, B, B // 2)])
        assert np.array_equal(beam, want)
        sents = np.concatenate([tok, C.make("w14", 1)["tok"]])
        loader = pkg.ae.DataLoader(labels={"train": sents, "val": sents}, ix_to_word={str(i): f"w{i}" for i in range(1, V + 1)})
        loss0, greedy = tr.eval_split(loader, "val")
        loss1, drawn = tr.eval_split(loader, "val", sample_opts={"sample_max": 0, "temperature": 1.5, "seed": 2})
        loss2, beams = tr.eval_split(loader, "val", sample_opts={"beam_size": 3})
        assert loss0 == loss1 == loss2 and len(greedy) == len(drawn) == len(beams)
        assert [p["prediction"] for p in greedy] != [p["prediction"] for p in drawn]
        tr.load_corpus(loader)
        rows = np.arange(B)
        assert np.array_equal(tr.sample(rows, beam_size=2), tr.sample(loader.corpus()[0][rows], beam_size=2))
    finally:
        tr.ctx.close()
