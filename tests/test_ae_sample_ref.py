"""The float64 decoders of tests/ae_sample_ref.py, pinned without a device: the beam against greedy decoding and against an
exhaustive enumeration, the multinomial pick against its distribution and against greedy decoding at a low temperature, and
the ABI's new struct and symbols."""
import ctypes
import itertools

import numpy as np

import ae2_ref_torch as ref2
import ae_ref_torch as ref
import ae_sample_cases as cases
import ae_sample_ref as sref


def _tokens(rng, B, D, V):
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(rng.integers(1, D + 1, B)):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def _upto_end(seq, end):
    """rows cut behind their first END, zero-padded"""
    out = np.zeros_like(seq)
    for b, row in enumerate(seq):
        e = np.nonzero(row == end)[0]
        n = e[0] + 1 if e.size else len(row)
        out[b, :n] = row[:n]
    return out


def test_beam_of_one_is_greedy_up_to_end():
    for name, seed in (("w14", 163), ("w14_ae2", 19)):  # seeds whose greedy decodes hold END in front of other tokens
        case = cases.make(name, seed)
        dims, arch, tok, img = case["dims"], case["arch"], case["tok"], case["img"]
        V, p = dims[2], case["p"].astype(np.float64)
        want = ref.greedy(dims, p, tok) if arch == 3 else ref2.greedy(dims, p, tok, img)
        seq, lp, *_ = sref.beam(dims, p, tok, 1, images=img, arch=arch)
        assert np.array_equal(seq, _upto_end(want, V + 1))
        assert (want[:, :-1] == V + 1).any() and (want[:, -1] != V + 1).any(), "the case must exercise the cut behind END"
        assert np.all(lp[seq == 0] == 0) and np.all(lp[seq != 0] < 0)


def test_wide_beam_finds_the_best_of_all_enumerated_sequences():
    dims = B, D, V, E, R, L = (1, 3, 3, 4, 4, 1)
    rng = np.random.default_rng(2)
    p = rng.uniform(-1.5, 1.5, ref.layout(*dims)["_total"])
    tok = np.array([[2, 1, 3]], np.int32)
    best, best_seq = -np.inf, None
    seen = set()
    for cand in itertools.product(range(1, V + 2), repeat=D):
        S, cut = sref.sequence_score(dims, p, tok, cand)
        if tuple(cut) not in seen:
            seen.add(tuple(cut))
            if S > best:
                best, best_seq = S, cut
    assert len(seen) == 3 ** 3 + 3 ** 2 + 3 + 1  # sequences that END at position 3 (or not at all), 2, 1, 0
    seq, lp, *_ = sref.beam(dims, p, tok, 64)
    assert list(seq[0][:len(best_seq)]) == best_seq and not seq[0][len(best_seq):].any()
    assert abs(lp[0].sum() - best) < 1e-12


def test_multinomial_picks_follow_the_distribution():
    z = np.log(np.array([0.05, 0.3, 0.02, 0.4, 0.23]))
    N = 20000
    for T in (1.0, 0.5):
        q = np.exp(z / T) / np.exp(z / T).sum()
        counts = np.bincount([sref.multinomial_pick(z, sref.uniform(77, 3, i), T) for i in range(N)], minlength=5)
        sigma = np.sqrt(N * q * (1 - q))
        assert np.all(np.abs(counts - N * q) <= 4 * sigma), (counts, N * q, sigma)
    # the pick is the smallest c with CDF(c) > u: u = CDF(c) exactly belongs to the next bin, u = 0 to the first
    F = sref.cdf(z, 1.0)
    assert sref.multinomial_pick(z, 0.0, 1.0) == 0 and sref.multinomial_pick(z, F[1], 1.0) == 2
    assert sref.multinomial_pick(z, np.nextafter(F[1], 0), 1.0) == 1


def test_low_temperature_reproduces_greedy():
    dims = B, D, V, E, R, L = (6, 5, 13, 8, 8, 2)
    rng = np.random.default_rng(3)
    p = rng.uniform(-0.6, 0.6, ref.layout(*dims)["_total"])  # wide weights: decisive logits
    tok = _tokens(rng, B, D, V)
    u = sref.uniforms(1, 0, B, D)
    want = ref.greedy(dims, p, tok)
    top = np.sort(sref.greedy_check(dims, p, tok, want)["z"], axis=-1)
    assert (top[..., -1] - top[..., -2]).min() > 0.15  # decisive: at T = 0.01 the runner-up weighs exp(-15) at most
    seq, lp = sref.sample(dims, p, tok, u, 0.01)
    assert np.array_equal(seq, want)
    chk = sref.sample_check(dims, p, tok, u, 0.01, seq)
    assert np.array_equal(chk["pick"], seq) and np.allclose(chk["l"], lp, rtol=0, atol=1e-12)
    assert np.all(chk["cdf_lo"] <= u) and np.all(u < chk["cdf_hi"])


def test_sample_opts_struct_and_symbols(pkg):
    b = pkg.binding
    assert ctypes.sizeof(b.SampleOpts) == 32
    assert [n for n, _ in b.SampleOpts._fields_] == ["mode", "beam_size", "temperature", "pad_", "seed", "step"]
    assert b.SampleOpts.seed.offset == 16 and b.SampleOpts.step.offset == 24
    assert {"nvqa_ae_sample", "nvqa_ae_sample_rows"} <= set(b.SYMBOLS)
    assert (b.SAMPLE_ARGMAX, b.SAMPLE_MULTINOMIAL, b.SAMPLE_BEAM) == (0, 1, 2)


def test_the_device_tests_inputs_are_decisive():
    """What tests/test_gpu_ae_sample.py demands of its inputs, checked where no device is needed.  Mode 1: on the float64 model's
    own picks every u keeps more than 2 delta from its bin's boundaries, so a device within the logit tolerance reproduces
    every pick (the 95 % the GPU test asks for is a cap below that).  Mode 2: the beam's smallest gap exceeds 2 D max _logit_tol.
    The beams cover K = 1, 2, 3, 8, n K == B and n K < B, sequences cut by END and sequences of full length."""
    for (name, T), seed in cases.SAMPLE_SEEDS.items():
        margin, seq = cases.sample_margin(cases.make(name), T, seed)
        assert margin > 0, (name, T, margin)
        assert len(np.unique(seq)) >= 5, "the draws must not collapse onto one class"
    fills, ends = set(), set()
    for (name, K, n), seed in cases.BEAM_SEEDS.items():
        case = cases.make(name, seed)
        margin, seq, lp, _ = cases.beam_reference(case, K, n)
        assert margin > 0, (name, K, n, margin)
        fills.add(n * K == case["dims"][0])
        ends.add(bool((seq == case["dims"][2] + 1).any()))
    assert fills == {True, False} and ends == {True, False}
    assert {K for _, K, _ in cases.BEAM_SEEDS} == {1, 2, 3, 8}
