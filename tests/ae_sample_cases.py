"""Inputs of the decoding tests (test_ae_sample_ref.py checks their preconditions on the CPU, test_gpu_ae_sample.py runs them).

Every weight is uniform(-0.6, 0.6), as in the greedy decoding tests.  On top of that a few classes, END always among them, get a
staggered boost of b_proj.  Without it the preconditions the tests demand of their inputs cannot hold: a near-uniform softmax
over 14 774 classes has bins of 7e-5, far below the band 2 delta ~ 3e-3 that the multinomial test keeps around every bin
boundary, and neighbouring beam candidates closer than the f32 logit tolerance; and END would never be emitted, so nothing
would exercise the cut behind it.  A trained decoder is peaked in the same way."""
import numpy as np

import ae_ref_torch as ref
import ae_sample_ref as sref
from util import _logit_tol

# name: ((B, D, V, E, R, L), arch, boosted classes (negative: END is not among them), the largest boost)
SHAPES = {
    "w14": ((6, 5, 13, 8, 8, 2), 3, 3, 1.5),            # V + 1 below one wave
    "w301": ((7, 6, 300, 8, 12, 1), 3, 10, 14.0),       # V + 1 past one 256-thread pass, odd row count
    "full": ((4, 5, 14773, 16, 16, 1), 3, 12, 22.0),    # the real vocabulary: 58 values a thread and more
    "w14_ae2": ((6, 5, 13, 8, 8, 2), 4, 3, 1.5),        # the first one's image-first-token twin
    "w14_b8": ((8, 5, 13, 8, 8, 2), 3, 3, 1.5),         # rows for a beam of 8
    "w14_b17": ((17, 5, 13, 8, 8, 2), 3, -3, 1.5),       # two beams of 8 and an unused row
    "full_b8": ((8, 5, 14773, 16, 16, 1), 3, 12, 22.0),
    "w301_live": ((7, 6, 300, 8, 12, 1), 3, -10, 14.0),  # END not boosted: the beams run to full length
    "full_live": ((4, 5, 14773, 16, 16, 1), 3, -12, 22.0),
}
STAGGER = 0.1

# mode 1: (shape, temperature) -> the seed of the draws; every u then lies more than 2 delta from a bin boundary of the float64
# model's own decode (found by search, asserted by test_ae_sample_ref.py)
SAMPLE_SEEDS = {("w14", 1.0): 1, ("w14", 0.7): 1, ("w14", 1.5): 1, ("w301", 1.0): 2, ("w301", 0.7): 1, ("w301", 1.5): 1,
                ("full", 1.0): 1, ("full", 0.7): 13, ("full", 1.5): 3, ("w14_ae2", 1.0): 1, ("w14_ae2", 0.7): 1, ("w14_ae2", 1.5): 1}
# mode 2: (shape, K, n) -> the seed of the parameters; the beam's smallest gap then exceeds 2 D max _logit_tol (same)
BEAM_SEEDS = {("w14", 1, 6): 2, ("w14", 2, 3): 52, ("w14", 3, 2): 521, ("w301", 1, 7): 114, ("w301", 2, 3): 154, ("w301", 3, 2): 114,
              ("full", 1, 4): 4, ("full", 2, 2): 22, ("full", 3, 1): 19, ("w14_ae2", 1, 6): 19, ("w14_ae2", 2, 3): 1,
              ("w14_ae2", 3, 1): 0, ("w14_b8", 8, 1): 0, ("full_b8", 8, 1): 12, ("w14_b17", 8, 2): 4, ("w301_live", 3, 2): 291,
              ("w301_live", 2, 3): 181, ("full_live", 2, 2): 117, ("full_live", 3, 1): 141}

_cache = {}


def make(name, seed=0):
    """dict(dims, arch, p [float32], tok [B x D], img [B x E] or None); the same object for the same (name, seed)"""
    if (name, seed) in _cache:
        return _cache[(name, seed)]
    dims, arch, npk, top = SHAPES[name]
    B, D, V, E, R, L = dims
    rng = np.random.default_rng([seed, len(name), V])
    lo = ref.layout(*dims)
    p = rng.uniform(-0.6, 0.6, lo["_total"]).astype(np.float32)
    cls = np.concatenate([[V], rng.choice(V, npk - 1, replace=False)]) if npk > 0 else rng.choice(V, -npk, replace=False)
    npk = abs(npk)
    o = lo["b_proj"][0]
    p[o + cls] += (top - STAGGER * rng.permutation(npk)).astype(np.float32)
    tok = np.zeros((B, D), np.int32)
    lens = rng.integers(1, D + 1, B)
    lens[0] = D - 1  # tmax < D: the decoder runs past the encoder's length
    lens = np.minimum(lens, D - 1)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    img = rng.standard_normal((B, E)).astype(np.float32) if arch == 4 else None
    out = {"name": name, "dims": dims, "arch": arch, "p": p, "tok": tok, "img": img}
    _cache[(name, seed)] = out
    return out


def delta(z_rows, T):
    """the band of the multinomial test: 1/2 max_row(_logit_tol(z64)) / T + 2e-6 per row of z_rows [... x (V+1)].  A perturbation
    of at most eps on the logits moves a softmax CDF by at most eps / 2 (d CDF(c) / d z_j = p_j ([j <= c] - CDF(c)), summed in
    absolute value: 2 CDF (1 - CDF) <= 1/2); eps is the project's f32 logit tolerance; 2e-6 covers the f32 sum of <= 14 774 weights."""
    z = np.asarray(z_rows, np.float64)
    flat = z.reshape(-1, z.shape[-1])
    return (0.5 * _logit_tol(flat).max(axis=1) / T + 2e-6).reshape(z.shape[:-1])


def lp_tol(z_rows, picks):
    """2 _logit_tol at the picked columns (picks 1-based, 0 = none -> 0): l = z - logsumexp(z) carries the error of z twice"""
    z = np.asarray(z_rows, np.float64)
    flat = z.reshape(-1, z.shape[-1])
    pk = np.asarray(picks).reshape(-1)
    t = _logit_tol(flat)[np.arange(flat.shape[0]), np.maximum(pk, 1) - 1]
    return (2 * t * (pk > 0)).reshape(z.shape[:-1])


def sample_margin(case, T, seed, step=0, n=None):
    """The float64 model's own multinomial decode of the case's first n rows under (seed, step): the smallest distance of a u
    from its bin's boundaries minus 2 delta (> 0: no f32 logit error within tolerance can move a pick), and that decode."""
    dims, n = case["dims"], case["dims"][0] if n is None else n
    u = sref.uniforms(seed, step, n, dims[1])
    img = None if case["img"] is None else case["img"][:n]
    p64 = case["p"].astype(np.float64)
    seq, _ = sref.sample(dims, p64, case["tok"][:n], u, T, images=img, arch=case["arch"])
    chk = sref.sample_check(dims, p64, case["tok"][:n], u, T, seq, images=img, arch=case["arch"])
    d = delta(chk["z"], T)
    return float(np.minimum(u - chk["cdf_lo"], chk["cdf_hi"] - u).min() - 2 * d.max()), seq


def beam_reference(case, K, n):
    """sref.beam on the case's first n rows, and its precondition: gap - 2 D max _logit_tol (> 0: no f32 logit error within
    tolerance can change a survivor set or the final winner; a score is a sum of at most D values of l, each off by at most
    2 _logit_tol, and a gap is a difference of two)."""
    dims = case["dims"]
    img = None if case["img"] is None else case["img"][:n]
    seq, lp, gap, zabs, z = sref.beam(dims, case["p"].astype(np.float64), case["tok"][:n], K, images=img, arch=case["arch"])
    return gap - 2 * dims[1] * float(_logit_tol(np.array([[zabs]])).max()), seq, lp, z
