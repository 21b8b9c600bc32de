"""The f32 auto-encoder cases that leave the first tile, slab and chunk, and their inputs, shared by tests/test_ae_tile_cases.py
(CPU: each case crosses the boundaries it is listed for, and f32 arithmetic can meet the tolerances) and
tests/test_gpu_ae_tiles.py (the device against the float64 model).  Nothing here imports the library.

Every case is the smallest shape that crosses its boundaries in novel-vqa_amd/csrc/ae.hip: a full gate-GEMM row tile followed by
a partial one (B > 64), a second unit tile that is not full (R = 72, 132), 128 x 128 tiles with row, column and K tails, a
split-K depth above 4 with a last slice that is no multiple of 32 rows, the slab budget cutting Z, column sums split over rows
(M >= 512), and lookup-gradient tokens of more than one chunk of 16 rows.  tests/test_ae_tile_cases.py restates the host rules
and asserts each of these per case, so a case cannot be shrunk back inside one tile unnoticed.

Inputs follow the arch's existing GPU module: parameters uniform(-0.08, 0.08), Dropout(1, 0.5, 77, 3), ragged lengths with row 0
at full length (tmax = D), seeded from zlib.crc32(name); the weak-paired cases draw their projection / bridge / lookup /
features as tests/test_gpu_ae2wp.py and tests/test_gpu_ae1wp.py do."""
import collections
import functools
import zlib

import numpy as np

import ae1wp_ref_torch
import ae2_ref_torch
import ae2wp_ref_torch
import ae_ref_torch

Case = collections.namedtuple("Case", "name arch dims drop variant")

CASES = [
    #    name                     arch     (B, D, V, E, R, L[, I]) -- AE1_WP: (B, D, V, E, R, I)   dropout  variant
    Case("b136_l2_drop",          "ae1",   (136, 6, 699, 40, 72, 2),                               True,    None),
    Case("b200_l1",               "ae1",   (200, 5, 300, 68, 132, 1),                              False,   None),
    Case("b264_v1100_drop",       "ae1",   (264, 3, 1100, 16, 16, 1),                              True,    None),
    Case("b70_v3_drop",           "ae1",   (70, 5, 3, 12, 8, 1),                                   True,    None),
    Case("ae2_b136_l2_drop_img",  "ae2",   (136, 5, 300, 40, 72, 2),                               True,    "img"),
    Case("ae2_b200_null_img",     "ae2",   (200, 4, 90, 68, 132, 1),                               False,   "null"),
    Case("wp_b136_same_drop",     "ae2wp", (136, 5, 60, 40, 72, 1, 100),                           True,    "same"),
    Case("wp_b136_null",          "ae2wp", (136, 5, 60, 40, 72, 1, 100),                           False,   "null"),
    Case("ae1wp_b136_same_drop",  "ae1wp", (136, 5, 60, 40, 72, 100),                              True,    "same"),
    Case("ae1wp_b136_skip",       "ae1wp", (136, 5, 60, 40, 72, 100),                              False,   "skip"),
]
BY_NAME = {c.name: c for c in CASES}

Dropout = collections.namedtuple("Dropout", "mode p seed step")
DROPOUT = Dropout(1, 0.5, 77, 3)

# greedy ties: two identical W_proj rows / b_proj entries that beat every other column; (lo, hi) placements over k_ae_argmax's
# 256 threads -- neighbouring lanes, two waves, the same thread one stride later, and lo in wave 3 with hi in wave 0 of the
# next stride (the case the final cross-wave loop's index comparison exists for)
TIE_DIMS = (4, 3, 600, 8, 8, 1)
TIE_PAIRS = [(10, 11), (10, 74), (10, 266), (200, 300)]
TIE_BIAS = 50.0


def tokens(rng, B, D, V, tmax):
    lens = np.minimum(rng.integers(1, D + 1, B), tmax)
    lens[0] = tmax
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def features(rng, B, I):
    """post-ReLU-like rows: non-negative with zeros"""
    f = rng.uniform(0, 1, (B, I)).astype(np.float32)
    f[rng.uniform(0, 1, (B, I)) < 0.3] = 0.0
    return f


def layout(case):
    if case.arch == "ae1wp":
        B, D, V, E, R, I = case.dims
        return ae1wp_ref_torch.layout(D, V, E, R, I)
    return ae_ref_torch.layout(*case.dims[:6])


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict of the case's inputs (read-only: shared between tests): p (f32 flat parameters), tok (int32 [B x D]), dr (DROPOUT or
    None), and per arch -- ae2: img ([B x E] or None); ae2wp: w [E x I], b [E], f [B x I], et (encoder tokens or None);
    ae1wp: wlk [(V+1) x E], f [B x I], et (encoder tokens or None), es (encoder state [B x 2R] or None)"""
    case = BY_NAME[name]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    lo = layout(case)
    B, D, V, E, R = case.dims[:5]
    out = {"dr": DROPOUT if case.drop else None}
    p = rng.uniform(-0.08, 0.08, lo["_total"]).astype(np.float32)
    if case.arch in ("ae1", "ae2"):
        out["tok"] = tokens(rng, B, D, V, D)
        if case.arch == "ae2":
            out["img"] = rng.uniform(-1.0, 1.0, (B, E)).astype(np.float32) if case.variant == "img" else None
    elif case.arch == "ae2wp":
        I = case.dims[6]
        out["w"] = rng.uniform(-0.08, 0.08, (E, I)).astype(np.float32)
        out["b"] = rng.uniform(-0.05, 0.05, E).astype(np.float32)
        out["tok"] = tokens(rng, B, D, V, D)
        out["et"] = out["tok"] if case.variant == "same" else None
        out["f"] = features(rng, B, I)
    else:
        I = case.dims[5]
        # the bridge as the trainer draws it (nn.Linear's default), so that tanh is neither flat nor saturated
        for w, fan_in in (("w_q", 2 * R), ("b_q", 2 * R), ("w_v", I), ("b_v", I)):
            o, n = lo[w]
            p[o:o + n] = rng.uniform(-1, 1, n) / np.sqrt(fan_in)
        out["wlk"] = rng.uniform(-1.0, 1.0, (V + 1, E)).astype(np.float32)
        out["tok"] = tokens(rng, B, D, V, D)
        out["et"] = out["tok"] if case.variant == "same" else None
        out["es"] = rng.uniform(-0.5, 0.5, (B, 2 * R)).astype(np.float32) if case.variant == "skip" else None
        out["f"] = features(rng, B, I)
    out["p"] = p
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """the float64 model of the case's arch on its inputs (computed once per process; read-only)"""
    case, x = BY_NAME[name], inputs(name)
    p = x["p"].astype(np.float64)
    if case.arch == "ae1":
        return ae_ref_torch.forward(case.dims, p, x["tok"], dr=x["dr"], train=True)
    if case.arch == "ae2":
        img = None if x["img"] is None else x["img"].astype(np.float64)
        return ae2_ref_torch.forward(case.dims, p, x["tok"], images=img, dr=x["dr"])
    if case.arch == "ae2wp":
        return ae2wp_ref_torch.forward(case.dims, p, x["w"], x["b"], x["f"], x["tok"], enc_tokens=x["et"], dr=x["dr"])
    return ae1wp_ref_torch.forward(case.dims, p, x["wlk"], x["f"], x["tok"], enc_tokens=x["et"], enc_state=x["es"], dr=x["dr"])


def tie_inputs(lo_col, hi_col):
    """(params f32, tokens) of the greedy-tie context: W_proj rows lo_col and hi_col (0-based columns of the logits) and their
    b_proj entries identical, the bias TIE_BIAS above anything the other columns can reach (|h| < 1, |W| <= 0.08, R = 8)"""
    B, D, V, E, R, L = TIE_DIMS
    lay = ae_ref_torch.layout(*TIE_DIMS)
    rng = np.random.default_rng(zlib.crc32(b"greedy_ties") + 1000 * lo_col + hi_col)
    p = rng.uniform(-0.08, 0.08, lay["_total"]).astype(np.float32)
    ow, ob = lay["w_proj"][0], lay["b_proj"][0]
    p[ow + hi_col * R:ow + (hi_col + 1) * R] = p[ow + lo_col * R:ow + (lo_col + 1) * R]
    p[ob + lo_col] = p[ob + hi_col] = TIE_BIAS
    return p, tokens(rng, B, D, V, D)


# a case is what its row of the table says only if its batch reaches tmax = D
for _c in CASES:
    assert ae_ref_torch.tmax_of(inputs(_c.name)["tok"]) == _c.dims[1], _c.name
