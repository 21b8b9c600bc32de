"""The cases of the auto-encoder bf16 operand mode and their inputs, shared by tests/test_ae_bf16_ref.py (CPU: the reference
alone meets the conditions) and tests/test_gpu_ae_bf16.py (the device against the reference), plus the three reference runs a
case needs.  Nothing here imports the library."""
import collections
import zlib

import numpy as np
import torch

import ae_bf16_ref_torch as ref

Case = collections.namedtuple("Case", "name dims tmax drop ae2 wide")

CASES = [
    #    name                 (B, D, V, E, R, L)              tmax dropout ae2 (image rows) wide
    Case("l1_t2",             (8, 4, 30, 32, 32, 1),          2,   False,  False,           False),
    Case("l2_drop_t3",        (7, 5, 60, 32, 64, 2),          3,   True,   False,           False),
    Case("l2_drop_t6",        (16, 6, 200, 64, 64, 2),        6,   True,   False,           False),
    Case("ae2_img_t3",        (12, 5, 60, 32, 32, 2),         3,   False,  True,            False),
    # wide, short cascades (R = 512: nothing for a flipped rounding to amplify through); the last at full vocabulary width
    Case("wide_l1_t1",        (256, 2, 2000, 512, 512, 1),    1,   False,  False,           True),
    Case("wide_l2_t2",        (256, 2, 2000, 512, 512, 2),    2,   False,  False,           True),
    Case("wide_fullvocab_t3", (64, 3, 14773, 512, 512, 1),    3,   False,  False,           True),
]
# D = 16, full vocabulary, E = R = 512, B cut to 256 so that the CPU reference stays affordable
LONG = Case("long_d16_fullvocab", (256, 16, 14773, 512, 512, 1), 16, False, False, False)

Dropout = collections.namedtuple("Dropout", "mode p seed step")
DROPOUT = Dropout(1, 0.5, 77, 3)

# greedy decoding: the shape and weight range of tests/test_gpu_ae.py's evaluate test
GREEDY_DIMS = (6, 5, 13, 8, 8, 2)
GREEDY_SEED = 9  # (seeds 5 - 7 leave a top-two gap below the bound of test_greedy_input_has_decisive_argmaxes in this mode)


def tokens(rng, B, D, V, tmax):
    lens = np.minimum(rng.integers(1, D + 1, B), tmax)
    lens[0] = tmax
    tok = np.zeros((B, D), np.int32)
    for b, n in enumerate(lens):
        tok[b, :n] = rng.integers(1, V + 1, n)
    return tok


def inputs(case):
    """(params f32, tokens int32 [B x D], images f32 [B x E] or None, dropout or None)"""
    B, D, V, E, R, L = case.dims
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    p = rng.uniform(-0.08, 0.08, ref.layout(*case.dims)["_total"]).astype(np.float32)
    tok = tokens(rng, B, D, V, case.tmax)
    img = rng.uniform(-1.0, 1.0, (B, E)).astype(np.float32) if case.ae2 else None
    return p, tok, img, DROPOUT if case.drop else None


def greedy_inputs():
    rng = np.random.default_rng(GREEDY_SEED)
    B, D, V = GREEDY_DIMS[:3]
    p = rng.uniform(-0.6, 0.6, ref.layout(*GREEDY_DIMS)["_total"]).astype(np.float32)  # wide weights: decisive argmaxes
    return p, tokens(rng, B, D, V, 4)


def l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / (np.linalg.norm(b) + 1e-300))


def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def references(case, with_self=True):
    """The bf16 reference in f64 arithmetic (`ref`), its f32-arithmetic twin (`ref32`, None without with_self) and the unrounded
    f64 model (`exact`), each ae_bf16_ref_torch.forward's dict, and the layout entries the distance conditions apply to:
    b_proj is left out (no product feeds it: its bf16-to-f32 distance is ~2e-6) and so is every tensor whose reference
    gradient is all zero (the encoder's w_h2h at tmax = 1)."""
    p, tok, img, dr = inputs(case)
    kw = dict(images=img, ae2=case.ae2, dr=dr)
    out = {"ref": ref.forward(case.dims, p, tok, **kw),
           "ref32": ref.forward(case.dims, p, tok, dtype=torch.float32, **kw) if with_self else None,
           "exact": ref.forward(case.dims, p, tok, rounded=False, **kw)}
    lo = ref.layout(*case.dims)
    g = out["ref"]["grads"]
    out["tensors"] = {k: v for k, v in lo.items()
                      if not k.startswith("_") and k != "b_proj" and np.abs(g[v[0]:v[0] + v[1]]).max() > 0}
    out["layout"] = lo
    return out


def distances(refs, got=None):
    """per tensor: dist = bf16-to-f32 distance of the reference, self = the reference's f32 twin against it, self_to_f32 = the
    twin's distance to the unrounded model; with got (a flat gradient): e = its distance to the reference and to_f32 = its
    distance to the unrounded model.  All L2, relative to the second operand."""
    out = {}
    for k, (o, n) in refs["tensors"].items():
        s = slice(o, o + n)
        d = {"dist": l2(refs["ref"]["grads"][s], refs["exact"]["grads"][s])}
        if refs["ref32"] is not None:
            d["self"] = l2(refs["ref32"]["grads"][s], refs["ref"]["grads"][s])
            d["self_to_f32"] = l2(refs["ref32"]["grads"][s], refs["exact"]["grads"][s])
        if got is not None:
            d["e"] = l2(got[s], refs["ref"]["grads"][s])
            d["to_f32"] = l2(got[s], refs["exact"]["grads"][s])
        out[k] = d
    return out
