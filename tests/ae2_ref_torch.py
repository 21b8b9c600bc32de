"""Independent float64 PyTorch-autograd model of the reference's image-first-token text auto-encoder and its criterion,
written from the Lua (001_train_autoencoder/misc/AutoEncoder.lua, misc/LSTM_encoder.lua, 003_train_vqa_arch2/misc/
LSTM_decoder.lua).  The yardstick of tests/test_*ae2*.py; nothing here imports the library.

The encoder runs tmax + 2 steps: the image row [B x E] fed directly as x (:262-264), START (:265-269), then the tokens
seq[t-2] with 0 -> 1 (:270-291).  The decoder runs START, then the tokens, tmax + 1 steps (:318-360).  The lookup is a plain
nn.LookupTable (:28): no Dropout, no Tanh.  d(images) is the encoder's step-1 input gradient (:405-414).

Dropout masks come from tests/ref_autograd.py's drop_scales with the NVQA_ARCH_AE2 indices of include/nvqa_rng.h (a step
stride of D + 2).  The layout, tmax rule and criterion targets are the arch1 auto-encoder's (ae_ref_torch.py)."""
import numpy as np
import torch

from ae_ref_torch import _cell, criterion_targets, layout, tmax_of
from ref_autograd import drop_scales

SITE_TOP, SITE_LSTM = 7, 8

__all__ = ["layout", "tmax_of", "criterion_targets", "encoder_steps", "forward", "greedy"]


def encoder_steps(tokens):
    """the encoder's tmax of updateOutput (:258-309): image, START, then every column up to the last non-null one"""
    return tmax_of(tokens) + 2


def _seg_fn(P, lo):
    def seg(name, shape):
        o, n = lo[name]
        return P[o:o + n].view(*shape)
    return seg


def _lstm_step(seg, part, k, t, x, state, dr, B, D, E, R, L):
    """one step of the encoder (k = 0) / decoder (k = 1) at its step t: returns the new [(c, h)] per layer"""
    new, inp = [], x
    for l in range(L):
        if l > 0:
            sc = drop_scales(dr, SITE_LSTM, (B, R), lambda b, j: (((k * L + l) * B + b) * (D + 2) + t) * R + j)
            inp = new[l - 1][1] * sc
        n_in = E if l == 0 else R
        a = (inp @ seg(f"{part}{l}_w_i2h", (4 * R, n_in)).T + seg(f"{part}{l}_b_i2h", (4 * R,))
             + state[l][1] @ seg(f"{part}{l}_w_h2h", (4 * R, R)).T + seg(f"{part}{l}_b_h2h", (4 * R,)))
        new.append(_cell(a, state[l][0], R))
    return new


def forward(dims, params_np, tokens, images=None, dr=None, train=True, want_grads=True, nvalid=None):
    """Training / evaluate-mode forward + criterion (+ backward).  dims: (B, D, V, E, R, L); images [B x E] or None (zeros,
    the text script's DataLoader).  Returns dict(loss, grads (flat float64 numpy or None), dimages ([B x E] or None),
    logits [(tmax+1), B, V+1], n, tmax)."""
    B, D, V, E, R, L = dims
    lo = layout(*dims)
    tok = np.asarray(tokens, np.int64)
    nvalid = B if nvalid is None else nvalid
    P = torch.tensor(np.asarray(params_np, np.float64), requires_grad=want_grads)
    seg = _seg_fn(P, lo)
    dr = dr if train else None
    T = tmax_of(tok)
    Wlk = seg("w_lk", (V + 1, E))
    img = torch.zeros(B, E, dtype=torch.float64) if images is None else torch.tensor(np.asarray(images, np.float64))
    img.requires_grad_(want_grads)

    def lookup(ids):
        return Wlk[torch.as_tensor(np.asarray(ids, np.int64) - 1)]

    toks = np.where(tok[:, :T] == 0, 1, tok[:, :T]).T  # [T, B], 0 -> 1
    start = np.full(B, V + 1)
    xs_enc = [img, lookup(start)] + [lookup(toks[t]) for t in range(T)]
    xs_dec = [lookup(start)] + [lookup(toks[t]) for t in range(T)]

    zero = torch.zeros(B, R, dtype=torch.float64)
    st = [(zero, zero)] * L
    for t, x in enumerate(xs_enc):
        st = _lstm_step(seg, "enc", 0, t, x, st, dr, B, D, E, R, L)
    tops = []
    for s, x in enumerate(xs_dec):  # the decoder starts from the encoder's final state (:312-316)
        st = _lstm_step(seg, "dec", 1, s, x, st, dr, B, D, E, R, L)
        tops.append(st[-1][1])
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    logits = []
    for s, h in enumerate(tops):
        sc = drop_scales(dr, SITE_TOP, (B, R), lambda b, j: (b * (D + 2) + s) * R + j)
        logits.append((h * sc) @ Wp.T + bp)
    logits = torch.stack(logits)  # [T+1, B, V+1]
    logp = torch.log_softmax(logits, dim=2)
    tg, _ = criterion_targets(tok[:nvalid], V)
    n = len(tg)
    loss = -sum(logp[s, b, c] for (s, b), c in tg.items()) / n
    grads = dimages = None
    if want_grads:
        loss.backward()
        grads = P.grad.detach().numpy().copy()
        dimages = img.grad.detach().numpy().copy()
    return {"loss": float(loss.detach()), "grads": grads, "dimages": dimages, "logits": logits.detach().numpy(), "n": n,
            "tmax": T}


def greedy(dims, params_np, tokens, images=None):
    """sample(imgs, sents) with sample_max = 1 (:131-217): encode image, START and the tokens as the training forward does
    (0 -> 1, up to tmax), then decode by argmax.  Returns [B x D] 1-based tokens (V+1 = END)."""
    B, D, V, E, R, L = dims
    lo = layout(*dims)
    P = torch.tensor(np.asarray(params_np, np.float64))
    seg = _seg_fn(P, lo)
    tok = np.asarray(tokens, np.int64)
    T = tmax_of(tok)
    Wlk = seg("w_lk", (V + 1, E))
    img = torch.zeros(B, E, dtype=torch.float64) if images is None else torch.tensor(np.asarray(images, np.float64))

    def lookup(ids):
        return Wlk[torch.as_tensor(np.asarray(ids, np.int64) - 1)]

    zero = torch.zeros(B, R, dtype=torch.float64)
    st = [(zero, zero)] * L
    xs = [img, lookup(np.full(B, V + 1))] + [lookup(np.where(tok[:, t] == 0, 1, tok[:, t])) for t in range(T)]
    for t, x in enumerate(xs):
        st = _lstm_step(seg, "enc", 0, t, x, st, None, B, D, E, R, L)
    out = np.zeros((B, D), np.int64)
    ids = np.full(B, V + 1)
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    for s in range(D):
        st = _lstm_step(seg, "dec", 1, s, lookup(ids), st, None, B, D, E, R, L)
        lg = (st[-1][1] @ Wp.T + bp).numpy()
        ids = lg.argmax(axis=1) + 1
        out[:, s] = ids
    return out
