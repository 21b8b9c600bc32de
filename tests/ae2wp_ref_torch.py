"""Independent float64 PyTorch-autograd model of the reference's weak-paired auto-encoder and its criterion, written from the
Lua: L2Normalize -> Linear(I, E) (the end of build_cnn, 001_train_autoencoder/misc/net_utils.lua:37-41) -> AutoEncoderNull
(misc/AutoEncoderNull.lua) -> LanguageModelCriterion.  The yardstick of tests/test_*ae2wp*.py; nothing here imports the library.

AutoEncoderNull is AutoEncoder.lua with two token streams: the encoder reads {feats row, START, seq_input} for
2 + tmax(seq_input) steps (:272-309: a column whose tokens are all null is skipped, so the null sentence gives 2 steps); the
decoder and the criterion read seq (:318-365).  parameters() leaves out the lookup table (:86-107) and updateGradInput never
calls the lookup's backward (:389-391, :411-412): the lookup slice of `grads` is zero here.  dx0 is the encoder's step-1 input
gradient (dimgs, :409-410); it flows into the Linear: dW_p = dx0^T f^, db_p = colsum(dx0).

The LSTM steps, layout, tmax rule, criterion targets and dropout indices are the image-first-token auto-encoder's
(ae2_ref_torch.py): the masks of NVQA_ARCH_AE2_WP use NVQA_ARCH_AE2's indices (include/nvqa_rng.h)."""
import numpy as np
import torch

from ae2_ref_torch import _lstm_step, _seg_fn, criterion_targets, layout, tmax_of
from ref_autograd import drop_scales

SITE_TOP = 7

__all__ = ["layout", "tmax_of", "criterion_targets", "encoder_steps", "l2_normalize", "forward", "greedy"]


def encoder_steps(enc_tokens):
    """the encoder's tmax_enc of updateOutput: feats row and START always run, then every column up to the last one that holds
    a non-null token; None (the null sentence the script feeds with probability rand_val) gives 2"""
    return 2 + (0 if enc_tokens is None else tmax_of(enc_tokens))


def l2_normalize(feats, nvalid=None):
    """misc/L2Normalize.lua: every row divided by its L2 norm (an all-zero row gives 0/0, as in Torch); rows from nvalid on
    (the padding rows of an evaluate with n < B) are left as they are"""
    f = np.array(feats, np.float64)
    n = f.shape[0] if nvalid is None else nvalid
    f[:n] /= np.sqrt((f[:n] ** 2).sum(axis=1, keepdims=True))
    return f


def _encoder_inputs(x0, lookup, enc_tokens, B, V):
    te = encoder_steps(enc_tokens)
    xs = [x0, lookup(np.full(B, V + 1))]
    if te > 2:
        et = np.asarray(enc_tokens, np.int64)
        xs += [lookup(np.where(et[:, t] == 0, 1, et[:, t])) for t in range(te - 2)]
    return xs


def forward(dims, params_np, w_p, b_p, feats, tokens, enc_tokens=None, dr=None, train=True, want_grads=True, nvalid=None):
    """Training / evaluate-mode forward + criterion (+ backward).  dims: (B, D, V, E, R, L, I); w_p [E x I], b_p [E];
    feats [B x I] before L2Normalize; enc_tokens None = the null sentence.  Returns dict(loss, grads (flat, lookup slice 0),
    dw_p, db_p, dx0, fhat, x0, n, tmax, te)."""
    B, D, V, E, R, L, I = dims
    lo = layout(B, D, V, E, R, L)
    tok = np.asarray(tokens, np.int64)
    nvalid = B if nvalid is None else nvalid
    dr = dr if train else None
    P = torch.tensor(np.asarray(params_np, np.float64), requires_grad=want_grads)
    W = torch.tensor(np.asarray(w_p, np.float64).reshape(E, I), requires_grad=want_grads)
    bias = torch.tensor(np.asarray(b_p, np.float64).reshape(E), requires_grad=want_grads)
    seg = _seg_fn(P, lo)
    fhat = l2_normalize(feats, nvalid)
    x0 = torch.from_numpy(fhat) @ W.T + bias
    if want_grads:
        x0.retain_grad()
    Wlk = seg("w_lk", (V + 1, E))

    def lookup(ids):
        return Wlk[torch.as_tensor(np.asarray(ids, np.int64) - 1)]

    T = tmax_of(tok)
    xs_enc = _encoder_inputs(x0, lookup, enc_tokens, B, V)
    toks = np.where(tok[:, :T] == 0, 1, tok[:, :T]).T
    xs_dec = [lookup(np.full(B, V + 1))] + [lookup(toks[t]) for t in range(T)]
    zero = torch.zeros(B, R, dtype=torch.float64)
    st = [(zero, zero)] * L
    for t, x in enumerate(xs_enc):
        st = _lstm_step(seg, "enc", 0, t, x, st, dr, B, D, E, R, L)
    tops = []
    for s, x in enumerate(xs_dec):
        st = _lstm_step(seg, "dec", 1, s, x, st, dr, B, D, E, R, L)
        tops.append(st[-1][1])
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    logits = []
    for s, h in enumerate(tops):
        sc = drop_scales(dr, SITE_TOP, (B, R), lambda b, j: (b * (D + 2) + s) * R + j)
        logits.append((h * sc) @ Wp.T + bp)
    logits = torch.stack(logits)
    logp = torch.log_softmax(logits, dim=2)
    tg, _ = criterion_targets(tok[:nvalid], V)
    n = len(tg)
    loss = -sum(logp[s, b, c] for (s, b), c in tg.items()) / n
    out = {"loss": float(loss.detach()), "grads": None, "dw_p": None, "db_p": None, "dx0": None, "fhat": fhat,
           "x0": x0.detach().numpy().copy(), "n": n, "tmax": T, "te": len(xs_enc)}
    if want_grads:
        loss.backward()
        g = P.grad.detach().numpy().copy()
        o, k = lo["w_lk"]
        g[o:o + k] = 0.0  # no lookup backward: the table is frozen
        out.update(grads=g, dw_p=W.grad.detach().numpy().copy(), db_p=bias.grad.detach().numpy().copy(),
                   dx0=x0.grad.detach().numpy().copy())
    return out


def greedy(dims, params_np, w_p, b_p, feats, enc_tokens, nvalid=None):
    """sample(feats, sents, sents) with sample_max = 1 (:131-217), the encoder fed as the training forward feeds it (2 +
    tmax(enc_tokens) steps, 0 -> 1), then decoding by argmax for D steps.  Returns [B x D] 1-based tokens (V+1 = END)."""
    B, D, V, E, R, L, I = dims
    lo = layout(B, D, V, E, R, L)
    P = torch.tensor(np.asarray(params_np, np.float64))
    seg = _seg_fn(P, lo)
    Wlk = seg("w_lk", (V + 1, E))

    def lookup(ids):
        return Wlk[torch.as_tensor(np.asarray(ids, np.int64) - 1)]

    fhat = torch.from_numpy(l2_normalize(feats, nvalid))
    x0 = fhat @ torch.tensor(np.asarray(w_p, np.float64).reshape(E, I)).T + torch.tensor(np.asarray(b_p, np.float64))
    zero = torch.zeros(B, R, dtype=torch.float64)
    st = [(zero, zero)] * L
    for t, x in enumerate(_encoder_inputs(x0, lookup, enc_tokens, B, V)):
        st = _lstm_step(seg, "enc", 0, t, x, st, None, B, D, E, R, L)
    out = np.zeros((B, D), np.int64)
    ids = np.full(B, V + 1)
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    for s in range(D):
        st = _lstm_step(seg, "dec", 1, s, lookup(ids), st, None, B, D, E, R, L)
        ids = (st[-1][1] @ Wp.T + bp).numpy().argmax(axis=1) + 1
        out[:, s] = ids
    return out
