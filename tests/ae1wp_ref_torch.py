"""Independent float64 PyTorch-autograd model of the reference's arch1 weak-paired auto-encoder and its criterion, written from
the Lua: L2Normalize (the end of build_cnn_2) -> AutoEncoder_vqa (001_train_autoencoder/misc/AutoEncoder_vqa_arch.lua) ->
LanguageModelCriterion.  The yardstick of tests/test_*ae1wp*.py; nothing here imports the library.

AutoEncoder_vqa is the text auto-encoder of AutoEncoder_text_nostart.lua (one layer, :33) with
  * a frozen lookup LookupTable -> Dropout -> Tanh whose clones stay in evaluate() mode while training (:133-134), so
    x = tanh(W_lk[token]) without a mask, and parameters() leaves the table out (:103-127);
  * two token streams: the encoder reads seq_enc for tmax(seq_enc) steps (:293-331), the decoder START then seq (:354-397);
  * a bridge between them (:35-40, :337-350): with j = JoinTable(final state) = [c_T | h_T] (LSTM_encoder returns c before h:
    num_state - 1 is the cell, num_state the hidden state, :342-343),
        m = Dropout(0.5)(netdef.AxB(2R, I, 2R, 0.5){j, f^}) = D_Z (tanh(W_q (D_Q j) + b_q) * tanh(W_v (D_V f^) + b_v)),
        decoder state (c, h) = (c_T + m[:, :R], h_T + m[:, R:]);
  * encoder_skip_flag = 1 (:332-335): the encoder does not run, j is input[2] and (c_T, h_T) are its halves; the backward pass
    then never touches the encoder (:440), whose gradient stays zero.
The flat vector is parameters(): [encoder | decoder | multimodal], multimodal = W_q, b_q, W_v, b_v (include/nvqa_layout.h,
arch 6).  Dropout masks: the bridge uses the counter-based sites Q (b 2R + k), V (b I + k), Z (b 2R + k) of include/nvqa_rng.h,
the top-h Dropout AE1's site and index (ae_ref_torch.py)."""
import numpy as np
import torch

from ae_ref_torch import _cell, criterion_targets, tmax_of
from ae2wp_ref_torch import l2_normalize
from ref_autograd import drop_scales

SITE_Q, SITE_V, SITE_Z, SITE_TOP = 2, 3, 4, 7

__all__ = ["layout", "tmax_of", "criterion_targets", "l2_normalize", "forward", "encode", "greedy"]


def layout(D, V, E, R, I):
    """{name: (offset, size)} of the flat vector [encoder | decoder | multimodal] (include/nvqa_layout.h, arch 6; L = 1)."""
    lo, off = {}, 0
    for part in ("enc", "dec"):
        for name, size in (("w_i2h", 4 * R * E), ("b_i2h", 4 * R), ("w_h2h", 4 * R * R), ("b_h2h", 4 * R)):
            lo[f"{part}0_{name}"] = (off, size)
            off += size
        if part == "enc":
            lo["_seg0"] = off
    for name, size in (("w_proj", (V + 1) * R), ("b_proj", V + 1)):
        lo[name] = (off, size)
        off += size
    lo["_seg1"] = off - lo["_seg0"]
    for name, size in (("w_q", 4 * R * R), ("b_q", 2 * R), ("w_v", 2 * R * I), ("b_v", 2 * R)):
        lo[name] = (off, size)
        off += size
    lo["_seg2"] = off - lo["_seg0"] - lo["_seg1"]
    lo["_total"] = off
    return lo


def _step(seg, part, x, state, E, R):
    c, h = state
    a = (x @ seg(f"{part}0_w_i2h", (4 * R, E)).T + seg(f"{part}0_b_i2h", (4 * R,))
         + h @ seg(f"{part}0_w_h2h", (4 * R, R)).T + seg(f"{part}0_b_h2h", (4 * R,)))
    return _cell(a, c, R)


def _model(dims, P, w_lk):
    B, D, V, E, R, I = dims
    lo = layout(D, V, E, R, I)

    def seg(name, shape):
        o, n = lo[name]
        return P[o:o + n].view(*shape)

    Wlk = torch.tensor(np.asarray(w_lk, np.float64).reshape(V + 1, E))

    def lookup(ids):
        ids = np.asarray(ids, np.int64)
        return torch.tanh(Wlk[torch.as_tensor(np.where(ids == 0, 1, ids) - 1)])

    return lo, seg, lookup


def _encode(dims, seg, lookup, enc_tokens):
    B, D, V, E, R, I = dims
    et = np.asarray(enc_tokens, np.int64)
    zero = torch.zeros(B, R, dtype=torch.float64)
    st = (zero, zero)
    for t in range(tmax_of(et)):
        st = _step(seg, "enc", lookup(et[:, t]), st, E, R)
    return st


def _bridge(dims, seg, c_T, h_T, fhat, dr):
    B, D, V, E, R, I = dims
    j = torch.cat([c_T, h_T], dim=1)
    dq = drop_scales(dr, SITE_Q, (B, 2 * R), lambda b, k: b * 2 * R + k)
    dv = drop_scales(dr, SITE_V, (B, I), lambda b, k: b * I + k)
    dz = drop_scales(dr, SITE_Z, (B, 2 * R), lambda b, k: b * 2 * R + k)
    qc = torch.tanh((j * dq) @ seg("w_q", (2 * R, 2 * R)).T + seg("b_q", (2 * R,)))
    ic = torch.tanh((fhat * dv) @ seg("w_v", (2 * R, I)).T + seg("b_v", (2 * R,)))
    m = dz * (qc * ic)
    return c_T + m[:, :R], h_T + m[:, R:]


def forward(dims, params_np, w_lk, feats, tokens, enc_tokens=None, enc_state=None, dr=None, train=True, want_grads=True,
            nvalid=None, normalize=True):
    """Training / evaluate-mode forward + criterion (+ backward).  dims: (B, D, V, E, R, I); w_lk [(V+1) x E] frozen; feats
    [B x I] before L2Normalize; exactly one of enc_tokens [B x D] and enc_state [B x 2R] (encoder_skip_flag = 1).
    normalize=False takes feats as f^ itself (finite differences of dfhat).
    Returns dict(loss, grads (flat), dfhat [B x I], state [B x 2R] = [c_T | h_T], logits, n, tmax, te)."""
    B, D, V, E, R, I = dims
    assert (enc_tokens is None) != (enc_state is None)
    tok = np.asarray(tokens, np.int64)
    nvalid = B if nvalid is None else nvalid
    dr = dr if train else None
    P = torch.tensor(np.asarray(params_np, np.float64), requires_grad=want_grads)
    lo, seg, lookup = _model(dims, P, w_lk)
    fhat = torch.tensor(l2_normalize(feats, nvalid) if normalize else np.array(feats, np.float64), requires_grad=want_grads)
    if enc_state is None:
        c_T, h_T = _encode(dims, seg, lookup, enc_tokens)
        te = tmax_of(enc_tokens)
    else:
        j = torch.tensor(np.asarray(enc_state, np.float64).reshape(B, 2 * R))
        c_T, h_T, te = j[:, :R], j[:, R:], 0
    st = _bridge(dims, seg, c_T, h_T, fhat, dr)
    T = tmax_of(tok)
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    logits = []
    for s in range(T + 1):
        x = lookup(np.full(B, V + 1) if s == 0 else tok[:, s - 1])
        st = _step(seg, "dec", x, st, E, R)
        sc = drop_scales(dr, SITE_TOP, (B, R), lambda b, k: (b * (D + 1) + s) * R + k)
        logits.append((st[1] * sc) @ Wp.T + bp)
    logits = torch.stack(logits)
    logp = torch.log_softmax(logits, dim=2)
    tg, _ = criterion_targets(tok[:nvalid], V)
    n = len(tg)
    loss = -sum(logp[s, b, c] for (s, b), c in tg.items()) / n
    out = {"loss": float(loss.detach()), "grads": None, "dfhat": None, "logits": logits.detach().numpy(), "n": n, "tmax": T,
           "te": te, "state": torch.cat([c_T, h_T], dim=1).detach().numpy().copy()}
    if want_grads:
        loss.backward()
        out["grads"] = P.grad.detach().numpy().copy()
        out["dfhat"] = fhat.grad.detach().numpy().copy()
    return out


def encode(dims, params_np, w_lk, enc_tokens):
    """evaluate-mode [c_T | h_T] [B x 2R]"""
    P = torch.tensor(np.asarray(params_np, np.float64))
    _, seg, lookup = _model(dims, P, w_lk)
    c_T, h_T = _encode(dims, seg, lookup, enc_tokens)
    return torch.cat([c_T, h_T], dim=1).numpy()


def greedy(dims, params_np, w_lk, feats, enc_tokens, nvalid=None):
    """sample(feats, sents) with sample_max = 1 (:159-250), the encoder fed as the training forward feeds it (tmax(enc_tokens)
    steps, 0 -> 1; the reference's sample() runs all seq_length steps: DESIGN.md 9.3), then decoding by argmax for D steps.
    Returns (tokens [B x D] 1-based, V+1 = END; gap [B x D] = top-1 minus top-2 logit of every decoded step)."""
    B, D, V, E, R, I = dims
    P = torch.tensor(np.asarray(params_np, np.float64))
    _, seg, lookup = _model(dims, P, w_lk)
    c_T, h_T = _encode(dims, seg, lookup, enc_tokens)
    st = _bridge(dims, seg, c_T, h_T, torch.from_numpy(l2_normalize(feats, nvalid)), None)
    out, gap = np.zeros((B, D), np.int64), np.zeros((B, D))
    ids = np.full(B, V + 1)
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    for s in range(D):
        st = _step(seg, "dec", lookup(ids), st, E, R)
        lg = (st[1] @ Wp.T + bp).numpy()
        ids = lg.argmax(axis=1) + 1
        top2 = np.sort(lg, axis=1)[:, -2:]
        out[:, s], gap[:, s] = ids, top2[:, 1] - top2[:, 0]
    return out, gap
