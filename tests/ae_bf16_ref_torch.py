"""PyTorch-autograd model of the text auto-encoders (NVQA_ARCH_AE1, and NVQA_ARCH_AE2 with its image row first) in the bf16
operand mode of nvqa_ae_set_precision: the yardstick of tests/test_ae_bf16_ref.py and tests/test_gpu_ae_bf16.py.  Nothing
here imports the library.

The contract (include/nvqa.h): both operands of every dense product are rounded to bf16
(round-to-nearest-even) and the product accumulates in higher precision; everything else -- parameters, activations, the
cell, lookup -> dropout -> tanh, the dropout masks (applied before the rounding), biases and their gradients, the softmax and
(softmax - onehot) / n before it is rounded as an operand, the lookup gradient -- is not rounded.  Every `x @ W^T` of the model
goes through ONE autograd function, _Matmul: forward r(x) @ r(W)^T, backward dx = r(g) @ r(W), dW = r(g)^T @ r(x), with
r = f32 -> bf16 -> back.  `rounded=False` turns r off (the model is then ae_ref_torch.forward / ae2_ref_torch.forward), and
`dtype` selects the arithmetic between the roundings: torch.float64 (the reference) or torch.float32 (its own f32 twin, whose
distance to the f64 version is the yardstick's self-distance).

Layout, tmax rule, criterion targets and the cell are ae_ref_torch's; dropout masks come from ref_autograd.drop_scales with
the auto-encoder sites and the indices of include/nvqa_rng.h (AE2: a step stride of D + 2)."""
import numpy as np
import torch

from ae_ref_torch import _cell, criterion_targets, layout, tmax_of
from ref_autograd import drop_scales

SITE_ENC_LK, SITE_DEC_LK, SITE_TOP, SITE_LSTM = 5, 6, 7, 8

__all__ = ["layout", "tmax_of", "criterion_targets", "r", "forward", "greedy"]


def r(t):
    """f32 -> bf16 (round to nearest even) -> back to t's dtype"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class _Matmul(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, rounded):
        ctx.save_for_backward(x, W)
        ctx.rounded = rounded
        return (r(x) @ r(W).t()) if rounded else x @ W.t()

    @staticmethod
    def backward(ctx, g):
        x, W = ctx.saved_tensors
        if ctx.rounded:
            return r(g) @ r(W), r(g).t() @ r(x), None
        return g @ W, g.t() @ x, None


def _chain(dims, P, tok, img, ae2, dr, dtype, rounded, direct_decode=False):
    """The encoder over the batch's tokens, then the decoder: teacher-forced (returns the logits [T+1, B, V+1]) or, with
    direct_decode, fed its own argmax for D steps (returns the samples [B x D] and the logits of those D steps)."""
    B, D, V, E, R, L = dims
    lo = layout(*dims)
    T = tmax_of(tok)
    stride = D + 2 if ae2 else D + 1  # the step stride of the dropout indices

    def seg(name, shape):
        o, n = lo[name]
        return P[o:o + n].view(*shape)

    def mm(x, W):
        return _Matmul.apply(x, W, rounded)

    def scales(site, shape, fn):
        return drop_scales(dr, site, shape, fn).to(dtype)

    Wlk = seg("w_lk", (V + 1, E))

    def lookup(ids, site, fn):
        rows = Wlk[torch.as_tensor(np.asarray(ids, np.int64) - 1)]
        if ae2:  # a plain nn.LookupTable
            return rows
        return torch.tanh(rows * scales(site, (B, E), fn))  # LookupTable -> Dropout -> Tanh

    def step(part, k, t, x, state):
        new, inp = [], x
        for l in range(L):
            if l > 0:
                inp = new[l - 1][1] * scales(SITE_LSTM, (B, R), lambda b, j: (((k * L + l) * B + b) * stride + t) * R + j)
            n_in = E if l == 0 else R
            a = (mm(inp, seg(f"{part}{l}_w_i2h", (4 * R, n_in))) + seg(f"{part}{l}_b_i2h", (4 * R,))
                 + mm(state[l][1], seg(f"{part}{l}_w_h2h", (4 * R, R))) + seg(f"{part}{l}_b_h2h", (4 * R,)))
            new.append(_cell(a, state[l][0], R))
        return new

    toks = np.where(tok[:, :T] == 0, 1, tok[:, :T]).T  # [T, B], 0 -> 1
    start = np.full(B, V + 1)
    zero = torch.zeros(B, R, dtype=dtype)
    st = [(zero, zero)] * L
    if ae2:
        xs = [img, lookup(start, 0, None)] + [lookup(toks[t], 0, None) for t in range(T)]
    else:
        xs = [lookup(toks[t], SITE_ENC_LK, lambda b, e, t=t: (b * D + t) * E + e) for t in range(T)]
    for t, x in enumerate(xs):
        st = step("enc", 0, t, x, st)
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))

    def project(s, h):
        return mm(h * scales(SITE_TOP, (B, R), lambda b, j: (b * stride + s) * R + j), Wp) + bp

    def dec_input(s, ids):
        return lookup(ids, SITE_DEC_LK, lambda b, e: (b * (D + 1) + s) * E + e)

    logits = []
    if direct_decode:
        out, ids = np.zeros((B, D), np.int64), start
        for s in range(D):
            st = step("dec", 1, s, dec_input(s, ids), st)
            logits.append(project(s, st[-1][1]))
            ids = logits[-1].detach().numpy().argmax(axis=1) + 1
            out[:, s] = ids
        return out, torch.stack(logits)
    for s in range(T + 1):
        st = step("dec", 1, s, dec_input(s, start if s == 0 else toks[s - 1]), st)
        logits.append(project(s, st[-1][1]))
    return torch.stack(logits)


def forward(dims, params_np, tokens, images=None, ae2=False, dr=None, train=True, want_grads=True, nvalid=None,
            dtype=torch.float64, rounded=True):
    """Training / evaluate-mode forward + criterion (+ backward).  dims: (B, D, V, E, R, L); ae2: the image row [B x E]
    (None = zeros) and START run in front of the encoder's tokens.  Returns dict(loss, grads (flat float64 numpy or None),
    dimages (AE2, [B x E]) or None, logits, n, tmax)."""
    B, D, V, E, R, L = dims
    tok = np.asarray(tokens, np.int64)
    nvalid = B if nvalid is None else nvalid
    P = torch.tensor(np.asarray(params_np, np.float64)).to(dtype).requires_grad_(want_grads)
    img = None
    if ae2:
        img = torch.zeros(B, E, dtype=dtype) if images is None else torch.tensor(np.asarray(images, np.float64)).to(dtype)
        img.requires_grad_(want_grads)
    logits = _chain(dims, P, tok, img, ae2, dr if train else None, dtype, rounded)
    logp = torch.log_softmax(logits, dim=2)
    tg, n = criterion_targets(tok[:nvalid], V)
    keys = sorted(tg)
    si, bi = np.array([k[0] for k in keys]), np.array([k[1] for k in keys])
    ci = np.array([tg[k] for k in keys])
    loss = -logp[torch.as_tensor(si), torch.as_tensor(bi), torch.as_tensor(ci)].sum() / n
    grads = dimages = None
    if want_grads:
        loss.backward()
        grads = P.grad.detach().to(torch.float64).numpy().copy()
        if ae2:
            dimages = img.grad.detach().to(torch.float64).numpy().copy()
    return {"loss": float(loss.detach()), "grads": grads, "dimages": dimages,
            "logits": logits.detach().to(torch.float64).numpy(), "n": n, "tmax": tmax_of(tok)}


def greedy(dims, params_np, tokens, images=None, ae2=False, dtype=torch.float64, rounded=True):
    """sample() with sample_max = 1: the encoder as in the training forward (evaluate mode), then D decoder steps fed their own
    argmax.  Returns (samples [B x D] 1-based with V+1 = END, logits [D, B, V+1] float64 numpy)."""
    B, D, V, E, R, L = dims
    tok = np.asarray(tokens, np.int64)
    P = torch.tensor(np.asarray(params_np, np.float64)).to(dtype)
    img = None
    if ae2:
        img = torch.zeros(B, E, dtype=dtype) if images is None else torch.tensor(np.asarray(images, np.float64)).to(dtype)
    with torch.no_grad():
        out, logits = _chain(dims, P, tok, img, ae2, None, dtype, rounded, direct_decode=True)
    return out, logits.to(torch.float64).numpy()
