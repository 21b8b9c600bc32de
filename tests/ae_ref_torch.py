"""Independent float64 PyTorch-autograd model of the reference's text auto-encoder and its criterion, written from the Lua
(001_train_autoencoder/misc/AutoEncoder_text_nostart.lua, misc/LSTM_encoder.lua, 003_train_vqa_arch2/misc/LSTM_decoder.lua),
plus a NumPy mirror of adam() (misc/optim_updates.lua:78-111) with the clamp / weight decay of lossFun
(001_train_arch1_text_autoencoder.lua:237-243).  The yardstick of tests/test_ae_*.py; nothing here imports the library.

Dropout masks come from tests/ref_autograd.py's hash32 / drop_scales with the auto-encoder sites of include/nvqa_rng.h."""
import numpy as np
import torch

from ref_autograd import drop_scales

SITE_ENC_LK, SITE_DEC_LK, SITE_TOP, SITE_LSTM = 5, 6, 7, 8


def layout(B, D, V, E, R, L):
    """{name: (offset, size)} of the flat vector: [encoder | decoder | lookup] (include/nvqa_layout.h, arch 3)."""
    lo, off = {}, 0
    for part in ("enc", "dec"):
        for l in range(L):
            n_in = E if l == 0 else R
            for name, size in (("w_i2h", 4 * R * n_in), ("b_i2h", 4 * R), ("w_h2h", 4 * R * R), ("b_h2h", 4 * R)):
                lo[f"{part}{l}_{name}"] = (off, size)
                off += size
        if part == "enc":
            lo["_seg0"] = off
        else:
            lo["w_proj"] = (off, (V + 1) * R)
            off += (V + 1) * R
            lo["b_proj"] = (off, V + 1)
            off += V + 1
            lo["_seg1"] = off - lo["_seg0"]
    lo["w_lk"] = (off, (V + 1) * E)
    off += (V + 1) * E
    lo["_seg2"] = off - lo["_seg0"] - lo["_seg1"]
    lo["_total"] = off
    return lo


def tmax_of(tokens):
    """last 1-based column with a non-null token in any row (:249-292)"""
    nz = np.nonzero((np.asarray(tokens) != 0).any(axis=0))[0]
    return int(nz[-1]) + 1 if nz.size else 0


def criterion_targets(tokens, V):
    """LanguageModelCriterion (:416-450): {(s, b): 0-based class} for the decoder steps s = 0..D, and n."""
    tok = np.asarray(tokens)
    B, D = tok.shape
    out = {}
    for b in range(B):
        first = True
        for s in range(D + 1):
            v = int(tok[b, s]) if s < D else 0
            if v == 0 and first:
                v = V + 1
                first = False
            if v != 0:
                out[(s, b)] = v - 1
    return out, len(out)


def _cell(a, c_prev, R):
    i, f, o, g = torch.sigmoid(a[:, :R]), torch.sigmoid(a[:, R:2 * R]), torch.sigmoid(a[:, 2 * R:3 * R]), torch.tanh(a[:, 3 * R:])
    c = f * c_prev + i * g
    return c, o * torch.tanh(c)


def forward(dims, params_np, tokens, dr=None, train=True, want_grads=True, nvalid=None):
    """Training / evaluate-mode forward + criterion (+ backward).  dims: (B, D, V, E, R, L).
    Returns dict(loss, grads (flat float64 numpy, or None), logits [(tmax+1), B, V+1], n, tmax)."""
    B, D, V, E, R, L = dims
    lo = layout(*dims)
    tok = np.asarray(tokens, np.int64)
    nvalid = B if nvalid is None else nvalid
    P = torch.tensor(np.asarray(params_np, np.float64), requires_grad=want_grads)

    def seg(name, shape):
        o, n = lo[name]
        return P[o:o + n].view(*shape)

    dr = dr if train else None
    T = tmax_of(tok)
    Wlk = seg("w_lk", (V + 1, E))

    def lookup(ids, site, index_fn, nsteps):
        # LookupTable -> Dropout -> Tanh; ids [nsteps, B] 1-based
        sc = drop_scales(dr, site, (nsteps, B, E), index_fn)
        return torch.tanh(Wlk[torch.as_tensor(ids - 1)] * sc)

    enc_ids = np.where(tok[:, :T] == 0, 1, tok[:, :T]).T  # [T, B]
    x_enc = lookup(enc_ids, SITE_ENC_LK, lambda t, b, e: (b * D + t) * E + e, T)
    dec_ids = np.empty((T + 1, B), np.int64)
    dec_ids[0] = V + 1
    if T > 0:
        dec_ids[1:] = np.where(tok[:, :T] == 0, 1, tok[:, :T]).T
    x_dec = lookup(dec_ids, SITE_DEC_LK, lambda s, b, e: (b * (D + 1) + s) * E + e, T + 1)

    def run(part, k, xs, state):
        """one LSTM (encoder k = 0 / decoder k = 1) over len(xs) steps from state [(c, h)] per layer; returns the new
        state and the top h of every step"""
        tops = []
        for t, x in enumerate(xs):
            new = []
            inp = x
            for l in range(L):
                if l > 0:
                    sc = drop_scales(dr, SITE_LSTM, (B, R), lambda b, j: (((k * L + l) * B + b) * (D + 1) + t) * R + j)
                    inp = new[l - 1][1] * sc
                n_in = E if l == 0 else R
                a = (inp @ seg(f"{part}{l}_w_i2h", (4 * R, n_in)).T + seg(f"{part}{l}_b_i2h", (4 * R,))
                     + state[l][1] @ seg(f"{part}{l}_w_h2h", (4 * R, R)).T + seg(f"{part}{l}_b_h2h", (4 * R,)))
                new.append(_cell(a, state[l][0], R))
            state = new
            tops.append(new[-1][1])
        return state, tops

    zero = torch.zeros(B, R, dtype=torch.float64)
    st, _ = run("enc", 0, [x_enc[t] for t in range(T)], [(zero, zero)] * L)
    _, tops = run("dec", 1, [x_dec[s] for s in range(T + 1)], st)
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    logits = []
    for s, h in enumerate(tops):
        sc = drop_scales(dr, SITE_TOP, (B, R), lambda b, j: (b * (D + 1) + s) * R + j)
        logits.append((h * sc) @ Wp.T + bp)
    logits = torch.stack(logits)  # [T+1, B, V+1]
    logp = torch.log_softmax(logits, dim=2)
    tg, _ = criterion_targets(tok[:nvalid], V)
    n = len(tg)
    loss = -sum(logp[s, b, c] for (s, b), c in tg.items()) / n
    grads = None
    if want_grads:
        loss.backward()
        grads = P.grad.detach().numpy().copy()
    return {"loss": float(loss.detach()), "grads": grads, "logits": logits.detach().numpy(), "n": n, "tmax": T}


def greedy(dims, params_np, tokens):
    """sample() with sample_max = 1 (:134-210), encoder fed as the training forward does (0 -> 1, up to tmax).
    Returns [B x D] 1-based tokens (V+1 = END)."""
    B, D, V, E, R, L = dims
    lo = layout(*dims)
    P = torch.tensor(np.asarray(params_np, np.float64))

    def seg(name, shape):
        o, n = lo[name]
        return P[o:o + n].view(*shape)

    tok = np.asarray(tokens, np.int64)
    T = tmax_of(tok)
    Wlk = seg("w_lk", (V + 1, E))

    def step(part, x, state):
        new, inp = [], x
        for l in range(L):
            if l > 0:
                inp = new[l - 1][1]
            n_in = E if l == 0 else R
            a = (inp @ seg(f"{part}{l}_w_i2h", (4 * R, n_in)).T + seg(f"{part}{l}_b_i2h", (4 * R,))
                 + state[l][1] @ seg(f"{part}{l}_w_h2h", (4 * R, R)).T + seg(f"{part}{l}_b_h2h", (4 * R,)))
            new.append(_cell(a, state[l][0], R))
        return new

    zero = torch.zeros(B, R, dtype=torch.float64)
    st = [(zero, zero)] * L
    for t in range(T):
        ids = np.where(tok[:, t] == 0, 1, tok[:, t])
        st = step("enc", torch.tanh(Wlk[torch.as_tensor(ids - 1)]), st)
    out = np.zeros((B, D), np.int64)
    ids = np.full(B, V + 1)
    Wp, bp = seg("w_proj", (V + 1, R)), seg("b_proj", (V + 1,))
    for s in range(D):
        st = step("dec", torch.tanh(Wlk[torch.as_tensor(ids - 1)]), st)
        lg = (st[-1][1] @ Wp.T + bp).numpy()
        ids = lg.argmax(axis=1) + 1
        out[:, s] = ids
    return out


class Adam:
    """NumPy mirror of lossFun's clamp + weight decay and adam() (misc/optim_updates.lua:78-111), float32 state."""

    def __init__(self, n):
        self.m = np.zeros(n, np.float32)
        self.v = np.zeros(n, np.float32)
        self.t = 0

    def update(self, x, g, lr, beta1, beta2, eps, wd, clamp):
        """returns (new x, paramsNorm, # updates) -- the statistics of x before the update, g after clamp + wd"""
        x = np.asarray(x, np.float32)
        g = np.clip(np.asarray(g, np.float32), -clamp, clamp) if clamp > 0 else np.asarray(g, np.float32)
        g = (g + np.float32(wd) * x).astype(np.float32)
        norm = float(np.sqrt((x.astype(np.float64) ** 2).sum()))
        count = int((np.abs(g * np.float32(lr)) >= np.abs(x) * np.float32(0.01)).sum())
        self.m = (np.float32(beta1) * self.m + np.float32(1 - beta1) * g).astype(np.float32)
        self.v = (np.float32(beta2) * self.v + np.float32(1 - beta2) * g * g).astype(np.float32)
        self.t += 1
        step = lr * np.sqrt(1 - beta2 ** self.t) / (1 - beta1 ** self.t)
        x = (x - np.float32(step) * (self.m / (np.sqrt(self.v) + np.float32(eps)))).astype(np.float32)
        return x, norm, count
