"""Float64 decoders of the two text auto-encoders: the yardstick of nvqa_ae_sample (tests/test_ae_sample_ref.py pins this file,
tests/test_gpu_ae_sample.py compares the device with it).  Built on the step functions of ae_ref_torch.py / ae2_ref_torch.py;
nothing here imports the library.

sample(sents, opt) of 001_train_autoencoder/misc/AutoEncoder_text_nostart.lua:134-210 (and the same block of misc/AutoEncoder.lua):
the encoder is fed as the training forward feeds it (0 -> 1, up to the batch's tmax), the decoder START and then its own picks.
With z the logits row of a decoder step and l = z - logsumexp(z):
  multinomial  w_c = exp((z_c - max z) / T), CDF(c) = sum_{j<=c} w_j / sum_j w_j, pick = the smallest c with CDF(c) > u,
               u = (hash32(seed, step, 9, b D + s) >> 8) 2^-24; the reported log-prob is the untempered l[pick]
  beam         K hypotheses per sentence, score = sum of l, no length normalisation; position 0 expands one hypothesis; a live
               hypothesis k offers (k, c) at S_k + l_kc, a finished one (last token END = V+1) itself once at S_k, ranked as
               (k, END); the K best survive, ties to the smaller k (V+1) + c, best first; the output is hypothesis 0, END
               included, zeros behind it."""
import numpy as np
import torch

from ae2_ref_torch import _lstm_step, _seg_fn
from ae_ref_torch import layout, tmax_of
from ref_autograd import hash32

SITE_AE_SAMPLE = 9


def uniform(seed, step, idx):
    """the draw of sample position idx = b D + s: 24 bits of nvqa_hash32, exactly representable in f32"""
    return (hash32(seed, step, SITE_AE_SAMPLE, idx) >> 8) / 16777216.0


def uniforms(seed, step, n, D):
    return np.array([[uniform(seed, step, b * D + s) for s in range(D)] for b in range(n)])


def cdf(z, T):
    w = np.exp((z - z.max()) / T)
    return np.cumsum(w) / w.sum()


def multinomial_pick(z, u, T):
    """0-based pick of one row"""
    return min(int(np.searchsorted(cdf(np.asarray(z, np.float64), T), u, side="right")), len(z) - 1)


def log_softmax(z):
    m = z.max(axis=-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(axis=-1, keepdims=True))


class Model:
    """arch 3 (AE1: LookupTable -> Tanh) or 4 (AE2: plain LookupTable, image row and START in front of the encoder's tokens)"""

    def __init__(self, dims, params, arch=3):
        self.dims = B, D, V, E, R, L = dims
        self.arch = arch
        self.seg = _seg_fn(torch.tensor(np.asarray(params, np.float64)), layout(*dims))
        self.Wlk = self.seg("w_lk", (V + 1, E))
        self.Wp, self.bp = self.seg("w_proj", (V + 1, R)), self.seg("b_proj", (V + 1,))

    def lookup(self, ids):
        x = self.Wlk[torch.as_tensor(np.asarray(ids, np.int64) - 1)]
        return torch.tanh(x) if self.arch == 3 else x

    def _step(self, part, x, state):
        _, D, _, E, R, L = self.dims
        return _lstm_step(self.seg, part, 0, 0, x, state, None, x.shape[0], D, E, R, L)

    def encode(self, tokens, images=None):
        """[(c, h)] per layer, one row per sentence"""
        _, _, V, E, R, L = self.dims
        tok = np.asarray(tokens, np.int64)
        n, T = tok.shape[0], tmax_of(tok)
        zero = torch.zeros(n, R, dtype=torch.float64)
        st = [(zero, zero)] * L
        xs = []
        if self.arch == 4:
            xs = [torch.zeros(n, E, dtype=torch.float64) if images is None else torch.tensor(np.asarray(images, np.float64)),
                  self.lookup(np.full(n, V + 1))]
        xs += [self.lookup(np.where(tok[:, t] == 0, 1, tok[:, t])) for t in range(T)]
        for x in xs:
            st = self._step("enc", x, st)
        return st

    def decode_step(self, state, ids):
        """one decoder step fed the 1-based tokens ids: (new state, logits [rows x (V+1)] as numpy)"""
        st = self._step("dec", self.lookup(ids), state)
        return st, (st[-1][1] @ self.Wp.T + self.bp).numpy()


def rows_of(state, idx):
    idx = torch.as_tensor(np.asarray(idx, np.int64))
    return [(c[idx], h[idx]) for c, h in state]


def sample(dims, p, tok, u, T, images=None, arch=3):
    """the float64 model's own multinomial decode: (seq [n x D] 1-based, log-probs [n x D])"""
    return _decode(dims, p, tok, u, T, None, images, arch)[:2]


def sample_check(dims, p, tok, u, T, device_seq, images=None, arch=3):
    """The decoder replayed on the DEVICE's picks device_seq [n x D] (1-based).  Per position: cdf_lo / cdf_hi = the float64
    CDF just below and at the device's pick, pick = the float64 model's own pick for the same u (1-based), l = the float64
    log-prob of the device's pick, z = the float64 logits rows [n x D x (V+1)]."""
    seq, _, out = _decode(dims, p, tok, u, T, np.asarray(device_seq, np.int64), images, arch)
    out["pick"] = seq
    return out


def _decode(dims, p, tok, u, T, forced, images, arch):
    _, D, V, _, _, _ = dims
    m = Model(dims, p, arch)
    n = np.asarray(tok).shape[0]
    st = m.encode(tok, images)
    ids = np.full(n, V + 1)
    seq, lps = np.zeros((n, D), np.int64), np.zeros((n, D))
    out = {"cdf_lo": np.zeros((n, D)), "cdf_hi": np.zeros((n, D)), "l": np.zeros((n, D)), "z": np.zeros((n, D, V + 1))}
    for s in range(D):
        st, z = m.decode_step(st, ids)
        l = log_softmax(z)
        for b in range(n):
            c = multinomial_pick(z[b], u[b, s], T) if T is not None else int(z[b].argmax())
            seq[b, s] = c + 1
            lps[b, s] = l[b, c]
            if forced is not None:
                d, F = int(forced[b, s]) - 1, cdf(z[b], T) if T is not None else None
                if F is not None:
                    out["cdf_lo"][b, s], out["cdf_hi"][b, s] = (F[d - 1] if d > 0 else 0.0), F[d]
                out["l"][b, s] = l[b, d]
        out["z"][:, s] = z
        ids = seq[:, s] if forced is None else forced[:, s]
    return seq, lps, out


def greedy_check(dims, p, tok, device_seq, images=None, arch=3):
    """sample_check for the argmax: l of the device's picks and the logits rows, the decoder fed the device's picks"""
    return _decode(dims, p, tok, None, None, np.asarray(device_seq, np.int64), images, arch)[2]


def beam(dims, p, tok, K, images=None, arch=3):
    """(seq [n x D] with zeros behind END, log-probs [n x D], gap, zabs, z [n x D x (V+1)] the logits rows the tokens of seq were
    picked from, zeros behind END).  gap = the smallest score difference met between the
    K-th kept and the best rejected candidate at any position, and between the best and the second hypothesis after the last
    one (a smaller perturbation of the scores cannot change the output); zabs = the largest |logit| of any expanded row."""
    _, D, V, _, _, _ = dims
    m = Model(dims, p, arch)
    tok = np.asarray(tok)
    n, END = tok.shape[0], V  # 0-based END column
    enc = m.encode(tok, images)
    seq, lps, gap, zabs, zs = np.zeros((n, D), np.int64), np.zeros((n, D)), np.inf, 0.0, np.zeros((n, D, V + 1))
    for i in range(n):
        st = rows_of(enc, [i])
        hyps = [{"S": 0.0, "tok": [], "lp": [], "z": [], "fin": False}]
        for s in range(D):
            live = [k for k, h in enumerate(hyps) if not h["fin"]]
            cands = [(h["S"], k * (V + 1) + END, k, None, 0.0) for k, h in enumerate(hyps) if h["fin"]]
            if live:
                ids = [hyps[k]["tok"][-1] if s else V + 1 for k in live]
                new, z = m.decode_step(rows_of(st, live), ids)
                zabs = max(zabs, float(np.abs(z).max()))
                l = log_softmax(z)
                for j, k in enumerate(live):  # a row's K + 1 best hold every candidate that can be kept or be the best rejected
                    top = np.argsort(-l[j], kind="stable")[:K + 1]
                    cands += [(hyps[k]["S"] + l[j, c], k * (V + 1) + int(c), k, int(c), l[j, c]) for c in top]
            cands.sort(key=lambda t: (-t[0], t[1]))
            if len(cands) > K:
                gap = min(gap, cands[K - 1][0] - cands[K][0])
            nxt, parents = [], []
            for S, _, k, c, lc in cands[:K]:
                h = hyps[k]
                if c is None:
                    nxt.append({"S": S, "tok": h["tok"] + [0], "lp": h["lp"] + [0.0], "z": h["z"] + [0.0], "fin": True, "src": None})
                else:
                    nxt.append({"S": S, "tok": h["tok"] + [c + 1], "lp": h["lp"] + [lc], "z": h["z"] + [z[live.index(k)]],
                                "fin": c == END, "src": live.index(k)})
            # the survivors' states: a live parent's new state; a finished hypothesis never steps again (any row will do)
            if live:
                st = rows_of(new, [h["src"] if h["src"] is not None else 0 for h in nxt])
            hyps = nxt
        if len(hyps) > 1:
            gap = min(gap, hyps[0]["S"] - hyps[1]["S"])
        seq[i], lps[i] = hyps[0]["tok"], hyps[0]["lp"]
        for s, zr in enumerate(hyps[0]["z"]):
            zs[i, s] = zr
    return seq, lps, float(gap), zabs, zs


def sequence_score(dims, p, tok_row, seq, images=None, arch=3):
    """sum of l over seq (1-based tokens, cut behind the first END), teacher-forced; tok_row is a batch of one sentence"""
    _, D, V, _, _, _ = dims
    m = Model(dims, p, arch)
    st = m.encode(np.asarray(tok_row).reshape(1, -1), images)
    ids, S, out = [V + 1], 0.0, []
    for t in seq:
        st, z = m.decode_step(st, ids)
        S += log_softmax(z)[0, t - 1]
        out.append(t)
        if t == V + 1:
            break
        ids = [t]
    return S, out
