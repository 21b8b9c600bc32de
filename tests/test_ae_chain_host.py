"""The integer rules of an auto-encoder step (novel-vqa_amd/csrc/ae_chain.h), on the CPU: the checker tests/shim/ae_chain_check.cc
is built here with g++ and the host sanitizers (it includes the header the kernels and ae.hip compile) and prints, for one batch,
chain_token of every chain row (q, b), the lookup gradient's index (nu, nch and its four arrays), every row's row_last,
criterion_count and criterion_target, and te.  They are compared with NumPy restatements built on the reference models' own rules:
ae_ref_torch.tmax_of / criterion_targets, ae2_ref_torch.encoder_steps, ae2wp_ref_torch.encoder_steps.

The batch is every row over {0, 1, 2}^3 (B = 27, D = 3, V = 2): all-null rows, interior and leading nulls, full rows whose END
falls at s = D, and more than 16 rows on one token, so the index crosses a chunk boundary."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import ae2_ref_torch
import ae2wp_ref_torch
import ae_ref_torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AE2, BRIDGE, ENC = 1, 2, 4  # AE_CHAIN_*
LK_CHUNK = 16               # NVQA_AE_LK_CHUNK
D, V = 3, 2
BATCH = np.array(list(itertools.product(range(V + 1), repeat=D)), np.int32)  # [27 x 3]
B = len(BATCH)
SHORT = BATCH * (np.arange(D) < 2)  # the same rows with a null last column
ARCHS = {"ae1": 0, "ae2": AE2, "ae2wp": AE2 | ENC, "ae1wp": BRIDGE | ENC}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++")
    assert cxx, "g++ not found"
    out = str(tmp_path_factory.mktemp("ae_chain") / "ae_chain_check")
    r = subprocess.run([cxx, "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "novel-vqa_amd", "csrc"), "-o", out,
                        os.path.join(ROOT, "tests", "shim", "ae_chain_check.cc")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def run(exe, flags, tokens, enc=None, n=None, skip=False, direct=None, V=V):
    tokens = np.asarray(tokens)
    n = len(tokens) if n is None else n
    words = [flags, B, D, V, n, int(skip), int(enc is not None), int(direct is not None)]
    for m in (tokens[:n], None if enc is None else np.asarray(enc)[:n], direct):
        if m is not None:
            words += [int(x) for x in np.asarray(m).ravel()]
    r = subprocess.run([exe], input=" ".join(map(str, words)), capture_output=True, text=True, timeout=60)
    assert not r.stderr, r.stderr[-3000:]  # the sanitizers' reports
    out = {}
    for l in r.stdout.splitlines():
        k, *v = l.split()
        out.setdefault(k, []).append([int(x) for x in v if x.lstrip("-").isdigit()] if k != "bad" else v)
    return r.returncode, out


def fed(col):
    """a token column as the lookup is fed it: 0 -> 1"""
    return np.where(col == 0, 1, col)


def expected_chain(arch, tok, enc, skip, direct=None):
    """(te, [chain rows]): the token of every chain row from the reference models' step counts"""
    tmax = ae_ref_torch.tmax_of(tok)
    start = np.full(B, V + 1)
    if arch == "ae1":
        te, rows = tmax, [fed(tok[:, q]) for q in range(tmax)]
    elif arch == "ae2":
        te = ae2_ref_torch.encoder_steps(tok)
        rows = [np.zeros(B, int), start] + [fed(tok[:, q]) for q in range(te - 2)]
    elif arch == "ae2wp":
        te = ae2wp_ref_torch.encoder_steps(enc)
        rows = [np.zeros(B, int), start] + [fed(enc[:, q]) for q in range(te - 2)]
    else:
        te = 0 if skip else ae_ref_torch.tmax_of(enc)
        rows = [fed(enc[:, q]) for q in range(te)]
    assert len(rows) == te
    rows += [start] + [fed(tok[:, s - 1]) if direct is None else fed(direct) for s in range(1, tmax + 1)]
    return te, [r.tolist() for r in rows]


def expected_index(arch, chain):
    """the counting sort of the chain rows by token (AE2: without the image row): tokens ascending, rows ascending inside a token,
    chunks of LK_CHUNK rows inside one token"""
    r_lo = B if ARCHS[arch] & AE2 else 0
    flat = np.concatenate(chain)[r_lo:]
    lk_tok, lk_tc, lk_start, lk_pos = [], [], [], []
    for v in np.unique(flat):
        rows = np.nonzero(flat == v)[0] + r_lo
        lk_tok.append(int(v))
        lk_tc.append(len(lk_start))
        lk_start += [len(lk_pos) + k for k in range(0, len(rows), LK_CHUNK)]
        lk_pos += rows.tolist()
    return {"nu": [len(lk_tok), len(lk_start)], "lk_tok": lk_tok, "lk_tc": lk_tc + [len(lk_start)],
            "lk_start": lk_start + [len(lk_pos)], "lk_pos": lk_pos}


def check(exe, arch, tok, enc=None, n=None, skip=False, direct=None):
    rc, out = run(exe, ARCHS[arch], tok, enc, n, skip, direct)
    assert rc == 0, out
    n = len(tok) if n is None else n
    tok, src = np.zeros((B, D), np.int64), tok  # as staged: rows from n on are nulls
    tok[:n] = np.asarray(src)[:n]
    if enc is not None:
        enc, src = np.zeros((B, D), np.int64), enc
        enc[:n] = np.asarray(src)[:n]
    assert out["staged"][0] == tok.ravel().tolist()
    te, chain = expected_chain(arch, tok, enc if enc is not None else np.zeros_like(tok), skip)
    tmax = ae_ref_torch.tmax_of(tok)
    assert out["tmax"] == [[tmax, te]]
    assert out["chain"] == chain
    if direct is not None:
        assert out["direct"] == expected_chain(arch, tok, enc if enc is not None else np.zeros_like(tok), skip, direct)[1]
    idx = expected_index(arch, chain)
    assert out["nu"] == [idx["nu"]]
    for k in ("lk_tok", "lk_tc", "lk_start", "lk_pos"):
        assert out[k] == [idx[k]], k
    assert max(np.diff(idx["lk_tc"])) > 1  # a token with more than one chunk
    tg, count = ae_ref_torch.criterion_targets(tok, V)
    rows = np.array(out["row"])
    assert rows[:, 0].tolist() == [ae_ref_torch.tmax_of(tok[b:b + 1]) for b in range(B)]
    assert rows[:, 2:].tolist() == [[tg.get((s, b), -1) for s in range(D + 1)] for b in range(B)]
    assert rows[:, 1].tolist() == (rows[:, 2:] >= 0).sum(axis=1).tolist() and int(rows[:, 1].sum()) == count
    return te


@pytest.mark.parametrize("arch", ["ae1", "ae2"])
def test_one_stream(exe, arch):
    lead = 2 if arch == "ae2" else 0
    assert check(exe, arch, BATCH) == D + lead
    check(exe, arch, BATCH, direct=np.arange(B) % (V + 2))  # decoding: the last picks, 0 .. V + 1
    assert check(exe, arch, SHORT) == 2 + lead               # the last column is null: tmax = 2
    assert check(exe, arch, BATCH[::-1], n=18) == D + lead   # rows from n on are staged as nulls
    assert check(exe, arch, BATCH[::9]) == 1 + lead          # n = 3: (0, 0, 0), (1, 0, 0), (2, 0, 0), so tmax = 1


def test_ae2wp_two_streams(exe):
    assert check(exe, "ae2wp", BATCH, enc=BATCH[::-1]) == D + 2
    assert check(exe, "ae2wp", BATCH, enc=None) == 2  # the null sentence
    assert check(exe, "ae2wp", BATCH, enc=SHORT) == 4


def test_ae1wp_two_streams_and_skip(exe):
    assert check(exe, "ae1wp", BATCH, enc=BATCH[::-1]) == D
    assert check(exe, "ae1wp", BATCH, enc=SHORT) == 2
    assert check(exe, "ae1wp", BATCH, enc=None, skip=True) == 0
    assert check(exe, "ae1wp", BATCH, enc=BATCH[::-1], skip=True) == 0


@pytest.mark.parametrize("value", [-1, V + 1])
def test_invalid_tokens_are_reported_with_their_position(exe, value):
    bad = BATCH.copy()
    bad[14, 1] = value
    bad[20, 0] = value  # the first in row order is reported
    for arch, kw, what in (("ae1", {"tokens": bad}, "tokens"), ("ae2", {"tokens": bad}, "tokens"),
                           ("ae2wp", {"tokens": BATCH, "enc": bad}, "enc_tokens"), ("ae1wp", {"tokens": BATCH, "enc": bad}, "enc_tokens")):
        rc, out = run(exe, ARCHS[arch], **kw)
        assert rc == 2 and out["bad"] == [[what, str(value), "14", "1"]], (arch, out)
    rc, out = run(exe, ARCHS["ae1"], bad, n=14)  # rows from n on are not read
    assert rc == 0 and "bad" not in out
