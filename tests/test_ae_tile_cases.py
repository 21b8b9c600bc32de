"""The preconditions of tests/test_gpu_ae_tiles.py, on the CPU.

Boundary census: a Python restatement of the two host rules of novel-vqa_amd/csrc/ae.hip that decide how a step is cut up --
wgrad()'s tiles -> Z -> slab budget -> kslice -> Z and colsum()'s row splits S -- plus the tile shapes of the
GEMM configurations and the lookup gradient's chunking, evaluated on every case of tests/ae_tile_cases.py.  Each case must
cross the boundaries it is listed for; shrinking one back inside a tile, a slab or a chunk fails here.

Reachability: the f32 CPU evaluation of the same model (ae_bf16_ref_torch.forward with the rounding off and dtype float32)
stays within a quarter of TOL_LOSS / TOL_GRAD of the float64 model on the AE1 / AE2 cases, so the bounds the device is held to
are ones correct f32 arithmetic meets with room; and the two reference files describe one model (1e-12)."""
import numpy as np
import pytest
import torch

import ae2_ref_torch
import ae2wp_ref_torch
import ae_bf16_ref_torch as bf
import ae_ref_torch
import ae_tile_cases as cases

TOL_LOSS = 1e-6  # tests/test_gpu_ae.py, tests/test_gpu_ae2.py
TOL_GRAD = 2e-5

LK_CHUNK = 16  # NVQA_AE_LK_CHUNK


def ceil_div(a, b):
    return (a + b - 1) // b


def tiling(n, t):
    """(number of tiles of t over n, size of the last one)"""
    k = ceil_div(n, t)
    return k, n - (k - 1) * t


# ---- restatement of wgrad() and colsum() -----------------------------------------------------------------------------------------
def slab_floats(case):
    """ae_create: a.slab_floats"""
    E, R = case.dims[3], case.dims[4]
    n = 8 * 4 * R * max(E, R)
    if case.arch == "ae1wp":
        n = max(n, 2 * R * max(2 * R, case.dims[5]))
    return n


def wgrad_plan(M, N, K, budget):
    """wgrad(), f32: returns dict(z0 = Z from the tile count, zb = Z behind the slab budget, kslice, z = slices launched,
    last = rows of the last slice)"""
    tiles = ceil_div(M, 128) * ceil_div(N, 128)
    z0 = max(1, min(16, 512 // max(tiles, 1)))
    zb = z0
    while zb > 1 and zb * M * N > budget:
        zb -= 1
    kslice = ceil_div(ceil_div(K, zb), 32) * 32
    z = ceil_div(K, kslice)
    return {"z0": z0, "zb": zb, "kslice": kslice, "z": z, "last": K - (z - 1) * kslice}


def colsum_plan(M):
    """colsum(): (S row splits, rows per split)"""
    S = min(64, max(1, M // 256))
    rps = ceil_div(M, S)
    return ceil_div(M, rps), rps


# ---- what a step of each arch launches (ae_backward) ----------------------------------------------------------------------------
def chain(case):
    """(encoder chain steps, decoder steps) of the case's batch, by the rules of the arch's float64 model: AE1 tmax(tokens),
    AE2 image + START + tmax, the weak-paired archs from their encoder tokens (AE2_WP: 2 for the null sentence; AE1_WP: none
    when the encoder's state is given)"""
    x = cases.inputs(case.name)
    if case.arch == "ae1":
        te = ae_ref_torch.tmax_of(x["tok"])
    elif case.arch == "ae2":
        te = ae2_ref_torch.encoder_steps(x["tok"])
    elif case.arch == "ae2wp":
        te = ae2wp_ref_torch.encoder_steps(x["et"])
    else:
        te = 0 if x["et"] is None else ae_ref_torch.tmax_of(x["et"])
    return te, ae_ref_torch.tmax_of(x["tok"]) + 1


def products(case):
    """{name: (M, N, K)} of the step's wgrad() calls and {name: rows} of its colsum() calls"""
    B, D, V, E, R = case.dims[:5]
    L = 1 if case.arch == "ae1wp" else case.dims[5]
    te, nd = chain(case)
    w, c = {"w_proj": (V + 1, R, nd * B)}, {"b_proj": nd * B}
    for l in range(L):
        n_in = E if l == 0 else R
        for part, steps in (("enc", te), ("dec", nd)):
            if steps == 0:
                continue  # AE1_WP with the encoder skipped
            w[f"{part}{l}_w_i2h"] = (4 * R, n_in, steps * B)
            w[f"{part}{l}_w_h2h"] = (4 * R, R, steps * B)
            c[f"{part}{l}_b"] = steps * B
    if case.arch == "ae2wp":
        w["w_p"], c["b_p"] = (E, case.dims[6], B), B
    if case.arch == "ae1wp":
        w["w_q"], w["w_v"], c["b_q"], c["b_v"] = (2 * R, 2 * R, B), (2 * R, case.dims[5], B), B, B
    return w, c


def plans(case):
    w, c = products(case)
    budget = slab_floats(case)
    return {k: wgrad_plan(*v, budget) for k, v in w.items()}, {k: colsum_plan(v) for k, v in c.items()}


def lookup_rows(case):
    """{token: rows} of the lookup gradient's index (ae_upload): every chain row but AE2's image row, 0 -> 1, START = V + 1"""
    B, D, V = case.dims[:3]
    tok = cases.inputs(case.name)["tok"]
    fed = np.where(tok == 0, 1, tok).ravel()
    ids = np.concatenate([fed, fed, np.full(B * (2 if case.arch == "ae2" else 1), V + 1)])
    u, n = np.unique(ids, return_counts=True)
    return dict(zip(u.tolist(), n.tolist()))


# ---- the table of tests/ae_tile_cases.py, entry by entry --------------------------------------------------------------------------
def test_every_case_leaves_the_first_tile_slab_and_chunk():
    for case in cases.CASES:
        B = case.dims[0]
        wp, _ = plans(case)
        assert tiling(B, 64)[0] >= 2 and tiling(B, 64)[1] < 64, case.name  # a full gate row tile, then a partial one
        assert any(p["last"] % 32 for p in wp.values()), case.name         # a last K slice that is no multiple of 32 rows
        if case.arch in ("ae1", "ae2"):
            rows = lookup_rows(case)
            assert rows[case.dims[2] + 1] > LK_CHUNK, case.name            # START has more than one chunk
    for name in ("b136_l2_drop", "b200_l1", "b264_v1100_drop", "ae2_b136_l2_drop_img", "ae2_b200_null_img"):
        wp, cp = plans(cases.BY_NAME[name])
        assert max(p["z"] for p in wp.values()) > 4, name
        assert max(s for s, _ in cp.values()) > 1, name


def test_b136_l2_drop_boundaries():
    case = cases.BY_NAME["b136_l2_drop"]
    B, D, V, E, R, L = case.dims
    te, nd = chain(case)
    wp, cp = plans(case)
    # gate GEMM (AeCfgGates 64 rows x 64 units): 3 row tiles (64, 64, 8) x 2 unit tiles (64, 8)
    assert tiling(B, 64) == (3, 8) and tiling(R, 64) == (2, 8)
    # ae_i2h (AeCfgWide 128 x 128, BK = 32): M = 816 in 7 tiles, the last of 48; N = 288 in 3, the last of 32; K = 40 = 32 + 8
    assert te * B == 816 and tiling(816, 128) == (7, 48) and tiling(4 * R, 128) == (3, 32) and E % 32 == 8
    # dW_proj: the slab budget cuts Z from 16 to 3; slices of 320, the last of 312
    assert wp["w_proj"] == {"z0": 16, "zb": 3, "kslice": 320, "z": 3, "last": 312}
    assert 4 * (V + 1) * R > slab_floats(case) >= 3 * (V + 1) * R  # the budget binds
    # dW_i2h of the encoder's layer 0: 13 slices of 64, the last of 48; dW_h2h of the decoder (K = 952): 8 of 128, the last of 56
    assert (wp["enc0_w_i2h"]["z"], wp["enc0_w_i2h"]["kslice"], wp["enc0_w_i2h"]["last"]) == (13, 64, 48)
    assert nd * B == 952
    for l in range(L):
        assert (wp[f"dec{l}_w_h2h"]["z"], wp[f"dec{l}_w_h2h"]["kslice"], wp[f"dec{l}_w_h2h"]["last"]) == (8, 128, 56)
    assert cp["dec0_b"] == (3, 318) and cp["b_proj"][0] == 3  # colsum: S = 3 over 952 rows
    # START: 9 chunks, the last of 8 rows
    assert tiling(lookup_rows(case)[V + 1], LK_CHUNK) == (9, 8)


def test_b200_l1_boundaries():
    case = cases.BY_NAME["b200_l1"]
    B, D, V, E, R, L = case.dims
    wp, cp = plans(case)
    assert tiling(B, 64) == (4, 8)
    assert tiling(R, 64) == (3, 4)   # gate GEMM: 3 unit tiles, the last of 4 units
    assert tiling(R, 32) == (5, 4)   # AeCfgStepBwd (64 x 32): 5 column tiles, the last of 4
    assert E % 32 == 4 and E % 64 == 4 and R % 32 == 4 and R % 64 == 4  # K tails of 4 with BK = 32 and BK = 64
    assert (wp["w_proj"]["z"], wp["w_proj"]["kslice"], wp["w_proj"]["last"]) == (13, 96, 48)
    assert wp["w_proj"]["zb"] < wp["w_proj"]["z0"]
    assert cp["b_proj"] == (4, 300) and cp["dec0_b"] == (4, 300)  # S = 4 over 1200 rows


def test_b264_v1100_drop_boundaries():
    case = cases.BY_NAME["b264_v1100_drop"]
    B, D, V, E, R, L = case.dims
    wp, cp = plans(case)
    rows = (D + 1) * B
    assert rows == 1056 and rows > 256 * 4           # k_ae_loss: every thread sums more than one row loss
    assert tiling(V + 1, 128) == (9, 77)             # projection: 9 column tiles, the last of 77
    assert (V + 1 + 3) // 4 * 4 - (V + 1) == 3       # ldl = 1104: three padding columns
    assert (V + 1) // 32 == 34 and (V + 1) % 32 == 13  # EpiAeTop dgrad: K = 1101 = 34 x 32 + 13
    # dW_proj: M = 1101 through A_MC in 9 row tiles; not even two slabs fit the budget, so the one slice goes straight out
    assert tiling(V + 1, 128)[0] * tiling(R, 128)[0] == 9 and (wp["w_proj"]["z0"], wp["w_proj"]["z"]) == (16, 1)
    assert (wp["enc0_w_i2h"]["z"], wp["enc0_w_i2h"]["last"]) == (7, 24)
    assert ceil_div(V + 1, 256) == 5 and cp["b_proj"] == (4, 264)  # b_proj colsum: 5 column blocks, S = 4 over 1056 rows


def test_b70_v3_drop_every_lookup_token_is_multi_chunk():
    case = cases.BY_NAME["b70_v3_drop"]
    rows = lookup_rows(case)
    assert case.dims[2] + 1 == 4 and sorted(rows) == [1, 2, 3, 4]
    assert min(rows.values()) > 2 * LK_CHUNK, rows
    assert any(n % LK_CHUNK for n in rows.values())


def test_ae2_cases_boundaries():
    case = cases.BY_NAME["ae2_b136_l2_drop_img"]
    B, D, V, E, R, L = case.dims
    rows = lookup_rows(case)
    assert rows[V + 1] == 2 * B and tiling(2 * B, LK_CHUNK) == (17, 16)  # START of the encoder and the decoder: 17 chunks
    assert sum(rows.values()) == (chain(case)[0] - 1 + chain(case)[1]) * B  # every chain row but the image's
    assert sum(n > LK_CHUNK for n in rows.values()) >= 2                 # the padding token too
    assert cases.inputs(case.name)["img"] is not None
    wp, cp = plans(case)
    assert wp["enc0_w_i2h"]["z"] > 4 and cp["enc0_b"][0] > 1
    case = cases.BY_NAME["ae2_b200_null_img"]
    assert cases.inputs(case.name)["img"] is None and tiling(case.dims[0], 64) == (4, 8) and tiling(case.dims[4], 64) == (3, 4)


def test_weak_paired_cases_boundaries():
    for name in ("wp_b136_same_drop", "wp_b136_null"):
        case = cases.BY_NAME[name]
        B, D, V, E, R, L, I = case.dims
        wp, _ = plans(case)
        # ae_wp_project: M = 136 (two row tiles of AeCfgWide), K = 100 = 3 x 32 + 4; dW_p: K = B = 136 in 5 slices, the last of 8
        assert tiling(B, 128) == (2, 8) and I % 32 == 4
        assert (wp["w_p"]["z"], wp["w_p"]["kslice"], wp["w_p"]["last"]) == (5, 32, 8)
    assert "enc0_w_i2h" in plans(cases.BY_NAME["wp_b136_null"])[0]  # the null sentence still runs the image row and START
    for name in ("ae1wp_b136_same_drop", "ae1wp_b136_skip"):
        case = cases.BY_NAME[name]
        B, D, V, E, R, I = case.dims
        wp, _ = plans(case)
        # the bridge and its backward above one row tile: 3 row tiles of 64 (AeCfgStepBwd, EpiAe1wpDj), 2 of 128 (AeCfgWide,
        # EpiAe1wpDf), with 2R = 144 and R = 72 leaving partial column tiles
        assert tiling(B, 64) == (3, 8) and tiling(B, 128) == (2, 8) and tiling(R, 32) == (3, 8) and tiling(2 * R, 128) == (2, 16)
        assert (wp["w_q"]["z"], wp["w_q"]["last"]) == (5, 8) and (wp["w_v"]["z"], wp["w_v"]["last"]) == (5, 8)
    assert "enc0_w_i2h" not in plans(cases.BY_NAME["ae1wp_b136_skip"])[0]


def test_tie_placements_cover_lanes_waves_and_strides():
    """k_ae_argmax runs 256 threads: column c sits in thread c % 256, wave (c % 256) // 64, stride iteration c // 256"""
    where = [((lo % 256) // 64, lo // 256, (hi % 256) // 64, hi // 256) for lo, hi in cases.TIE_PAIRS]
    assert where[0] == (0, 0, 0, 0) and cases.TIE_PAIRS[0][1] == cases.TIE_PAIRS[0][0] + 1  # neighbouring lanes
    assert where[1] == (0, 0, 1, 0)                                                         # two waves
    assert where[2] == (0, 0, 0, 1) and cases.TIE_PAIRS[2][1] - cases.TIE_PAIRS[2][0] == 256  # the same thread, one stride later
    assert where[3] == (3, 0, 0, 1)                                                         # lo in wave 3, hi in wave 0 of the next stride
    assert all(lo < hi < cases.TIE_DIMS[2] + 1 for lo, hi in cases.TIE_PAIRS)


@pytest.mark.parametrize("lo_col,hi_col", cases.TIE_PAIRS, ids=["%d_%d" % p for p in cases.TIE_PAIRS])
def test_tied_pair_wins_every_step_of_the_float64_model(lo_col, hi_col):
    """the precondition of the GPU test: the two columns are the same parameters and one of them is the float64 model's argmax at
    every row and step, so the device's samples are decided by its tie rule alone"""
    B, D, V, E, R, L = cases.TIE_DIMS
    p, tok = cases.tie_inputs(lo_col, hi_col)
    lay = ae_ref_torch.layout(*cases.TIE_DIMS)
    W = p[lay["w_proj"][0]:lay["w_proj"][0] + (V + 1) * R].reshape(V + 1, R)
    b = p[lay["b_proj"][0]:lay["b_proj"][0] + V + 1]
    assert np.array_equal(W[lo_col], W[hi_col]) and b[lo_col] == b[hi_col] == cases.TIE_BIAS
    assert np.abs(np.delete(b, [lo_col, hi_col])).max() + R * 0.08 < cases.TIE_BIAS - R * 0.08  # |h| < 1, |W| <= 0.08
    got = ae_ref_torch.greedy(cases.TIE_DIMS, p.astype(np.float64), tok)
    assert set(np.unique(got).tolist()) <= {lo_col + 1, hi_col + 1}


# ---- reachability of the tolerances ---------------------------------------------------------------------------------------------
def relmax(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))


@pytest.mark.parametrize("name", [c.name for c in cases.CASES if c.arch in ("ae1", "ae2")])
def test_f32_arithmetic_reaches_a_quarter_of_the_tolerances(name):
    """Measured on these cases: loss <= 1.13e-7 relative (b264_v1100_drop), gradients <= 4.65e-7 of the tensor's largest element
    (d(images) of ae2_b136_l2_drop_img): 9 x and 43 x under the bounds; the two reference files agree to 4e-15."""
    case, x = cases.BY_NAME[name], cases.inputs(name)
    want = cases.reference(name)
    kw = dict(images=x.get("img"), ae2=case.arch == "ae2", dr=x["dr"], rounded=False)
    same = bf.forward(case.dims, x["p"], x["tok"], **kw)
    f32 = bf.forward(case.dims, x["p"], x["tok"], dtype=torch.float32, **kw)
    assert abs(same["loss"] - want["loss"]) <= 1e-12 * abs(want["loss"])
    assert np.abs(same["grads"] - want["grads"]).max() <= 1e-12
    el = abs(f32["loss"] - want["loss"]) / abs(want["loss"])
    eg = {k: relmax(f32["grads"][o:o + n], want["grads"][o:o + n]) for k, (o, n) in
          ((k, v) for k, v in cases.layout(case).items() if not k.startswith("_"))}
    if case.arch == "ae2":
        assert np.abs(same["dimages"] - want["dimages"]).max() <= 1e-12
        eg["dimages"] = relmax(f32["dimages"], want["dimages"])
    print(name, "loss %.3g" % el, "worst %s %.3g" % (max(eg, key=eg.get), max(eg.values())))
    assert el <= 0.25 * TOL_LOSS, el
    assert max(eg.values()) <= 0.25 * TOL_GRAD, eg
