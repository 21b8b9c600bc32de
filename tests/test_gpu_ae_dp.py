"""Data-parallel text auto-encoder training (nvqa_ae_comm_init) with TWO RANKS that hold DIFFERENT half-batches.

Two processes = two ranks on device 0 (librccl refuses two ranks on one device), exchanging through the stand-in's
shared-memory mode (tests/shim, NCCL_SHIM_SHM: a real stream-ordered all-reduce between processes), launched as
tests/test_gpu_dp.py launches its ranks.  Everything else is the library's own path: the count's all-reduce under the forward
pass, the rank weight n_r world / N in the criterion's kernels, one all-reduce per bucket, the closing {status, loss} exchange,
1/world and the clamp in k_adam.

The halves have criterion counts 13 and 23, so the mean of the ranks' means is NOT the global batch's gradient (off by 0.45 to
0.49 of a tensor's largest element on these inputs, in the float64 models); both halves hold a full-length row, so both have
tmax = D and the float64 model run on the CONCATENATED batch is the reference.  One launch per arch runs everything (three Adam
steps without dropout, one step with dropout and distinct rank seeds, then rank 0 evaluates alone after rank 1 has closed its
context); the tests share its record, and a launch that failed is not started again."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the project's bounds for the f32 auto-encoder step (tests/test_gpu_ae.py)
TOL_LOSS = 1e-6
TOL_GRAD = 2e-5
TOL_PARAM = 1e-6

B, D, V, E, R = 4, 5, 19, 8, 8           # B per rank
LENS = ([5, 1, 1, 2], [5, 5, 4, 5])      # criterion counts 13 and 23; both ranks have a full-length row: tmax = D
COUNTS = (13, 23)
ARCHS = {"ae1_l2": (3, 2), "ae2_l1": (4, 1)}
STEPS = 3
LR, B1, B2, EPS, WD, CLAMP = 2e-2, 0.8, 0.999, 1e-8, 1e-2, 1e-3
DROP_SEED, DROP_STEP = 77, 4             # rank r draws its masks from DROP_SEED + 1000 r


def _layout_total(L):
    n = 0
    for _ in range(2):
        for l in range(L):
            n += 4 * R * (E if l == 0 else R) + 4 * R + 4 * R * R + 4 * R
    return n + (V + 1) * R + (V + 1) + (V + 1) * E


def _inputs(name):
    """parameters, per-step tokens [step][rank] and per-rank images of one case: the same in the ranks and in the checker"""
    arch, L = ARCHS[name]
    rng = np.random.default_rng(1000 + arch)
    p = rng.uniform(-0.08, 0.08, _layout_total(L)).astype(np.float32)
    toks = []
    for _ in range(STEPS + 1):
        per_rank = []
        for lens in LENS:
            t = np.zeros((B, D), np.int32)
            for b, n in enumerate(lens):
                t[b, :n] = rng.integers(1, V + 1, n)
            per_rank.append(t)
        toks.append(per_rank)
    imgs = [rng.standard_normal((B, E)).astype(np.float32) for _ in range(2)] if arch == 4 else [None, None]
    return p, toks, imgs


# ---------------------------------------------------------------------------------------------------------------------
# one rank, as a process of its own
# ---------------------------------------------------------------------------------------------------------------------
def _wait_for(path, what):
    t0 = time.time()
    while not os.path.exists(path):
        assert time.time() - t0 < 60, what
        time.sleep(0.02)


def _main_rank(name, rank, out_dir):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    arch, L = ARCHS[name]
    p, toks, imgs = _inputs(name)
    img = imgs[rank]
    dims = pkg.binding.Dims(arch, B, D, V, E, R, L, 0, 0, 0)
    ctx = pkg.binding.Context(dims, 0)
    ctx.set_params(p)
    idf = os.path.join(out_dir, "comm_id.bin")
    if rank == 0:
        cid = ctx.comm_unique_id()
        with open(idf + ".tmp", "wb") as f:
            f.write(cid)
        os.replace(idf + ".tmp", idf)
    else:
        _wait_for(idf, "rank 0 never published the communicator id")
        cid = open(idf, "rb").read()
    ctx.ae_comm_init(rank, 2, cid)
    rec = {}

    def step(it, dr):
        rec[f"x{it}"] = ctx.get_params()
        if arch == 4:
            loss, dimg = ctx.ae_step(toks[it][rank], dr, images=img, want_dimages=True)
            rec[f"dimg{it}"] = dimg
        else:
            loss = ctx.ae_step(toks[it][rank], dr)
        rec[f"loss{it}"] = np.float32(loss)
        rec[f"g{it}"] = ctx.get_grads()

    for it in range(STEPS):
        step(it, None)
        rec[f"stats{it}"] = np.array(ctx.adam_update(LR, B1, B2, EPS, WD, CLAMP, stats=True), np.float64)
    rec[f"x{STEPS}_after"] = ctx.get_params()
    step(STEPS, pkg.binding.Dropout(1, 0.5, DROP_SEED + 1000 * rank, DROP_STEP))
    done = os.path.join(out_dir, "rank1_closed")
    if rank == 1:
        ctx.close()
        open(done, "w").close()
    else:
        # rank 1 is gone: evaluate must not wait for it (no collective), and gives what a context without a communicator gives
        _wait_for(done, "rank 1 never closed its context")
        x = ctx.get_params()
        rec["eval_alone"] = np.float32(ctx.ae_evaluate(toks[0][0], images=img)[0])
        ctx.close()
        fresh = pkg.binding.Context(dims, 0)
        fresh.set_params(x)
        rec["eval_fresh"] = np.float32(fresh.ae_evaluate(toks[0][0], images=img)[0])
        fresh.close()
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), **rec)


# ---------------------------------------------------------------------------------------------------------------------
# the checker
# ---------------------------------------------------------------------------------------------------------------------
_RUNS = {}


def _launch(name, tmp_path_factory):
    """both ranks of one case, ONCE per session, whatever its outcome: {rank: record}.  A launch that failed or hung is
    recorded as such and never started again: the other tests of the case fail at once from the record."""
    if name not in _RUNS:
        try:
            _RUNS[name] = _launch_once(name, tmp_path_factory)
        except BaseException as e:  # (pytest.fail raises an Exception subclass outside the Exception tree)
            _RUNS[name] = e
            raise
    if isinstance(_RUNS[name], BaseException):
        pytest.fail(f"the 2-rank run of {name} failed earlier in this session and is not started again: {_RUNS[name]!r}")
    return _RUNS[name]


def _launch_once(name, tmp_path_factory):
    shim = os.path.join(os.path.dirname(os.path.abspath(__file__)), "shim", "libnccl_shim.so")
    assert os.path.exists(shim), "tests/shim/libnccl_shim.so missing: run __graft_entry__.build()"
    out = str(tmp_path_factory.mktemp("ae_dp_" + name))
    env = dict(os.environ, NVQA_RCCL_LIB=shim, NCCL_SHIM_SHM=f"/nvqa_aedp_{name}_{os.getpid()}", NCCL_SHIM_SHM_MB="1",
               NCCL_SHIM_DELAY_US="0", NCCL_SHIM_CUS="0", NVQA_QUIET="1")
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), name, str(r), out], env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=180) for p in procs]
    except subprocess.TimeoutExpired:
        for p in procs:
            p.kill()
        for p in procs:
            p.wait()
        _unlink_segment(env["NCCL_SHIM_SHM"])
        pytest.fail("2-rank shared-memory run did not complete")
    if rcs != [0, 0]:
        _unlink_segment(env["NCCL_SHIM_SHM"])  # (rank 0 unlinks it when it closes its context; a rank that died did not)
    assert rcs == [0, 0], rcs
    return {r: dict(np.load(os.path.join(out, f"rank{r}.npz"))) for r in range(2)}


def _unlink_segment(name):
    try:
        os.unlink("/dev/shm" + name)
    except OSError:
        pass


def _ref_of(arch):
    import ae2_ref_torch
    import ae_ref_torch
    return ae2_ref_torch if arch == 4 else ae_ref_torch


def _ref_forward(arch, dims, x, tok, img, dr=None):
    ref = _ref_of(arch)
    if arch == 4:
        return ref.forward(dims, x.astype(np.float64), tok, images=img, dr=dr, train=True)
    return ref.forward(dims, x.astype(np.float64), tok, dr=dr, train=True)


def _seg_errors(lo, got, want):
    out = {}
    for k, v in lo.items():
        if k.startswith("_"):
            continue
        o, n = v
        a, b = np.asarray(got[o:o + n], np.float64), np.asarray(want[o:o + n], np.float64)
        out[k] = float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-30))
    return out


@pytest.mark.parametrize("name", list(ARCHS))
def test_unequal_counts_global_batch_equivalence(pkg, tmp_path_factory, name):
    """Three Adam steps, dropout off, a clamp that bites and weight decay: at every step both ranks hold the same gradient and
    parameters bit for bit; gradient and loss are the float64 model's on the concatenated batch at the parameters the device
    holds; the parameters follow ref.Adam fed the returned gradient."""
    import ae_ref_torch
    arch, L = ARCHS[name]
    run = _launch(name, tmp_path_factory)
    _, toks, imgs = _inputs(name)
    lo = ae_ref_torch.layout(2 * B, D, V, E, R, L)
    assert lo["_total"] == _layout_total(L)
    mirror = ae_ref_torch.Adam(lo["_total"])
    img = None if arch == 3 else np.concatenate(imgs)
    bites = 0.0
    for it in range(STEPS):
        x, g = run[0][f"x{it}"], run[0][f"g{it}"]
        assert np.array_equal(x, run[1][f"x{it}"]), (it, "parameters differ between the ranks")
        assert np.array_equal(g, run[1][f"g{it}"]), (it, "gradients differ between the ranks")
        assert run[0][f"loss{it}"] == run[1][f"loss{it}"], (it, "losses differ between the ranks")
        assert np.array_equal(run[0][f"stats{it}"], run[1][f"stats{it}"]), (it, "Adam statistics differ between the ranks")
        tok = np.concatenate(toks[it])
        want = _ref_forward(arch, (2 * B, D, V, E, R, L), x, tok, img)
        assert want["n"] == sum(COUNTS) and want["tmax"] == D
        el = abs(float(run[0][f"loss{it}"]) - want["loss"]) / abs(want["loss"])
        eg = _seg_errors(lo, g, want["grads"])
        print(f"{name} step {it}: loss rel {el:.2e}, gradient rel max {max(eg.values()):.2e} ({max(eg, key=eg.get)})")
        assert el < TOL_LOSS, (it, float(run[0][f"loss{it}"]), want["loss"])
        assert max(eg.values()) < TOL_GRAD, (it, eg)
        if arch == 4:  # each rank's rows of d(global loss)/d(images), times world: scaled as the rank's gradient before the exchange
            for r in range(2):
                wd = 2.0 * want["dimages"][r * B:(r + 1) * B]
                ed = float(np.abs(run[r][f"dimg{it}"] - wd).max() / np.abs(wd).max())
                assert ed < TOL_GRAD, (it, r, ed)
        x_after = run[0][f"x{it + 1}"] if it + 1 < STEPS else run[0][f"x{STEPS}_after"]
        x_want, wnorm, wcount = mirror.update(x, g, LR, B1, B2, EPS, WD, CLAMP)
        ep = float(np.abs(x_after - x_want).max())
        assert ep < TOL_PARAM, (it, ep)
        norm, count = run[0][f"stats{it}"]
        assert abs(norm - wnorm) / wnorm < 1e-6
        assert abs(count - wcount) <= max(2, wcount // 1000)
        bites = max(bites, float(np.mean(np.abs(g) > CLAMP)))
    assert bites > 0.01, "the test clamp must bite"
    assert np.array_equal(run[0][f"x{STEPS}_after"], run[1][f"x{STEPS}_after"])


@pytest.mark.parametrize("name", list(ARCHS))
def test_dropout_with_distinct_rank_seeds(pkg, tmp_path_factory, name):
    """One step with dropout: masks are keyed by the rank-local element and each rank's own seed, so the reference is
    sum_r n_r G_r / N with G_r the float64 model on rank r's half under rank r's key."""
    import ae_ref_torch
    arch, L = ARCHS[name]
    run = _launch(name, tmp_path_factory)
    _, toks, imgs = _inputs(name)
    it = STEPS
    x, g = run[0][f"x{it}"], run[0][f"g{it}"]
    assert np.array_equal(x, run[1][f"x{it}"]) and np.array_equal(g, run[1][f"g{it}"])
    assert run[0][f"loss{it}"] == run[1][f"loss{it}"]
    lo = ae_ref_torch.layout(B, D, V, E, R, L)
    parts = []
    for r in range(2):
        dr = pkg.binding.Dropout(1, 0.5, DROP_SEED + 1000 * r, DROP_STEP)
        parts.append(_ref_forward(arch, (B, D, V, E, R, L), x, toks[it][r], imgs[r], dr=dr))
        assert parts[r]["n"] == COUNTS[r] and parts[r]["tmax"] == D
    N = float(sum(COUNTS))
    want_g = sum(COUNTS[r] * parts[r]["grads"] for r in range(2)) / N
    want_l = sum(COUNTS[r] * parts[r]["loss"] for r in range(2)) / N
    el = abs(float(run[0][f"loss{it}"]) - want_l) / abs(want_l)
    eg = _seg_errors(lo, g, want_g)
    print(f"{name} dropout step: loss rel {el:.2e}, gradient rel max {max(eg.values()):.2e} ({max(eg, key=eg.get)})")
    assert el < TOL_LOSS, (float(run[0][f"loss{it}"]), want_l)
    assert max(eg.values()) < TOL_GRAD, eg
    # the plain mean of the ranks' gradients is far outside the bound: the test can tell the two apart
    naive = _seg_errors(lo, 0.5 * (parts[0]["grads"] + parts[1]["grads"]), want_g)
    assert max(naive.values()) > 100 * TOL_GRAD


@pytest.mark.parametrize("name", list(ARCHS))
def test_a_rank_evaluates_alone(tmp_path_factory, name):
    """After the steps rank 0 called ae_evaluate while rank 1 had already closed its context: the call returned (the launch did
    not time out) with the loss of a fresh context without a communicator that holds the same parameters."""
    run = _launch(name, tmp_path_factory)
    assert np.isfinite(run[0]["eval_alone"])
    assert run[0]["eval_alone"] == run[0]["eval_fresh"]


if __name__ == "__main__":
    _main_rank(sys.argv[1], int(sys.argv[2]), sys.argv[3])
