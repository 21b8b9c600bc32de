"""The six-term bf16 weight-gradient kernel of the f32 mode (csrc/wgrad_split.h: an f32 product as six
v_mfma_f32_16x16x32_bf16 terms, smallest first, one f32 accumulator).

* The kernel alone, through the checker tests/shim/wgrad_split_check.hip (compiled here: it includes the library's header):
  the step's shapes -- 2048 x 512 and 2048 x 200, K = 13312 and 13000, split-K 8 and 16, one ragged profile, and 256 steps of 32 rows (the most the kernel's tables take) -- against an f64
  product of the UNROUNDED operands, beside an f32 fmaf chain on the same operands.  Six terms must stay within 1.5 x of the
  chain's L2-relative and 4 x of its max-relative error (the margins of tests/test_wgrad_split_numerics.py's emulation; how
  the MFMA sums its 32 products is the unknown measured here), and a second run must give the same bits.
* The whole step both ways, NVQA_WGRAD_SPLIT=0 and =1, headline shape, all lengths 26 and ragged: loss and every gradient
  segment but the LSTM weights bit-identical, the LSTM weight segments within TOL_GRAD of the f64 oracle and within 2 x of
  the f32 route's own error on the same step.
Measured (MI355X): checker ratios L2 1.10-1.21, max 0.47-1.89; step: the four LSTM weight segments 1.0-1.2e-6 from the
oracle on both routes (ratios 0.93-1.05); profiles/wgrad_split_ab.json."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from util import gdims, gdrop, grad_errors, record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FULL1 = dict(arch=1, B=512, T=26, V=14773, E=200, R=512, L=2, I=4096, C=1024, A=1000)
TOL_GRAD = 2e-5  # tests/test_gpu_parity_r2.py


def test_kernel_against_f64_product_and_f32_chain(tmp_path):
    exe = str(tmp_path / "wgrad_split_check")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "shim", "wgrad_split_check.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "600", exe], capture_output=True, text=True, timeout=660)
    print(r.stdout)
    lines = [l for l in r.stdout.splitlines() if "six terms" in l]
    ratios = [(float(m.group(1)), float(m.group(2))) for m in (re.search(r"ratio L2 ([0-9.eE+-]+) max ([0-9.eE+-]+),", l) for l in lines)]
    record("wgrad_split_check", {"cases": len(lines), "worst_ratio_l2": max(a for a, _ in ratios) if ratios else None,
                                 "worst_ratio_max": max(b for _, b in ratios) if ratios else None})
    assert len(lines) == 11, r.stdout + r.stderr
    assert all("rerun identical" in l for l in lines), r.stdout
    assert all(a <= 1.5 and b <= 4.0 for a, b in ratios), r.stdout
    assert r.returncode == 0 and all(l.endswith("OK") for l in lines), r.stdout + r.stderr


def _ctx(pkg, d, env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return pkg.binding.Context(gdims(pkg, d), 0)  # the switches are read at nvqa_create
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.mark.parametrize("full_length", [True, False], ids=["all26", "ragged"])
def test_step_both_routes(pkg, orc, full_length):
    d = orc.make_dims(**FULL1)
    params = orc.synth_params(d)
    tok, lens, img, lab = orc.synth_batch(d, full_length=full_length)
    dr = orc.Dropout(1, 0.5, 123, 7)
    ref = orc.Oracle(np.float64).step(d, params, tok, lens, img, lab, dr)
    out = {}
    for split in ("0", "1"):
        ctx = _ctx(pkg, d, {"NVQA_WGRAD_SPLIT": split})
        ctx.set_params(params)
        loss = ctx.step(tok, lens, img, lab, gdrop(pkg, dr))
        out[split] = (loss, np.array(ctx.get_grads(), copy=True))
        ctx.close()
    (loss0, g0), (loss1, g1) = out["0"], out["1"]
    assert loss0 == loss1
    lo = orc.layout(d)
    lstm_w = [k for k in lo if not k.startswith("_") and (k.startswith("w_i2h") or k.startswith("w_h2h"))]
    assert len(lstm_w) == 2 * d.L
    for k, v in lo.items():
        if k.startswith("_") or k in lstm_w:
            continue
        o, n = v
        assert np.array_equal(g0[o:o + n], g1[o:o + n]), f"{k} differs between the two routes"
    e0, e1 = grad_errors(orc, d, g0, ref["grads"]), grad_errors(orc, d, g1, ref["grads"])
    name = "wgrad_split_step_" + ("all26" if full_length else "ragged")
    record(name, {"f32_route": {k: e0[k] for k in lstm_w}, "split_route": {k: e1[k] for k in lstm_w}})
    print(name, {k: (e0[k], e1[k]) for k in lstm_w})
    for k in lstm_w:
        o, n = lo[k]
        assert not np.array_equal(g0[o:o + n], g1[o:o + n]), f"{k}: the switch did not change the route"
        assert max(e1[k]) <= TOL_GRAD, (k, e1[k])
        assert e1[k][0] <= 2.0 * e0[k][0] and e1[k][1] <= 2.0 * e0[k][1], (k, e0[k], e1[k])
