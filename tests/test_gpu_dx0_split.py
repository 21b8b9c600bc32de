"""The six-term bf16 d(layer-0 input) kernel of the f32 mode (csrc/dx0_split.h: dX0 = dG0 W_i2h0 with every f32 product as
six v_mfma_f32_16x16x32_bf16 terms, dG straight from global memory into the fragment registers, the three bf16 images of
W^T staged through LDS).

* The kernel alone, through the checker tests/shim/dx0_split_check.hip (compiled here: it includes the library's headers
  and makes the images with the library's TransposeJob code): the smallest shapes at which each mechanism can go wrong --
  one tile and one K step; a partial last row tile with a half-filled 13th column tile; narrow N with a long K; two column
  blocks; full, partly skipped and empty row segments; a segment height that is no multiple of the tile (nothing skipped);
  a padded leading dimension; N in the second column block; M one under and one over the workgroup height; two segments
  in one workgroup; segments of two row blocks (the rotation of row blocks inside a segment) -- each into a NaN-prefilled output, against the f64 product of the UNROUNDED operands
  beside an f32 fmaf chain.  Six terms must stay within 1.5 x of the chain's L2-relative and 4 x of its max-relative error
  (tests/test_dx0_split_numerics.py), every row that must be written is written, skipped tiles are still NaN, and a second
  run gives the same bits.
* The whole step through the public entry, NVQA_DX0_KERNEL=1 (the f32 MFMA GEMM) against the default, arch1 (E = 200) and
  arch2 (E = 512) at a small ragged shape: the loss and every gradient segment that dX0 does not feed bit-identical, the
  segments it feeds (arch1: w_e, b_e; arch2: w_lk, w_p, b_p) different, within TOL_GRAD of the f64 oracle and within 2 x
  of the old route's own error, and the route counter (nvqa_dx0_routes) showing which kernel ran.
Measured (MI355X): checker ratios max 0.20-1.12, L2 0.33-0.76; launch and step times in profiles/dx0_split_ab.json."""
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
TOL_GRAD = 2e-5  # tests/test_gpu_parity_r2.py
N_CASES = 12
SMALL = {1: dict(arch=1, B=32, T=5, V=50, E=200, R=64, L=2, I=64, C=48, A=12),
         2: dict(arch=2, B=32, T=5, V=50, E=512, R=64, L=2, I=64, C=4, A=12)}
FED = {1: ("w_e", "b_e"), 2: ("w_lk", "w_p", "b_p")}  # the segments dX0 feeds


def test_kernel_against_f64_product_and_f32_chain(tmp_path):
    exe = str(tmp_path / "dx0_split_check")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "shim", "dx0_split_check.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    lines = [l for l in r.stdout.splitlines() if "six terms" in l]
    ratios = [(float(m.group(1)), float(m.group(2))) for m in (re.search(r"\(([0-9.eE+-]+) x, ([0-9.eE+-]+) x\)", l) for l in lines)]
    record("dx0_split_check", {"cases": len(lines), "worst_ratio_max": max(a for a, _ in ratios) if ratios else None,
                               "worst_ratio_l2": max(b for _, b in ratios) if ratios else None})
    assert len(lines) == N_CASES, r.stdout + r.stderr
    assert all("unwritten 0," in l and "skipped rows touched 0," in l and "rerun identical" in l for l in lines), r.stdout
    assert all(a <= 4.0 and b <= 1.5 for a, b in ratios), r.stdout
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


@pytest.mark.parametrize("arch", [1, 2], ids=["arch1_e200", "arch2_e512"])
def test_step_both_routes(pkg, orc, arch):
    d = orc.make_dims(**SMALL[arch])
    params = orc.synth_params(d)
    tok, lens, img, lab = orc.synth_batch(d, full_length=False)
    dr = orc.Dropout(1, 0.5, 123, 7)
    ref = orc.Oracle(np.float64).step(d, params, tok, lens, img, lab, dr)
    out = {}
    for kernel in ("1", "0"):
        ctx = _ctx(pkg, d, {"NVQA_DX0_KERNEL": kernel} if kernel == "1" else {})
        ctx.set_params(params)
        loss = ctx.step(tok, lens, img, lab, gdrop(pkg, dr))
        out[kernel] = (loss, np.array(ctx.get_grads(), copy=True), ctx.dx0_routes())
        ctx.close()
    (loss_old, g_old, r_old), (loss_new, g_new, r_new) = out["1"], out["0"]
    print(r_old, r_new)
    assert r_old == {"f32_gemm": 1, "split": 0}, r_old
    assert r_new == {"f32_gemm": 0, "split": 1}, r_new
    assert np.float32(loss_old).tobytes() == np.float32(loss_new).tobytes()
    lo = orc.layout(d)
    fed = FED[arch]
    assert all(k in lo for k in fed)
    for k, v in lo.items():
        if k.startswith("_") or k in fed:
            continue
        o, n = v
        assert np.array_equal(g_old[o:o + n].view(np.uint32), g_new[o:o + n].view(np.uint32)), f"{k} differs between the two routes"
    e_old, e_new = grad_errors(orc, d, g_old, ref["grads"]), grad_errors(orc, d, g_new, ref["grads"])
    name = f"dx0_split_step_arch{arch}"
    record(name, {"f32_route": {k: e_old[k] for k in fed}, "split_route": {k: e_new[k] for k in fed}})
    print(name, {k: (e_old[k], e_new[k]) for k in fed})
    for k in fed:
        o, n = lo[k]
        assert not np.array_equal(g_old[o:o + n], g_new[o:o + n]), f"{k}: the switch did not change the route"
        assert max(e_new[k]) <= TOL_GRAD, (k, e_new[k])
        assert e_new[k][0] <= 2.0 * e_old[k][0] and e_new[k][1] <= 2.0 * e_old[k][1], (k, e_old[k], e_new[k])
