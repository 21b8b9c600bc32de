"""k_wgrad_split2 (csrc/wgrad_split2.h: the six-term weight gradients on 256 x 128 tiles with a pipelined K loop) against
k_wgrad_split (csrc/wgrad_split.h), which it replaces as the default: the two must give the SAME BITS.

* The kernels alone, through the checker tests/shim/wgrad_split2_check.hip (compiled here: it includes the library's
  headers): both kernels on the same operands into NaN-prefilled slab buffers, all ks slabs compared as bits, no element
  left unwritten, a second run of the new kernel repeating its bits.  Cases: one tile / two stages / direct write; partial
  tiles both ways with slices of 3 and of 2 stages; slices without a stage; a ragged batch with skipped padding stages; a
  26-row K tail with nrows given but no skipping; 256 steps of 32 rows; padded leading dimensions; and the step's shapes
  (2048 x 512 and 2048 x 200, K 13312 and 13000, 8 and 16 slices, full and ragged).  No tolerance is involved: the old
  kernel stays held against the f64 product by tests/test_gpu_wgrad_split.py.
* The whole step both ways, the default and NVQA_WGRAD_KERNEL=1, at the headline dimensions (all lengths 26, ragged) and at
  B = 500: loss and the whole gradient vector equal as bits, and the context's route counters (nvqa_wgrad_routes) show
  that the switch changed the kernel."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from util import gdims, gdrop

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FULL1 = dict(arch=1, B=512, T=26, V=14773, E=200, R=512, L=2, I=4096, C=1024, A=1000)
N_CASES = 7 + 16


def test_both_kernels_give_the_same_slabs(tmp_path):
    exe = str(tmp_path / "wgrad_split2_check")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "shim", "wgrad_split2_check.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "120", exe], capture_output=True, text=True, timeout=150)
    print(r.stdout)
    lines = [l for l in r.stdout.splitlines() if "slabs" in l]
    assert len(lines) == N_CASES, r.stdout + r.stderr
    assert all("slabs identical" in l and "unwritten 0," in l and "rerun identical" in l for l in lines), r.stdout
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


@pytest.mark.parametrize("B,full_length", [(512, True), (512, False), (500, False)], ids=["all26", "ragged", "b500"])
def test_step_is_bit_identical_on_both_kernels(pkg, orc, B, full_length):
    d = orc.make_dims(**dict(FULL1, B=B))
    params = orc.synth_params(d)
    tok, lens, img, lab = orc.synth_batch(d, full_length=full_length)
    dr = orc.Dropout(1, 0.5, 123, 7)
    out = {}
    for kernel in ("1", "2"):
        ctx = _ctx(pkg, d, {"NVQA_WGRAD_KERNEL": kernel} if kernel == "1" else {})
        ctx.set_params(params)
        loss = ctx.step(tok, lens, img, lab, gdrop(pkg, dr))
        out[kernel] = (loss, np.array(ctx.get_grads(), copy=True), ctx.wgrad_routes())
        ctx.close()
    (loss1, g1, r1), (loss2, g2, r2) = out["1"], out["2"]
    print(r1, r2)
    # the switch changes the route: the four LSTM weight gradients (two per layer) go through one kernel or the other
    assert r1["split"] == 2 * d.L and r1["split2"] == 0, r1
    assert r2["split2"] == 2 * d.L and r2["split"] == 0, r2
    assert np.float32(loss1).tobytes() == np.float32(loss2).tobytes()
    assert g1.dtype == np.float32 and g1.shape == g2.shape
    assert np.array_equal(g1.view(np.uint32), g2.view(np.uint32)), "the gradient vectors differ between the two kernels"
