"""The forward of the arch1 weak-paired auto-encoder's state bridge (csrc/ae_bridge.h) alone, through the checker
tests/shim/ae_bridge_check.hip (compiled here: it includes the library's header): at B = 16 / 10 rows, R = 512 and
I = 4096 / 2048, the split-K register-streaming launch and the un-split 128 x 128 LDS-tiled form, both through the finisher
k_ae1wp_bridge_fwd, against an f64 evaluation on the host -- qc, ic and the decoder's initial state within 2e-5 of their
largest element (the step tests' bound for every tensor) -- and a second run of the split form must give the same bits.
Measured (MI355X): the figures and the timing of both forms are in profiles/ae1wp_bridge_split_vs_wide.json."""
import os
import re
import shutil
import subprocess

import pytest

from util import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_bridge_forward_split_and_wide_against_f64(tmp_path):
    exe = str(tmp_path / "ae_bridge_check")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "tests", "shim", "ae_bridge_check.hip")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run(["timeout", "-k", "10", "300", exe], capture_output=True, text=True, timeout=360)
    print(r.stdout)
    lines = [l for l in r.stdout.splitlines() if l.startswith("B=")]
    errs = [(float(m.group(1)), float(m.group(2))) for m in (re.search(r"slabs, \d+ workgroups: max rel ([0-9.eE+-]+); wide un-split: max rel ([0-9.eE+-]+);", l) for l in lines)]
    record("ae_bridge_check", {"cases": len(lines), "split_max_rel": max(a for a, _ in errs) if errs else None,
                               "wide_max_rel": max(b for _, b in errs) if errs else None})
    assert len(lines) == 4, r.stdout + r.stderr
    assert all("rerun identical" in l for l in lines), r.stdout
    assert all(a < 2e-5 and b < 2e-5 for a, b in errs), r.stdout
    # the split launch covers the chip: at least as many workgroups as a 256-CU device has (the plan's aim)
    assert all(int(re.search(r"(\d+) workgroups", l).group(1)) >= 256 for l in lines), r.stdout
    assert r.returncode == 0 and all(l.endswith("OK") for l in lines), r.stdout + r.stderr
