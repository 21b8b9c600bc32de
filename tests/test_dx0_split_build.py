"""k_dx0_split (csrc/dx0_split.h) as the compiler builds it for gfx950, no GPU needed.  The kernel is designed for ONE
256-thread workgroup per CU, one wave per SIMD: a wave may use the whole register file of its SIMD lane (512 registers,
VGPRs and AGPRs together) but nothing in scratch, and the two 48 KB LDS buffers fill more than half of a CU's 160 KB so
that a second workgroup cannot join (208 workgroups then occupy 208 CUs).  The checker tests/shim/dx0_split_check.hip is
cross-compiled with the compiler's resource-usage remarks, and the launch's LDS request is read back from the header's
own function."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _usage(stderr, symbol):
    """{field: value} of the kernel-resource-usage remarks of the function whose mangled name contains `symbol`"""
    out, on = {}, False
    for line in stderr.splitlines():
        m = re.search(r"(Function Name|[A-Za-z]+(?: [A-Za-z]+)*(?: \[[a-z/A-Z]+\])?): (\S+) \[-Rpass-analysis=kernel-resource-usage\]", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            on = symbol in m.group(2)
        elif on:
            out[m.group(1)] = m.group(2)
    return out


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("dx0_build")
    src = os.path.join(ROOT, "tests", "shim", "dx0_split_check.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp / "dx0_split_check"), src],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    # the dynamic LDS the launch asks for: the header's function, evaluated by the compiler
    probe = tmp / "lds.cpp"
    probe.write_text('#include <stdio.h>\n#include "dx0_split.h"\n'
                     'int main() { printf("%d %d\\n", (int)nvqa::dx0_split_lds_bytes(), (int)NVQA_DX_THREADS); return 0; }\n')
    exe = str(tmp / "lds")
    p = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "novel-vqa_amd", "csrc"), "-o", exe, str(probe)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lds, threads = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split())
    return r.stderr, lds, threads


# the kernel's instances: 13 column tiles (N <= 208) and 16 (N <= 512)
@pytest.mark.parametrize("symbol", ["k_dx0_splitILi13EE", "k_dx0_splitILi16EE"], ids=["nt13", "nt16"])
def test_kernel_fits_one_workgroup_per_cu(remarks, symbol):
    stderr, lds, threads = remarks
    u = _usage(stderr, symbol)
    assert u, stderr[-3000:]
    print(u, lds)
    assert int(u["ScratchSize [bytes/lane]"]) == 0 and u["Dynamic Stack"] == "False"
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    # 4 waves of one workgroup on 4 SIMDs: one per SIMD has the 512 registers per lane to itself
    assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 512
    assert int(u["Occupancy [waves/SIMD]"]) == 1
    assert int(u["LDS Size [bytes/block]"]) + lds <= 163840, (u["LDS Size [bytes/block]"], lds)
    assert lds > 81920  # more than half a CU's LDS: a second workgroup cannot join, as designed
    assert threads == 256
