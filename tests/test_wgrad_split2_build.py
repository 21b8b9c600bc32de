"""k_wgrad_split2 (csrc/wgrad_split2.h) as the compiler builds it for gfx950, no GPU needed: the kernel is designed for one
512-thread workgroup per CU -- two waves per SIMD, so at most 256 registers per lane (VGPRs and AGPRs together), nothing
in scratch -- and for two 72 KB LDS buffers plus the stage tables inside the 160 KB of a CU.  The checker
tests/shim/wgrad_split2_check.hip is cross-compiled with the compiler's resource-usage remarks, and the launch's LDS
request is read back from the header's own macro."""
import os
import re
import shutil
import subprocess

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


def test_new_kernel_fits_one_workgroup_per_cu(tmp_path):
    src = os.path.join(ROOT, "tests", "shim", "wgrad_split2_check.hip")
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                        "-Rpass-analysis=kernel-resource-usage", "-o", str(tmp_path / "wgrad_split2_check"), src],
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    u = _usage(r.stderr, "k_wgrad_split2E")
    assert u, r.stderr[-3000:]
    print(u)
    assert int(u["ScratchSize [bytes/lane]"]) == 0 and u["Dynamic Stack"] == "False"
    assert int(u["VGPRs Spill"]) == 0 and int(u["SGPRs Spill"]) == 0
    # 8 waves of one workgroup on 4 SIMDs: two per SIMD share 512 registers per lane
    assert int(u["VGPRs"]) + int(u["AGPRs"]) <= 256
    assert int(u["Occupancy [waves/SIMD]"]) == 2
    # the old kernel is compiled into the same program, unchanged: still two workgroups per CU
    old = _usage(r.stderr, "k_wgrad_splitE")
    assert int(old["ScratchSize [bytes/lane]"]) == 0 and int(old["VGPRs"]) + int(old["AGPRs"]) <= 256

    # the dynamic LDS the launch asks for: the header's macro, evaluated by the compiler
    probe = tmp_path / "lds.cpp"
    probe.write_text('#include <stdio.h>\n#include "wgrad_split2.h"\n'
                     'int main() { printf("%d %d\\n", (int)NVQA_WS2_LDS_BYTES, (int)NVQA_WS2_THREADS); return 0; }\n')
    exe = str(tmp_path / "lds")
    r = subprocess.run([HIPCC, "-std=c++17", "--offload-arch=gfx950", "-x", "hip", "-I" + os.path.join(ROOT, "include"),
                        "-I" + os.path.join(ROOT, "novel-vqa_amd", "csrc"), "-o", exe, str(probe)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lds, threads = (int(x) for x in subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split())
    assert int(u["LDS Size [bytes/block]"]) + lds <= 163840, (u["LDS Size [bytes/block]"], lds)
    assert lds > 81920  # more than half a CU's LDS: a second workgroup cannot join, as designed
    assert threads == 512
