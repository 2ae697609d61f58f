"""What the compiler makes of the per-level solver kernels of csrc/slm_front.hip: registers, scratch memory, LDS and occupancy
of k_fL21 (the streamed row solves), and the figures of k_fschur, k_fL11 and k_fpull, which share slm_tile.h with it -- an edit
to a shared helper must not move them unnoticed.

The file is compiled device-only for gfx950 with build.py's flags plus the resource remark, and only the compiler's own
resource figures are read (``-Rpass-analysis=kernel-resource-usage``); no instruction is looked at.  Figures of this build:
k_fL21 167 VGPRs, 0 AGPRs, 0 B of scratch, no spills, 33 280 B of LDS, occupancy 3 (waves per SIMD = workgroups per CU).
No GPU needed; skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

from super_amd import build as B

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="needs hipcc")

FL21_OCCUPANCY = 3                      # waves per SIMD the kernel is launched for (__launch_bounds__(256, 3))
FL21_LDS_BYTES = 53 * 1024              # three workgroups per CU in 160 KB
# kernel -> (VGPRs, waves per SIMD, scratch bytes per lane) of the commit that introduced this test
HELD = {"k_fschur": (124, 4, 0), "k_fL11": (251, 2, 0), "k_fpull": (74, 6, 0)}


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """kernel name (unmangled stem) -> the remark's figures, LDS included"""
    out = tmp_path_factory.mktemp("fl21_resources") / "slm_front.s"
    flags = [f for f in B.FLAGS if f != "-fPIC"]
    cmd = [HIPCC, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
           os.path.join(B.CSRC, "slm_front.hip"), "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    found = {}
    for m in re.finditer(r"Function Name: _Z\d+(k_\w+?)PK8FrameDev\w*(.*?LDS Size \[bytes/block\]: \d+)", run.stderr, re.S):
        found[m.group(1)] = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", m.group(2))}
    return found


def test_the_compiler_reports_the_kernels(kernels):
    for name in ("k_fL21", *HELD):
        assert name in kernels, sorted(kernels)
        print(f"MEASURE {name} {kernels[name]}")
        assert {"VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill", "LDS Size"} <= set(kernels[name]), kernels[name]


def test_the_row_solves_use_no_scratch_memory_and_keep_their_occupancy(kernels):
    k = kernels["k_fL21"]
    assert k["ScratchSize"] == 0, k
    assert k["VGPRs Spill"] == 0 and k["SGPRs Spill"] == 0, k
    assert k["AGPRs"] == 0, k
    assert k["Occupancy"] == FL21_OCCUPANCY, k
    assert k["LDS Size"] <= FL21_LDS_BYTES, k


@pytest.mark.parametrize("name", list(HELD))
def test_the_neighbouring_kernels_keep_their_figures(kernels, name):
    vgprs, occupancy, scratch = HELD[name]
    k = kernels[name]
    assert (k["VGPRs"], k["Occupancy"], k["ScratchSize"]) == (vgprs, occupancy, scratch), (name, k)
