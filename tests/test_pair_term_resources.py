"""What the compiler makes of the Jacobian kernels of the LM terms that share csrc/slm_pairs.h and band_scatter_row
(csrc/slm_common.h): k_data_grad_pairs and k_data_grad (csrc/slm_data.hip, plain and weighted), k_corr_grad_pairs and
k_corr_grad (csrc/slm_corr.hip), every instantiation K = 1..8.  The shared bodies are inlined into kernels that sit at the
register limit, so an edit to them must not cost a kernel its occupancy, put it on scratch memory or change its LDS.

The two files are compiled device-only for gfx950 with build.py's flags plus the resource remark, and only the compiler's own
resource figures are read (``-Rpass-analysis=kernel-resource-usage``); no instruction is looked at:

    hipcc <build.py FLAGS without -fPIC> --cuda-device-only -Rpass-analysis=kernel-resource-usage -S csrc/slm_data.hip -o x.s

HELD is what that command gave for the commit before the kernels shared their bodies (the separate copies); a different compiler
build moves the figures, re-measure that commit with it before trusting the table.  Held per instantiation: scratch bytes not
above, waves per SIMD not below, LDS bytes equal, no SGPR spill, VGPR spills (to AGPRs: the scratch is 0) not above -- none
except the two of k_data_grad_pairs<8, DataWArgs>.  VGPR and AGPR counts may move; they are printed as MEASURE lines.
No GPU needed; skipped without hipcc."""
import os
import re
import shutil
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from super_amd import build as B

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="needs hipcc")

KS = range(1, 9)
# (kernel, what follows the K in its mangled template arguments) -> the row's name
ROWS = {("k_data_grad_pairs", "JE"): "k_data_grad_pairs<K>", ("k_data_grad_pairs", "J9DataWArgsE"): "k_data_grad_pairs<K,DataWArgs>",
        ("k_corr_grad_pairs", "Li1E"): "k_corr_grad_pairs<K,1>", ("k_corr_grad_pairs", "Li3E"): "k_corr_grad_pairs<K,3>",
        ("k_corr_grad", ""): "k_corr_grad<K>", ("k_data_grad", "J9DataWArgsE"): "k_data_grad<K,DataWArgs>",
        ("k_data_grad", "JE"): "k_data_grad<K>"}
# row -> (scratch bytes per lane, waves per SIMD, LDS bytes) for K = 1..8
HELD = {
    "k_data_grad_pairs<K>": ((0, 3, 11392), (0, 2, 12160), (0, 2, 27648), (0, 1, 28928), (0, 1, 49024), (0, 1, 50816), (0, 1, 75520), (0, 1, 77824)),
    "k_data_grad_pairs<K,DataWArgs>": ((0, 2, 11392), (0, 2, 12160), (0, 2, 27648), (0, 1, 28928), (0, 1, 49024), (0, 1, 50816), (0, 1, 75520), (0, 1, 77824)),
    "k_corr_grad_pairs<K,1>": ((0, 4, 11392), (0, 4, 12160), (0, 2, 27648), (0, 2, 28928), (0, 1, 49024), (0, 1, 50816), (0, 1, 75520), (0, 1, 77824)),
    "k_corr_grad_pairs<K,3>": ((0, 2, 28800), (0, 2, 29568), (0, 1, 61440), (0, 1, 62720), (0, 1, 99200), (0, 1, 100992), (0, 1, 142080), (0, 1, 144384)),
    "k_corr_grad<K>": ((0, 8, 3840), (0, 5, 8192), (0, 4, 11520), (0, 3, 15872), (0, 2, 19200), (0, 2, 23552), (0, 2, 26880), (0, 2, 31232)),
    "k_data_grad<K,DataWArgs>": ((0, 3, 3840), (0, 2, 8192), (0, 2, 11520), (0, 1, 15872), (0, 1, 19200), (0, 1, 23552), (0, 1, 26880), (0, 1, 31232)),
    "k_data_grad<K>": ((128, 3, 0), (184, 3, 0), (248, 2, 0), (304, 2, 0), (368, 2, 0), (424, 2, 0), (488, 1, 0), (544, 1, 0)),
}
VGPR_SPILLS_HELD = {("k_data_grad_pairs<K,DataWArgs>", 8): 2}   # every other instantiation: 0


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """(row, K) -> the remark's figures, LDS included"""
    tmp = tmp_path_factory.mktemp("pair_term_resources")
    flags = [f for f in B.FLAGS if f != "-fPIC"]

    def remarks(stem):
        cmd = [HIPCC, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
               os.path.join(B.CSRC, stem + ".hip"), "-o", str(tmp / (stem + ".s"))]
        run = subprocess.run(cmd, capture_output=True, text=True)
        assert run.returncode == 0, run.stderr[-3000:]
        return run.stderr

    with ThreadPoolExecutor(max_workers=2) as ex:
        text = "".join(ex.map(remarks, ("slm_data", "slm_corr")))
    found = {}
    for m in re.finditer(r"Function Name: _Z\d+(k_(?:data|corr)_grad(?:_pairs)?)ILi(\d)E(\w*?)EvPK8FrameDev\S*(.*?LDS Size \[bytes/block\]: \d+)",
                         text, re.S):
        figures = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", m.group(4))}
        found[(ROWS[(m.group(1), m.group(3))], int(m.group(2)))] = figures
    return found


def test_the_compiler_reports_every_instantiation(kernels):
    assert set(kernels) == {(row, k) for row in HELD for k in KS}, sorted(kernels)
    for row in HELD:
        print("MEASURE", row, "VGPRs/AGPRs/scratch/waves/LDS", " ".join(
            "{VGPRs}/{AGPRs}/{ScratchSize}/{Occupancy}/{LDS Size}".format(**kernels[(row, k)]) for k in KS))


@pytest.mark.parametrize("row", list(HELD))
def test_the_kernels_keep_scratch_spills_lds_and_occupancy(kernels, row):
    for k in KS:
        scratch, occupancy, lds = HELD[row][k - 1]
        f = kernels[(row, k)]
        print(f"MEASURE {row} K={k} {f}")
        assert f["ScratchSize"] <= scratch, (row, k, f)
        assert f["SGPRs Spill"] == 0 and f["VGPRs Spill"] <= VGPR_SPILLS_HELD.get((row, k), 0), (row, k, f)
        assert f["LDS Size"] == lds, (row, k, f)
        assert f["Occupancy"] >= occupancy, (row, k, f)
