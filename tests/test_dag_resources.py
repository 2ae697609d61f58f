"""What the compiler makes of csrc/slm_dag.hip: the scratch memory of k_fdag's task kinds and the kernel's occupancy.

The file is compiled device-only for gfx950 with build.py's flags plus the resource remark, to assembly, and only the
compiler's own resource figures are read: the ``; ScratchSize`` line of every function's info block in the assembly and the
``ScratchSize [bytes/lane]`` / ``Occupancy [waves/SIMD]`` remarks of the kernel.  No instruction is looked at.

A task kind that is compiled into the ticket loop has no function of its own: its figure is the kernel's.  The bounds are
the figures of the build in which every kind was a call (docs/LAB_NOTEBOOK.md "k_fdag: the task kinds in the
ticket loop"): POTRF -- the pivot chain -- must use none at all, no kind more than it did then, and k_fdag must keep two
workgroups per CU (occupancy 2).  Figures of this build: k_fdag 232 VGPRs, 0 AGPRs, 0 B of scratch, occupancy 2, no task
function left out of line.  No GPU needed; skipped without hipcc."""
import os
import re
import shutil
import subprocess

import pytest

from super_amd import build as B

# bytes of scratch memory per lane, by task kind: the build with one call per task (the parent of this test)
BOUND = {"POTRF": 0, "COL": 12, "SCHUR": 348, "BACKB": 224, "BACK": 240}
# the function a kind lives in when it is not inlined (mangled-name fragments; POTRF / COL: dag_task_factor<true / false>)
FUNCTION = {"POTRF": "dag_task_factorILb1E", "COL": "dag_task_factorILb0E", "SCHUR": "dag_task_schur", "BACKB": "dag_task_backb",
            "BACK": "dag_task_back"}
KERNEL = "_Z6k_fdag"

HIPCC = B.HIPCC if os.path.exists(B.HIPCC) else shutil.which("hipcc")
pytestmark = pytest.mark.skipif(not HIPCC, reason="needs hipcc")


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    """(function name -> ScratchSize from the assembly's info blocks, the kernel's remark figures)"""
    out = tmp_path_factory.mktemp("dag_resources") / "slm_dag.s"
    flags = [f for f in B.FLAGS if f != "-fPIC"]
    cmd = [HIPCC, *flags, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-S",
           os.path.join(B.CSRC, "slm_dag.hip"), "-o", str(out)]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr[-3000:]
    scratch = {}
    name = None
    for line in out.read_text().splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
        m = re.match(r"^; ScratchSize: (\d+)", line)
        if m and name:
            scratch[name] = int(m.group(1))
            name = None
    remark = re.search(r"Function Name: %s\w*(.*?)LDS Size" % KERNEL, run.stderr, re.S)
    assert remark, run.stderr[-3000:]
    kernel = {k: int(v) for k, v in re.findall(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", remark.group(1))}
    return scratch, kernel


def _figure(scratch, kind):
    """the kind's own function when it has one, else the kernel it is compiled into"""
    own = [n for n in scratch if FUNCTION[kind] in n and (kind != "BACK" or "backb" not in n)]
    assert len(own) <= 1, own
    kern = [n for n in scratch if n.startswith(KERNEL)]
    assert len(kern) == 1, sorted(scratch)
    return scratch[own[0]] if own else scratch[kern[0]]


def test_the_compiler_reports_the_kernel(resources):
    scratch, kernel = resources
    print(f"MEASURE k_fdag {kernel}; ScratchSize by function: { {n: v for n, v in scratch.items() if 'dag' in n} }")
    assert {"VGPRs", "AGPRs", "ScratchSize", "Occupancy", "SGPRs Spill", "VGPRs Spill"} <= set(kernel), kernel
    assert scratch[[n for n in scratch if n.startswith(KERNEL)][0]] == kernel["ScratchSize"]      # the two sources agree


def test_the_pivot_chain_uses_no_scratch_memory(resources):
    scratch, _ = resources
    assert _figure(scratch, "POTRF") == 0


@pytest.mark.parametrize("kind", list(BOUND))
def test_no_task_kind_uses_more_scratch_memory_than_as_a_call(resources, kind):
    scratch, _ = resources
    assert _figure(scratch, kind) <= BOUND[kind], (kind, _figure(scratch, kind))


def test_two_workgroups_per_cu(resources):
    _, kernel = resources
    assert kernel["Occupancy"] == 2, kernel
    assert kernel["VGPRs"] + kernel["AGPRs"] <= 256, kernel
