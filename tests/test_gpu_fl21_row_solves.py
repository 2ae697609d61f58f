"""k_fL21, the kernel that solves a boundary row tile of a front against the front's whole pivot block (the compact form of the
per-level launches): its column loop is one software-pipelined stream over the row's products -- column 0: Linv_0; column 1:
L(1,0), Linv_1; ... -- with the B tiles passing through LDS in half tiles.  The shapes at which that stream can go wrong: one
to four pivot tile columns (a stream of 1, 3, 6 and 10 products), a last column with 6 true pivots and one whose last
16-block is partial (trimmed products, the second half of Linv skipped), a last boundary tile row with fewer than 16 true rows
(waves 1 - 3 only move the B stream) and with 17 - 48 (some waves off), fronts with exactly one boundary row tile and with
several, levels small enough for the plain grid of workgroups (fronts x frames < 8) and levels on the XCD-ordered map.
Through the C ABI, one child process per case (SLM_ND_LEAF and SLM_COMPACT_MIN are read once per process), with the
machinery of tests/test_gpu_fl11_pivot_blocks.py.  Needs an MI355X (-m gpu).

Per case: slm_solve on solver_path 3 with two slots at u = 0 and u = 0.37 against the dense float64 solve of the oracle's
normal equations and of the library's own matrix (the comparisons and bounds of tests/test_gpu_solver_graphs.py, imported);
the same solve twice and on the other slot, byte for byte; status 0.  That the case reaches the kernel with the shape it is
about is asserted on the host analysis (the fronts of the plan at this process's SLM_ND_LEAF, level by level).  Each test
prints ``MEASURE`` lines (run with -s).

Largest figures on an MI355X over the five cases and both dampings: forward error 5.0e-14 (bound 1e-9), backward error
0.001 P eps (bound 64), against the dense solve of the library's own matrix 1.7e-12 at u = 0 and 1.5e-14 at u = 0.37 (bound
1e-11), repeated run and other slot 0 bytes apart.  18 s for the file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_graph_cases as sgc
import test_gpu_fl11_pivot_blocks as fl11
import test_gpu_solver_graphs as tsg

pytestmark = pytest.mark.gpu

ROOT = fl11.ROOT
US = fl11.US
NB = 64                              # SLM_NB: the tile edge
XCD_MIN = 8                          # make_map (csrc/slm_front.hip): the XCD-ordered map from fronts x frames >= 8 on
# name -> what the case must show besides its pivot-column count (fl11.CASES: scene, SLM_ND_LEAF, pivot tile columns)
CASES = {
    "leaf9": ("partial_last_block", "one_boundary_tile", "several_boundary_tiles", "last_rows_below_16", "last_rows_17_to_48",
              "plain_grid", "xcd_map"),
    "leaf10": ("six_pivots_in_last_column", "xcd_map"),
    "leaf18": ("several_boundary_tiles", "last_rows_below_16"),
    "leaf27": ("several_boundary_tiles", "last_rows_17_to_48", "plain_grid"),
    "leaf36": ("several_boundary_tiles", "plain_grid"),
}


def features(fronts, want_npt):
    """What k_fL21 meets on a plan: fronts = rows (depth, pivot nodes, boundary nodes, parent) of the host analysis.  Only fronts
    with a boundary in compact levels (at most 4 pivot tile columns; SLM_COMPACT_MIN = 1) count: those are the kernel's rows."""
    out = set()
    for d in set(fronts[:, 0].tolist()):
        lv = fronts[fronts[:, 0] == d]
        n1, n2 = 7 * lv[:, 1], 7 * lv[:, 2]
        npt = (n1 + NB - 1) // NB
        if npt.max() > fl11.COMPACT_NPT or not (n2 > 0).any():
            continue
        out.add("xcd_map" if len(lv) >= XCD_MIN else "plain_grid")        # one slot per slm_solve: frames = 1
        for a, b, p in zip(n1.tolist(), n2.tolist(), npt.tolist()):
            if b == 0:
                continue
            if p == want_npt:
                out.add("want_npt")
                last = a - NB * (p - 1)                                   # true pivots of the last tile column
                if last == 6:
                    out.add("six_pivots_in_last_column")
                if last % 16 != 0:
                    out.add("partial_last_block")
            tiles, rows = (b + NB - 1) // NB, b - NB * ((b + NB - 1) // NB - 1)
            out.add("one_boundary_tile" if tiles == 1 else "several_boundary_tiles")
            if rows < 16:
                out.add("last_rows_below_16")
            if 17 <= rows <= 48:
                out.add("last_rows_17_to_48")
    return out


CHILD = r"""
import ctypes as C, sys, numpy as np, torch
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import solver_graph_cases as sgc
import test_gpu_fl11_pivot_blocks as fl11
from super_amd import _lib
from super_amd.engine import DeviceFrame, Engine
kind, arg, out = {kind!r}, {arg!r}, {out!r}
dev = torch.device('cuda', 0)
sc = fl11._scene(kind, arg)
P = 7 * sc.J
# the fronts of the plan (this process's SLM_ND_LEAF applies): depth, pivot nodes, boundary nodes, parent
lib = sgc._nd_lib()
pts, knn, pairs = np.ascontiguousarray(sc.ed_points, np.float32), np.ascontiguousarray(sc.ed_knn_idx, np.int32), sgc.coupled_pairs(sc)
stats, fronts = np.zeros(8), np.zeros((sc.J + 1, 4), np.int32)
p = lambda a: a.ctypes.data_as(C.c_void_p)
n = lib.nd_stats(sc.J, knn.shape[1], p(pts), p(knn), p(pairs), len(pairs), p(stats), p(fronts), len(fronts), None)
assert 1 <= n <= len(fronts), n
res = dict(fronts=fronts[:n].copy(), sched=np.array(sgc.host_level_schedule(sc)))
def solve(e, slot, u):
    delta = torch.zeros(P, dtype=torch.float64, device='cuda')
    status = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    _lib.check(e.lib.slm_solve(e.h, slot, u, delta.data_ptr(), status.data_ptr(), e.stream), 'slm_solve')
    torch.cuda.synchronize()
    return delta.cpu().numpy(), int(status.item())
e = Engine(dev, max_frames=2, solver_path=3)
fr = DeviceFrame.from_scene(sc, dev)
e.bind(0, fr)
e.bind(1, fr)
bt = torch.from_numpy(np.ascontiguousarray(sgc.perturbed_beta(sc.J))).cuda()
for slot in (0, 1):
    _lib.check(e.lib.slm_set_beta(e.h, slot, bt.data_ptr(), e.stream), 'slm_set_beta')
torch.cuda.synchronize()
jtj = torch.zeros((P, P), dtype=torch.float64, device='cuda')
jtl = torch.zeros(P, dtype=torch.float64, device='cuda')
_lib.check(e.lib.slm_assemble(e.h, 0, jtj.data_ptr(), jtl.data_ptr(), e.stream), 'slm_assemble')
torch.cuda.synchronize()
res['jtj'], res['jtl'] = jtj.cpu().numpy(), jtl.cpu().numpy()
for k, u in enumerate(fl11.US):
    runs = [solve(e, 0, u), solve(e, 0, u), solve(e, 1, u)]
    res['delta%d' % k] = np.stack([r[0] for r in runs])
    res['status%d' % k] = np.array([r[1] for r in runs])
res['form'] = e.lib.slm_debug_last_solver_form(e.h)
info = e.plan_info(0)
res['plan'] = np.array([int(info['fronts']), int(info['levels'])])
e.close()
np.savez(out, **res)
"""


@pytest.mark.parametrize("name", list(CASES))
def test_row_solves_of_every_stream_length_solve_like_the_dense_solve(name, tmp_path):
    (kind, arg), leaf, want_npt = fl11.CASES[name]
    sc = fl11._scene(kind, arg)
    P = 7 * sc.J
    out = str(tmp_path / "fl21.npz")
    code = CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "python-super_amd"), tests=os.path.join(ROOT, "tests"),
                        kind=kind, arg=arg, out=out)
    env = dict(os.environ, SLM_COMPACT_MIN="1", SLM_ND_LEAF=str(leaf))
    env.pop("SLM_COMPACT_NPT", None)
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(out)

    # ---- the case reaches k_fL21 with the shapes it is about
    sched = [tuple(int(x) for x in row) for row in got["sched"]]
    seen = features(got["fronts"], want_npt)
    print(f"MEASURE {name} J={sc.J} levels (n_fronts, max_npt, max_nt) = {sched} plan={tuple(got['plan'])} form={int(got['form'])} "
          f"reaches {sorted(seen)}")
    assert int(got["form"]) == 0                                                     # per-level launches
    assert tuple(got["plan"]) == (len(got["fronts"]), len(sched))                    # the bind built the plan of this analysis
    assert any(npt == want_npt and npt <= fl11.COMPACT_NPT for _, npt, _ in sched), (want_npt, sched)
    assert {"want_npt", *CASES[name]} <= seen, sorted({"want_npt", *CASES[name]} - seen)

    # ---- the solves
    ref = fl11._reference(kind, arg)
    for k, u in enumerate(US):
        deltas, status = got[f"delta{k}"], got[f"status{k}"]
        d = deltas[0]
        own = np.linalg.solve(got["jtj"] + u * np.eye(P), got["jtl"])
        print(f"MEASURE {name} u={u} status={status.tolist()} own_matrix={np.abs(d - own).max():.3e} "
              f"run2={np.abs(deltas[1] - d).max():.3e} slot1={np.abs(deltas[2] - d).max():.3e}")
        assert (status == 0).all(), (u, status)
        tsg._check_against_oracle(f"{name} u={u}", d, ref[u])                        # forward 1e-9 max(1, |ref|), backward 64 P eps
        np.testing.assert_allclose(d, own, rtol=0, atol=1e-11)                       # as in test_gpu_solver_graphs.py
        assert deltas[1].tobytes() == d.tobytes()                                    # the same solve again
        assert deltas[2].tobytes() == d.tobytes()                                    # the other slot, identical input
