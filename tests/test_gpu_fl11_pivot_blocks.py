"""k_fL11, the kernel that factors a front's whole pivot block in one workgroup (the compact form of the per-level launches), at
every pivot-column count it serves -- one column whose last 16-pivot block is partial, two columns of which the second holds
6 true pivots, two, three and four full columns -- and on a graph whose separators are irregular: the tiles it hands from
one step to the next through LDS and registers must give the solve the global round trips gave.  Through the C ABI, one
child process per case (SLM_ND_LEAF and SLM_COMPACT_MIN are read once per process).  Needs an MI355X (-m gpu).

Per case: slm_solve on solver_path 3 with two slots at u = 0 and u = 0.37 against the dense float64 solve of the oracle's
normal equations and of the library's own matrix (the comparisons and bounds of tests/test_gpu_solver_graphs.py); the same
solve twice and on the other slot, byte for byte; chol_fail raised at u = 0 for a frame with a zero pivot and not otherwise.
That the case reaches the kernel is asserted on the host analysis: a level with the wanted pivot-column count exists, is
compact (at most 4 columns, fronts x frames >= SLM_COMPACT_MIN = 1), and -- for the grids -- a leaf of exactly SLM_ND_LEAF
nodes sits in a compact level.  Each test prints ``MEASURE`` lines (run with -s).

Largest figures on an MI355X over the six cases and both dampings: forward error 1.3e-13 (coincident, u = 0; bound 1e-9),
backward error 0.001 P eps (bound 64), against the dense solve of the library's own matrix 4.8e-13 on the grids and 7.4e-11 on
the coincident nodes at u = 0 (cond 7.8e7: the NumPy reference itself is good to 1.9e-9 there), repeated run and other slot
0 bytes apart, zero-pivot frame: status 1 at u = 0 and 0 at u = 0.37.  23 s for the file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_graph_cases as sgc
from oracle import lm_oracle as orc
from super_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
US = (0.0, sgc.U_SOLVE)
COMPACT_NPT = 4                      # launch_front_levels: a level is compact when max_npt <= 4 and fronts x frames >= SLM_COMPACT_MIN
# name -> (scene, SLM_ND_LEAF or None, pivot tile columns the case is about).  The 12 x 13 and 9 x 18 grids have, at these leaf
# sizes, a leaf of exactly SLM_ND_LEAF nodes and no level above four columns (checked below, on the CPU).
CASES = {
    "leaf9": (("grid", 156), 9, 1),      # 63 pivots: one column, last 16-block partial
    "leaf10": (("grid", 156), 10, 2),    # 70: two columns, the second with 6 true pivots
    "leaf18": (("grid", 162), 18, 2),    # 126: two columns
    "leaf27": (("grid", 156), 27, 3),    # 189: three columns
    "leaf36": (("grid", 162), 36, 4),    # 252: four columns, the compact limit
    "coincident": (("case", "coincident"), None, 4),   # 32 coincident nodes: separators of 23 and 32 nodes, a 4-column level of separators
}


@functools.lru_cache(maxsize=None)
def _scene(kind, arg):
    if kind == "case":
        return sgc.case(arg)
    return synth.make_scene(N=2500, J=arg, seed=500 + arg, **sgc.BASE)


def _failing(sc):
    """the scene without the surfels that list its middle node: under FAIL_OPT_ROT at u = 0 that node's qx pivot is exactly zero"""
    import copy
    out = copy.copy(sc)
    keep = (sc.sf_knn_idx != sc.J // 2).all(axis=1)
    for k in ("sf_points", "sf_norms", "sf_knn_idx", "sf_knn_w"):
        setattr(out, k, np.ascontiguousarray(getattr(sc, k)[keep]))
    return out


@functools.lru_cache(maxsize=None)
def _reference(kind, arg):
    """u -> (A, b, delta, norm(A, 2)) of the oracle's normal equations at the perturbed beta: computed once, read-only"""
    sc = _scene(kind, arg)
    JtJ, jtl, _ = orc.normal_equations(orc.Frame.from_scene(sc), sgc.perturbed_beta(sc.J), orc.default_opt())
    out = {}
    for u in US:
        A = JtJ + u * np.eye(len(jtl))
        d = orc.solve_damped(JtJ, jtl, u)
        for a in (A, d):
            a.setflags(write=False)
        out[u] = (A, jtl, d, float(np.linalg.norm(A, 2)))
    return out


CHILD = r"""
import copy, sys, numpy as np, torch
sys.path[:0] = [{root!r}, {pkg!r}, {tests!r}]
import solver_graph_cases as sgc
import test_gpu_fl11_pivot_blocks as me
from super_amd import _lib
from super_amd.engine import DeviceFrame, Engine
kind, arg, leaf, out = {kind!r}, {arg!r}, {leaf!r}, {out!r}
dev = torch.device('cuda', 0)
sc = me._scene(kind, arg)
P = 7 * sc.J
sched = sgc.host_level_schedule(sc)                       # (this process's SLM_ND_LEAF applies)
hp = sgc.host_plan(sc, leaf or sgc.LEAF)
def solve(e, slot, u):
    delta = torch.zeros(P, dtype=torch.float64, device='cuda')
    status = torch.full((1,), -7, dtype=torch.int32, device='cuda')
    _lib.check(e.lib.slm_solve(e.h, slot, u, delta.data_ptr(), status.data_ptr(), e.stream), 'slm_solve')
    torch.cuda.synchronize()
    return delta.cpu().numpy(), int(status.item())
res = dict(sched=np.array(sched), front_nv=hp['front_nv'], front_depth=hp['front_depth'], front_is_leaf=hp['front_is_leaf'])
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
for k, u in enumerate(me.US):
    runs = [solve(e, 0, u), solve(e, 0, u), solve(e, 1, u)]
    res['delta%d' % k] = np.stack([r[0] for r in runs])
    res['status%d' % k] = np.array([r[1] for r in runs])
res['form'] = e.lib.slm_debug_last_solver_form(e.h)
info = e.plan_info(0)
res['plan'] = np.array([int(info['fronts']), int(info['levels'])])
e.close()
# a frame with one exactly-zero pivot (solver_graph_cases: failure placement), at the identity
e = Engine(dev, max_frames=2, solver_path=3, use_arap=False, use_rot=True, u0=0.0)
e.bind(0, DeviceFrame.from_scene(me._failing(sc), dev))
res['fail_status'] = np.array([solve(e, 0, u)[1] for u in me.US])
e.close()
np.savez(out, **res)
"""


@pytest.mark.parametrize("name", list(CASES))
def test_pivot_blocks_of_every_column_count_solve_like_the_dense_solve(name, tmp_path):
    (kind, arg), leaf, want_npt = CASES[name]
    sc = _scene(kind, arg)
    P = 7 * sc.J
    out = str(tmp_path / "fl11.npz")
    code = CHILD.format(root=ROOT, pkg=os.path.join(ROOT, "python-super_amd"), tests=os.path.join(ROOT, "tests"),
                        kind=kind, arg=arg, leaf=leaf, out=out)
    env = dict(os.environ, SLM_COMPACT_MIN="1")
    env.pop("SLM_ND_LEAF", None)
    env.pop("SLM_COMPACT_NPT", None)
    if leaf:
        env["SLM_ND_LEAF"] = str(leaf)
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(out)

    # ---- the case reaches k_fL11 with the pivot-column count it is about
    sched = [tuple(int(x) for x in row) for row in got["sched"]]
    print(f"MEASURE {name} J={sc.J} levels (n_fronts, max_npt, max_nt) = {sched} plan={tuple(got['plan'])} form={int(got['form'])}")
    assert int(got["form"]) == 0                                                     # per-level launches
    assert tuple(got["plan"]) == (sum(n for n, _, _ in sched), len(sched))           # the bind built the plan of this schedule
    hit = [(n, npt, nt) for n, npt, nt in sched if npt == want_npt]
    assert hit, (want_npt, sched)
    assert all(npt <= COMPACT_NPT and n * 1 >= 1 for n, npt, nt in hit)              # compact: one slot per slm_solve, SLM_COMPACT_MIN = 1
    if leaf:
        # a leaf of exactly `leaf` nodes (7 leaf pivots: the column count and the true pivots of the last column of the table
        # above), in a compact level
        depth, nv, is_leaf = got["front_depth"], got["front_nv"], got["front_is_leaf"]
        full = np.nonzero(is_leaf & (nv == leaf))[0]
        assert len(full) > 0, sorted(set(nv[is_leaf].tolist()))
        assert (7 * leaf + 63) // 64 == want_npt
        level_npt = {int(d): int(((7 * nv[depth == d] + 63) // 64).max()) for d in set(depth.tolist())}
        assert all(level_npt[int(depth[i])] <= COMPACT_NPT for i in full), level_npt

    # ---- the solves
    ref = _reference(kind, arg)
    eps = np.finfo(np.float64).eps
    for k, u in enumerate(US):
        deltas, status = got[f"delta{k}"], got[f"status{k}"]
        A, b, want, norm2 = ref[u]
        d = deltas[0]
        own = np.linalg.solve(got["jtj"] + u * np.eye(P), got["jtl"])
        fwd, bwd = float(np.abs(d - want).max()), sgc.backward_error(A, b, d, norm2)
        print(f"MEASURE {name} u={u} status={status.tolist()} forward={fwd:.3e} backward={bwd:.3e} = {bwd / (P * eps):.3f} P eps "
              f"own_matrix={np.abs(d - own).max():.3e} run2={np.abs(deltas[1] - d).max():.3e} slot1={np.abs(deltas[2] - d).max():.3e}")
        assert (status == 0).all(), (u, status)                                      # chol_fail not raised on a positive definite matrix
        assert np.isfinite(d).all()
        np.testing.assert_allclose(d, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()))
        assert bwd <= sgc.backward_bound(P), (u, bwd, sgc.backward_bound(P))
        # (1e-11 as in test_gpu_solver_graphs.py, where the NumPy LU solve of the own matrix is good to that at u = 0.37; at
        #  u = 0 its own forward error, cond(A) eps |x|, can be larger -- 1.9e-9 for the coincident nodes, cond 7.8e7)
        A_own = got["jtj"] + u * np.eye(P)
        np.testing.assert_allclose(d, own, rtol=0, atol=max(1e-11, np.linalg.cond(A_own) * eps * np.abs(own).max()))
        assert deltas[1].tobytes() == d.tobytes()                                    # the same solve again
        assert deltas[2].tobytes() == d.tobytes()                                    # the other slot, identical input
    print(f"MEASURE {name} zero-pivot frame: status at u = {US} -> {got['fail_status'].tolist()}")
    assert got["fail_status"][0] != 0 and got["fail_status"][1] == 0
