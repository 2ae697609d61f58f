"""k_fdag, the task-graph launch of csrc/slm_dag.hip, on graphs small enough that ONE solve runs every task kind -- POTRF on
fronts of 1, 2 and >= 3 pivot tile columns (the first column, the streamed row solve and the look-ahead entry of the later
ones), COL, SCHUR, BACKB, and BACK in its plain and its fused form -- in the two forms the solver launches it in:
  (a) solver_path 2, one frame: the whole tree as tasks, one ticket stream;
  (b) solver_path 4, eight slots: the hybrid form -- the top of the tree and the whole back substitution as tasks, on an
      8-XCD device with one ticket stream per XCD and operand tiles through that XCD's L2.
Every kind is compiled into the ticket loop; what a task keeps in registers across its phases must give the solve
the dense solve gives.  One child process per graph (SLM_ND_LEAF is read once per process), each under its own time limit.
Needs an MI355X (-m gpu).

Per graph and form: delta against the dense float64 NumPy solve of the library's own slm_assemble matrix at u = 0.37 (1e-11, the
bound of tests/test_gpu_solver_graphs.py); delta and the solver's status byte for byte between two runs (and between the eight
slots of form b, which bind the same frame); status 0 and no record with SLM_ITER_SOLVER_TIMEOUT.  That the graph has every
task kind is asserted on the host analysis of the same plan.  Each test prints ``MEASURE`` lines (run with -s).

Largest figures on an MI355X over the three graphs: form (a) 2.1e-14, form (b) 2.1e-14 against the dense solve (bound 1e-11);
second run and other slots 0 bytes apart; form (b) ran with XCD-affine streams (mode 1).  11 s for the file."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import solver_graph_cases as sgc
from super_amd import synth

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = sgc.U_SOLVE
SLOTS = 8
BACK_FUSE_NPT = 2                    # slm_nd_host.hip: fronts with a boundary and at most this many pivot columns get the fused BACK
# name -> (scene, SLM_ND_LEAF or None).  Fronts as (pivot tile columns, boundary tile rows), root first:
#   grid_12x13 at 27-node leaves: (2,0) | (2,2) (2,2) | (3,2) (1,3) (1,3) (3,2) | (1,2) (2,3) (3,3) (2,2)
#   grid_9x18 at 27-node leaves:  (3,0) | (1,3) (2,3) | (3,2) (3,2) (2,3) (1,3) | (1,3) (2,2) (1,3) (2,2)
#   coincident (18-node leaves):  (3,0) | (1,3) (2,3) | (4,2) (1,2) (2,4) (1,2) | (2,3) (1,2) (1,3) (1,1)
# four levels each: the hybrid form runs the three upper ones as tasks (at most four fronts per level).
CASES = {
    "grid_12x13": (("grid", 156), 27),
    "grid_9x18": (("grid", 162), 27),
    "coincident": (("case", "coincident"), 18),
}


@functools.lru_cache(maxsize=None)
def _scene(kind, arg):
    if kind == "case":
        return sgc.case(arg)
    return synth.make_scene(N=2500, J=arg, seed=500 + arg, **sgc.BASE)


def _fronts(sc):
    """(depth, pivot nodes, boundary nodes, parent) per front of the plan this process's SLM_ND_LEAF gives"""
    import ctypes as C
    lib = sgc._nd_lib()
    pts = np.ascontiguousarray(sc.ed_points, np.float32)
    knn = np.ascontiguousarray(sc.ed_knn_idx, np.int32)
    pairs = sgc.coupled_pairs(sc)
    stats, fronts = np.zeros(8), np.zeros((sc.J + 1, 4), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib.nd_stats(sc.J, knn.shape[1], p(pts), p(knn), p(pairs), len(pairs), p(stats), p(fronts), len(fronts), None)
    assert 1 <= n <= len(fronts), n
    return fronts[:n].copy()


def _child(name, out):
    import torch
    from super_amd import _lib
    from super_amd.engine import DeviceFrame, Engine
    (kind, arg), _ = CASES[name]
    dev = torch.device("cuda", 0)
    sc = _scene(kind, arg)
    P = 7 * sc.J
    beta0 = np.ascontiguousarray(sgc.perturbed_beta(sc.J))
    bt = torch.from_numpy(beta0).cuda()
    res = dict(fronts=_fronts(sc))

    # ---- (a) the whole tree as tasks, one frame
    e = Engine(dev, max_frames=1, solver_path=2)
    e.bind(0, DeviceFrame.from_scene(sc, dev))
    _lib.check(e.lib.slm_set_beta(e.h, 0, bt.data_ptr(), e.stream), "slm_set_beta")
    jtj = torch.zeros((P, P), dtype=torch.float64, device="cuda")
    jtl = torch.zeros(P, dtype=torch.float64, device="cuda")
    _lib.check(e.lib.slm_assemble(e.h, 0, jtj.data_ptr(), jtl.data_ptr(), e.stream), "slm_assemble")
    torch.cuda.synchronize()
    res["jtj"], res["jtl"] = jtj.cpu().numpy(), jtl.cpu().numpy()
    deltas, status = [], []
    for _ in range(2):
        delta = torch.zeros(P, dtype=torch.float64, device="cuda")
        st = torch.full((1,), -7, dtype=torch.int32, device="cuda")
        _lib.check(e.lib.slm_solve(e.h, 0, U, delta.data_ptr(), st.data_ptr(), e.stream), "slm_solve")
        torch.cuda.synchronize()
        deltas.append(delta.cpu().numpy())
        status.append(int(st.item()))
    res["a_delta"], res["a_status"] = np.stack(deltas), np.array(status)
    res["a_form"] = e.lib.slm_debug_last_solver_form(e.h)
    res["a_plan"] = np.array([int(e.plan_info(0)["fronts"]), int(e.plan_info(0)["levels"])])
    e.close()

    # ---- (b) the hybrid form, eight slots of the same frame: one train-phase iteration at u0 = U is always accepted, so
    # beta - (the beta slm_set_beta gave the slot) is the slot's delta
    e = Engine(dev, max_frames=SLOTS, num_iterations=1, phase_test=False, u0=U, solver_path=4)
    e.bind_batch([DeviceFrame.from_scene(sc, dev) for _ in range(SLOTS)])
    runs, recs = [], []
    for _ in range(2):
        for i in range(SLOTS):
            _lib.check(e.lib.slm_set_beta(e.h, i, bt.data_ptr(), e.stream), "slm_set_beta")
        e.run(SLOTS)
        runs.append(np.stack([e.beta(i).cpu().numpy().reshape(-1) - beta0.reshape(-1) for i in range(SLOTS)]))
        recs.append([[r["status"], int(r["accepted"])] for i in range(SLOTS) for r in e.records(i)])
    res["b_delta"], res["b_records"] = np.stack(runs), np.array(recs)
    res["b_form"] = e.lib.slm_debug_last_solver_form(e.h)
    res["b_mode"] = e.lib.slm_debug_last_dag_mode(e.h)
    res["b_plan"] = np.array([int(e.plan_info(0)["fronts"]), int(e.plan_info(0)["levels"])])
    res["cus"] = torch.cuda.get_device_properties(0).multi_processor_count
    res["timeout_status"] = _lib.SLM_ITER_SOLVER_TIMEOUT
    e.close()
    np.savez(out, **res)


@pytest.mark.parametrize("name", list(CASES))
def test_every_task_kind_in_one_solve_matches_the_dense_solve(name, tmp_path):
    (kind, arg), leaf = CASES[name]
    sc = _scene(kind, arg)
    P = 7 * sc.J
    out = str(tmp_path / "kinds.npz")
    env = dict(os.environ, SLM_ND_LEAF=str(leaf))
    for k in ("SLM_DAG_XCD", "SLM_DAG_TOP_FRONTS", "SLM_BACK_FUSE_NPT", "SLM_DAG_MAX_NODES", "SLM_HYBRID"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "python-super_amd"), os.path.join(ROOT, "tests")] +
                                        [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    run = subprocess.run([sys.executable, os.path.abspath(__file__), name, out], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(out)

    # ---- the plan has every task kind, in both forms (the same leaf size: SLM_ND_LEAF)
    fr = got["fronts"]
    depth, npt, nbt = fr[:, 0], (7 * fr[:, 1] + 63) // 64, (7 * fr[:, 2] + 63) // 64
    print(f"MEASURE {name} J={sc.J} fronts (depth, pivot columns, boundary rows) = {sorted(zip(depth.tolist(), npt.tolist(), nbt.tolist()))}")
    assert tuple(got["a_plan"]) == tuple(got["b_plan"]) == (len(fr), int(depth.max()) + 1)
    assert {1, 2} <= set(npt.tolist()) and npt.max() >= 3                # POTRF: first column only / one streamed column / a chain
    assert (nbt > 0).any()                                               # COL of boundary rows, SCHUR
    assert ((nbt > 0) & (npt > BACK_FUSE_NPT)).any()                     # BACKB + plain BACK
    assert ((nbt > 0) & (npt <= BACK_FUSE_NPT)).any()                    # fused BACK
    assert ((nbt == 0) & (npt >= 2)).any()                               # the root: BACK over a chain, no boundary
    # form (b): per-level launches below the cut, so the kinds above must occur at the depths that run as tasks -- the levels
    # from the root down to the deepest one with at most four fronts (slm_nd_host.hip, SLM_DAG_TOP_FRONTS) -- except the back
    # substitution, which runs as tasks for the whole tree
    per_depth = np.bincount(depth)
    cut = min(max(d for d in range(len(per_depth)) if (per_depth[: d + 1] <= 4).all()), len(per_depth) - 2)
    top = depth <= cut
    assert cut + 1 < len(per_depth) and npt[top].max() >= 3 and {1, 2} <= set(npt[top].tolist()) and (nbt[top] > 0).any()

    own = np.linalg.solve(got["jtj"] + U * np.eye(P), got["jtl"])
    assert np.abs(own).max() > 0.005

    # ---- (a)
    d, status = got["a_delta"], got["a_status"]
    print(f"MEASURE {name} (a) form={int(got['a_form'])} status={status.tolist()} own_matrix={np.abs(d[0] - own).max():.3e} "
          f"run2={np.abs(d[1] - d[0]).max():.3e}")
    assert int(got["a_form"]) == 1
    assert (status == 0).all(), status                                   # 1: a non-positive pivot, 2: a wait timed out
    np.testing.assert_allclose(d[0], own, rtol=0, atol=1e-11)
    assert d[1].tobytes() == d[0].tobytes()

    # ---- (b)
    d, recs = got["b_delta"], got["b_records"]
    print(f"MEASURE {name} (b) form={int(got['b_form'])} mode={int(got['b_mode'])} records (status, accepted)={np.unique(recs.reshape(-1, 2), axis=0).tolist()} "
          f"own_matrix={np.abs(d[0] - own).max():.3e} run2={np.abs(d[1] - d[0]).max():.3e} slots={np.abs(d[0] - d[0][:1]).max():.3e}")
    assert int(got["b_form"]) == 2
    assert int(got["b_mode"]) == (1 if int(got["cus"]) == 256 else 0)    # 8 XCDs: the XCD-affine ticket streams were taken
    assert recs.shape == (2, SLOTS, 2)
    assert (recs[..., 0] != int(got["timeout_status"])).all()
    assert (recs[..., 0] == 0).all() and (recs[..., 1] == 1).all(), recs
    for i in range(SLOTS):
        np.testing.assert_allclose(d[0][i], own, rtol=0, atol=1e-11, err_msg=f"slot {i}")
        assert d[0][i].tobytes() == d[0][0].tobytes(), i                 # the same frame on another XCD's stream
    assert d[1].tobytes() == d[0].tobytes()


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
