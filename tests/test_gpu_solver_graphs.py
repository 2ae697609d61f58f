"""The multifrontal solver on the node graphs of tests/solver_graph_cases.py -- grid sizes at the edges of the plan constants,
relabelled / disconnected / hub / coincident / random dense graphs, self references and duplicates in the node KNN table --
against a dense Cholesky solve of the ORACLE's normal equations: one damped solve per case and solver form (no LM loop that
could correct a slightly wrong step), every slot of eight-frame batches in every batch form, and a zero pivot placed in the
first leaf and in the root front.  Through the C ABI.  Needs an MI355X (-m gpu).

Each test prints one ``MEASURE`` line per comparison (run with -s to see them).  Largest values seen on the MI355X:
MEASURED below."""
import numpy as np
import pytest

import solver_graph_cases as sgc

pytestmark = pytest.mark.gpu

U = sgc.U_SOLVE
FORM_OF_PATH = {3: 0, 2: 1, 1: -1, 0: 1}        # slm_debug_last_solver_form of a ONE-slot solver: per-level, task graph, band (none)
LEAF_OF_PATH = {3: 0, 4: 0, 2: 1, 0: 1}         # index into sgc.PLANS[name]: 18-node leaves / 50-node leaves (one slot, small batches)
# Largest figures over all cases, solver paths and batch slots of this file, measured on an MI355X: forward error against the
# oracle (bound 1e-9 max(1, |ref|)), backward error as a multiple of P eps (bound 64), against the dense solve of the library's
# own slm_assemble matrix (bound 1e-11).
MEASURED = dict(forward=5.0e-15, backward_in_P_eps=0.025, own_matrix=4.3e-14, batch_against_single_slot=7.3e-14)


def _engine(**kw):
    import torch
    from super_amd.engine import Engine
    return Engine(torch.device("cuda", 0), **kw)


class _closing:
    """``with _closing(_engine(...)) as e``: the solver handle is destroyed also when an assertion fails"""
    def __init__(self, e):
        self.e = e

    def __enter__(self):
        return self.e

    def __exit__(self, *exc):
        self.e.close()


def _dframe(sc):
    import torch
    from super_amd.engine import DeviceFrame
    return DeviceFrame.from_scene(sc, torch.device("cuda", 0))


def _set_beta(e, slot, beta):
    import torch
    from super_amd import _lib
    bt = torch.from_numpy(np.ascontiguousarray(beta)).cuda()
    _lib.check(e.lib.slm_set_beta(e.h, slot, bt.data_ptr(), e.stream), "slm_set_beta")
    torch.cuda.synchronize()                    # bt may go out of scope


def _solve(e, sc, own_matrix=True):
    """slm_solve(u = U) of slot 0 at its current beta -> (delta, status, form, dense solve of the library's own matrix)"""
    import torch
    from super_amd import _lib
    P = 7 * sc.J
    own = None
    if own_matrix:
        jtj = torch.zeros((P, P), dtype=torch.float64, device="cuda")
        jtl = torch.zeros(P, dtype=torch.float64, device="cuda")
        _lib.check(e.lib.slm_assemble(e.h, 0, jtj.data_ptr(), jtl.data_ptr(), e.stream), "slm_assemble")
        own = np.linalg.solve(jtj.cpu().numpy() + U * np.eye(P), jtl.cpu().numpy())
    delta = torch.zeros(P, dtype=torch.float64, device="cuda")
    status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(e.lib.slm_solve(e.h, 0, U, delta.data_ptr(), status.data_ptr(), e.stream), "slm_solve")
    return delta.cpu().numpy(), int(status.item()), e.lib.slm_debug_last_solver_form(e.h), own


def _check_against_oracle(tag, d, ref):
    """the two error checks of every comparison with the oracle: forward 1e-9 max(1, |ref|), backward 64 P eps"""
    A, b, want, norm2 = ref
    P = len(b)
    fwd = float(np.abs(d - want).max())
    bwd = sgc.backward_error(A, b, d, norm2)
    print(f"MEASURE {tag} P={P} forward={fwd:.3e} backward={bwd:.3e} = {bwd / (P * np.finfo(np.float64).eps):.3f} P eps")
    assert np.isfinite(d).all(), tag
    np.testing.assert_allclose(d, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()), err_msg=tag)
    assert bwd <= sgc.backward_bound(P), (tag, bwd, sgc.backward_bound(P))


# ------------------------------------------------------------------------------------------- one slot, one damped solve
@pytest.mark.parametrize("sp", [3, 2, 1, 0])
@pytest.mark.parametrize("name", sgc.CASES)
def test_one_damped_solve_matches_the_dense_solve_of_the_oracle(name, sp):
    """bind, slm_set_beta(perturbed), slm_solve(u = 0.37) on every case and solver path: status OK; delta against the oracle's
    Cholesky solve (forward and backward error) and against a NumPy solve of the library's own slm_assemble matrix (which goes
    through the band, not the fronts: it isolates the solver from the assembly); the form that ran is the one the path
    promises, and the plan is the one the host analysis gives for this graph.

    self_and_dup (a node KNN table that names the node itself and one neighbour twice): the bind ACCEPTS it -- slm_bind_frame
    only refuses ids outside [0, J) and a repeated id in a SURFEL row -- so the solve must be right, like the oracle's (a self
    edge contributes nothing to ARAP, a duplicate counts twice).  hub, random_dense and self_and_dup have rows that list a
    neighbour twice: k_reg_grad_nd must write that neighbour's ARAP cross block from ONE lane, with its multiplicity (two
    lanes that read-modify-write the same entries lose an update: delta wrong by 1e-2 on the fronts, right on the band)."""
    sc = sgc.case(name)
    with _closing(_engine(solver_path=sp)) as e:
        e.bind(0, _dframe(sc))
        _set_beta(e, 0, sgc.perturbed_beta(sc.J))
        d, status, form, own = _solve(e, sc)
        info = e.plan_info(0)
    print(f"MEASURE {name} sp={sp} form={form} solver={info['solver']!r} fronts={int(info['fronts'])} levels={int(info['levels'])} "
          f"own_matrix={np.abs(d - own).max():.3e}")
    assert status == 0
    assert form == FORM_OF_PATH[sp]
    if sp != 1:
        assert (int(info["fronts"]), int(info["levels"])) == sgc.PLANS[name][LEAF_OF_PATH[sp]]
    _check_against_oracle(f"{name} sp={sp}", d, sgc.reference(name))
    np.testing.assert_allclose(d, own, rtol=0, atol=1e-11)


@pytest.mark.parametrize("sp", [3, 2, 0])
@pytest.mark.parametrize("name", ["grid_j128", "hub", "random_dense"])
def test_a_solve_at_a_generic_beta_matches_the_library_s_own_matrix(name, sp):
    """sgc.perturbed_beta keeps the quaternions on a 2^-8 grid so that the oracle's float32 Rot term equals the library's.  Here
    the beta is NOT snapped -- generic low-order bits in the Rot blocks and the right-hand side -- and delta is compared with
    the dense solve of the library's own slm_assemble matrix alone (1e-11), which no rounding of the oracle enters."""
    sc = sgc.case(name)
    with _closing(_engine(solver_path=sp)) as e:
        e.bind(0, _dframe(sc))
        _set_beta(e, 0, sgc.generic_beta(sc.J))
        d, status, form, own = _solve(e, sc)
    print(f"MEASURE generic {name} sp={sp} own_matrix={np.abs(d - own).max():.3e}")
    assert status == 0 and form == FORM_OF_PATH[sp] and np.abs(own).max() > 0.005
    np.testing.assert_allclose(d, own, rtol=0, atol=1e-11)


# ------------------------------------------------------------------------------------------- batches: every slot
BATCHES = {"deep": sgc.DEEP_BATCH, "mixed": sgc.MIXED_BATCH}
# 8 slots x J <= 8 000: solver_path 0 runs ONE task graph; 4 the hybrid form when the trees have the same depth, else it falls
# back to the per-level launches (tests/test_solver_graph_cases.py pins the depths)
BATCH_FORM = {"deep": {0: 1, 4: 2, 2: 1, 3: 0}, "mixed": {0: 1, 4: 0, 2: 1, 3: 0}}


@pytest.mark.parametrize("sp", [0, 4, 2, 3])
@pytest.mark.parametrize("batch", list(BATCHES))
def test_every_slot_of_a_batch_matches_its_own_dense_solve(batch, sp):
    """Eight different graphs in one batch, one train-phase iteration at u0 = 0.37: the step is always accepted, so
    beta - (the beta that slm_set_beta gave the slot: it survives into slm_run, which continues from the slot's state) is the
    slot's delta.  Every slot against the oracle solve of ITS frame.  The form that ran is asserted, so that a silent
    fall-back cannot turn the four solver paths into runs of one form: over the two batches the task graph (1), the
    per-level launches (0) and the hybrid form (2) each run."""
    names = BATCHES[batch]
    scs = [sgc.case(n) for n in names]
    with _closing(_engine(max_frames=8, num_iterations=1, phase_test=False, u0=U, solver_path=sp)) as e:
        e.bind_batch([_dframe(sc) for sc in scs])
        for i, sc in enumerate(scs):
            _set_beta(e, i, sgc.perturbed_beta(sc.J))
        e.run(8)
        form = e.lib.slm_debug_last_solver_form(e.h)
        out = [(e.beta(i).cpu().numpy(), e.records(i), e.plan_info(i)) for i in range(8)]
    print(f"MEASURE batch={batch} sp={sp} form={form} levels={[int(o[2]['levels']) for o in out]} fronts={[int(o[2]['fronts']) for o in out]}")
    assert form == BATCH_FORM[batch][sp]
    for i, (name, sc) in enumerate(zip(names, scs)):
        beta, recs, info = out[i]
        assert len(recs) == 1 and recs[0]["status"] == 0 and recs[0]["accepted"] and recs[0]["u"] == U, (name, recs)
        assert (int(info["fronts"]), int(info["levels"])) == sgc.PLANS[name][LEAF_OF_PATH[sp]]
        _check_against_oracle(f"batch={batch} sp={sp} slot={i} {name}", (beta - sgc.perturbed_beta(sc.J)).reshape(-1), sgc.reference(name))


# ------------------------------------------------------------------------------------------- the split panel column
def test_the_split_panel_column_matches_the_dense_solve_of_the_oracle(tmp_path):
    """k_fpotrf + k_ftrsm, the split form of a tile column of the per-level launches: launch_front_levels takes it in a level
    that does not run the compact form when (max_nt - c) * n_fronts * n_frames > 512, which no batch above reaches (deep: at
    most 8 x 8 x 4 = 256).  Eight slots of sgc.split_column_case() under SLM_COMPACT_MIN=1000000 (no level compact; read once
    per process, hence the child), solver_path 3, one train-phase iteration at u0 = 0.37 from the perturbed beta: every slot
    against the oracle's dense solve of the frame, with the two bounds of this file.  That the split form runs -- and the
    fused one too, in the same solve -- is asserted on the level schedule of the host analysis, so a plan change fails here
    instead of silently running one form only; the plan the bind built is checked against that schedule."""
    import os
    import subprocess
    import sys
    sc = sgc.split_column_case()
    sched = sgc.host_level_schedule(sc)
    blocks = [(nt - c) * n * 8 for n, npt, nt in sched for c in range(npt)]      # workgroups of a fused panel launch, per tile column
    print(f"MEASURE split_column levels (n_fronts, max_npt, max_nt) = {sched}, fused panel workgroups per column = {blocks}")
    assert max(blocks) >= 512 + 128 and min(blocks) <= 512, blocks               # split with room to spare, and fused
    assert any(nt - c > 1 for n, npt, nt in sched for c in range(npt) if (nt - c) * n * 8 > 512)   # k_ftrsm has tiles to solve
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "split.npz")
    code = (
        "import sys, numpy as np, torch\n"
        f"sys.path[:0] = [{root!r}, {os.path.join(root, 'python-super_amd')!r}, {os.path.join(root, 'tests')!r}]\n"
        "import solver_graph_cases as sgc\n"
        "from super_amd import _lib\n"
        "from super_amd.engine import DeviceFrame, Engine\n"
        "dev = torch.device('cuda', 0)\n"
        "sc = sgc.split_column_case()\n"
        "e = Engine(dev, max_frames=8, num_iterations=1, phase_test=False, u0=sgc.U_SOLVE, solver_path=3)\n"
        "e.bind_batch([DeviceFrame.from_scene(sc, dev) for _ in range(8)])\n"
        "bt = torch.from_numpy(np.ascontiguousarray(sgc.perturbed_beta(sc.J))).cuda()\n"
        "for i in range(8):\n"
        "    _lib.check(e.lib.slm_set_beta(e.h, i, bt.data_ptr(), e.stream), 'slm_set_beta')\n"
        "e.run(8)\n"
        "recs = [e.records(i) for i in range(8)]\n"
        "info = e.plan_info(0)\n"
        f"np.savez({out!r}, beta=np.stack([e.beta(i).cpu().numpy() for i in range(8)]), form=e.lib.slm_debug_last_solver_form(e.h),\n"
        "         ok=[len(r) == 1 and r[0]['status'] == 0 and bool(r[0]['accepted']) and r[0]['u'] == sgc.U_SOLVE for r in recs],\n"
        "         plan=[int(info['fronts']), int(info['levels'])])\n"
        "e.close()\n")
    env = dict(os.environ, SLM_COMPACT_MIN="1000000")
    run = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = np.load(out)
    assert int(got["form"]) == 0 and got["ok"].all(), (got["form"], got["ok"])
    assert tuple(got["plan"]) == (sum(n for n, _, _ in sched), len(sched))
    ref = sgc.reference("split_column")
    for i in range(8):
        _check_against_oracle(f"split_column slot={i}", (got["beta"][i] - sgc.perturbed_beta(sc.J)).reshape(-1), ref)


# ------------------------------------------------------------------------------------------- failure placement
ROT = dict(use_arap=False, use_rot=True, u0=0.0)           # sgc.FAIL_OPT_ROT: the chosen node's qx pivot is the ONLY zero pivot
DATA = dict(use_arap=False, use_rot=False, u0=0.0)         # sgc.FAIL_OPT_DATA: every node has a zero pivot (see solver_graph_cases)
N_IT = 4
FAIL_FORM_ONE = {3: 0, 2: 1, 4: 2, 0: 1}                   # one slot: 4 runs the hybrid form (three or four levels at 18-node leaves)
FAIL_FORM_BATCH = {3: 0, 2: 1, 4: 2, 0: 1}                 # eight slots x 48 nodes: 0 runs one task graph


def _assert_stopped(e, slot, J):
    from super_amd import _lib
    recs = e.records(slot)
    assert recs[0]["status"] == _lib.SLM_ITER_SOLVER_FAILED, recs
    assert len(recs) == N_IT and all(r["status"] == _lib.SLM_ITER_NOT_RUN for r in recs[1:]), recs
    got = e.beta(slot).cpu().numpy()
    assert got.tobytes() == sgc.identity_beta(J).tobytes()                      # bitwise, -0.0 included


@pytest.mark.parametrize("sp", [3, 2, 4, 0])
@pytest.mark.parametrize("cfg", ["rot", "data"])
@pytest.mark.parametrize("name", sgc.FAILURES_ALL)
def test_a_zero_pivot_stops_the_loop_wherever_it_sits(name, cfg, sp):
    """One node without surfels, u0 = 0, one slot.  `rot` (data + Rot term): the node's block is diag(4, 0, ..., 0) with zero
    off-diagonal rows and every other pivot is positive, so the factorisation meets exactly one zero pivot -- in a leaf of
    the tree for fail_corner, in the ROOT front for fail_root, where the flag has furthest to travel (paths 3 and 4: five
    fronts, three levels; paths 2 and 0: one front of six tile columns, the node in column 0 / column 2) -- and for
    fail_root_j128 in the root front of a real tree in EVERY form (paths 3 and 4: 13 fronts, four levels; the task graph of
    paths 2 and 0: five fronts, three levels).  `data` (the data
    term alone, as in test_solver_failure_stops_like_the_reference): the same frames fail too, but every node's qw pivot is zero there.
    Iteration 0 records SLM_ITER_SOLVER_FAILED, the others SLM_ITER_NOT_RUN, beta stays the identity bitwise.  These are
    ordinary 'not positive definite' exits.  With u = 0.37 the same frame solves and matches the dense solve."""
    sc = sgc.failure_case(name)
    kw = ROT if cfg == "rot" else DATA
    with _closing(_engine(solver_path=sp, num_iterations=N_IT, **kw)) as e:
        e.bind(0, _dframe(sc))
        d, status, form, _ = _solve(e, sc, own_matrix=False)
        assert status == 0 and form == FAIL_FORM_ONE[sp]
        opt_kw = sgc.FAIL_OPT_ROT if cfg == "rot" else sgc.FAIL_OPT_DATA
        _check_against_oracle(f"{name} {cfg} sp={sp} u={U}", d, sgc.reference(name, "identity", opt_kw))
        e.bind(0, _dframe(sc))
        e.run(1)
        assert e.lib.slm_debug_last_solver_form(e.h) == FAIL_FORM_ONE[sp]
        info = e.plan_info(0)
        if name == "fail_root_j128":
            assert (int(info["fronts"]), int(info["levels"])) == ((13, 4) if sp in (3, 4) else (5, 3))
        _assert_stopped(e, 0, sc.J)


@pytest.fixture(scope="module")
def healthy_singles():
    """the seven healthy frames of the failure batches, each solved alone (one slot, default solver path), once"""
    out = []
    for k in range(7):
        sc = sgc.healthy_case(k)
        with _closing(_engine(num_iterations=N_IT, **ROT)) as e:
            e.bind(0, _dframe(sc))
            e.run(1)
            out.append((e.beta(0).cpu().numpy(), e.records(0)))
    return out


@pytest.mark.parametrize("sp", [3, 2, 4, 0])
@pytest.mark.parametrize("name", sgc.FAILURES)
def test_a_zero_pivot_in_slot_3_leaves_the_other_slots_alone(name, sp, healthy_singles):
    """the failing frame as slot 3 of eight: it stops like above; the seven healthy slots finish all their iterations and
    equal their single-slot runs to the 1e-6 of test_ragged_batch_and_k_ed_variants"""
    scs = [sgc.healthy_case(k) for k in range(7)]
    scs.insert(3, sgc.failure_case(name))
    with _closing(_engine(max_frames=8, solver_path=sp, num_iterations=N_IT, **ROT)) as e:
        e.bind_batch([_dframe(sc) for sc in scs])
        e.run(8)
        assert e.lib.slm_debug_last_solver_form(e.h) == FAIL_FORM_BATCH[sp]
        _assert_stopped(e, 3, scs[3].J)
        for k, slot in enumerate([0, 1, 2, 4, 5, 6, 7]):
            want_beta, want_recs = healthy_singles[k]
            recs = e.records(slot)
            assert len(recs) == N_IT and len(want_recs) == N_IT
            assert all(r["status"] == 0 for r in recs) and all(r["status"] == 0 for r in want_recs), (slot, recs)
            assert [r["accepted"] for r in recs] == [r["accepted"] for r in want_recs] and any(r["accepted"] for r in recs)
            got = e.beta(slot).cpu().numpy()
            print(f"MEASURE {name} sp={sp} slot={slot} batch-single={np.abs(got - want_beta).max():.3e}")
            np.testing.assert_allclose(got, want_beta, rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------- RECORD
# One run of this file on an MI355X (125 passed).  Per case: the plan (fronts, levels) that plan_info reports under solver_path 3
# and under 2 / 0, the form that ran under solver_path 3 / 2 / 1 / 0 (0 per-level launches, 1 task graph, -1 band), and the
# largest forward error, backward error and distance to the dense solve of the library's own matrix over the four paths; then the
# same two errors over the slots of the eight-frame batches the case is part of, and per batch the form and the slots' plans.
# case             fronts,levels sp 3 | 2, 0   form sp 3/2/1/0   forward    backward   own matrix   in batches: forward  backward
# grid_j4          (1, 1)   | (1, 1)          0/1/-1/1         2.0e-16    0.025 P eps  4.4e-16     2.0e-16  0.024 P eps
# grid_j9          (1, 1)   | (1, 1)          0/1/-1/1         7.1e-16    0.017 P eps  6.8e-16     -
# grid_j10         (1, 1)   | (1, 1)          0/1/-1/1         4.2e-16    0.009 P eps  3.4e-16     -
# grid_j18         (1, 1)   | (1, 1)          0/1/-1/1         7.2e-16    0.007 P eps  1.4e-15     -
# grid_j19         (3, 2)   | (1, 1)          0/1/-1/1         2.6e-15    0.014 P eps  6.1e-15     2.7e-15  0.014 P eps
# grid_j50         (5, 3)   | (1, 1)          0/1/-1/1         1.8e-15    0.002 P eps  3.8e-15     -
# grid_j51         (5, 3)   | (3, 2)          0/1/-1/1         4.0e-15    0.003 P eps  3.9e-15     4.0e-15  0.003 P eps
# grid_j64         (7, 3)   | (3, 2)          0/1/-1/1         3.3e-15    0.002 P eps  7.3e-15     3.3e-15  0.002 P eps
# grid_j97         (15, 4)  | (3, 2)          0/1/-1/1         2.6e-15    0.001 P eps  4.7e-15     2.6e-15  0.001 P eps
# grid_j100        (11, 4)  | (3, 2)          0/1/-1/1         3.3e-15    0.001 P eps  2.3e-14     3.0e-15  0.001 P eps
# grid_j128        (13, 4)  | (5, 3)          0/1/-1/1         3.0e-15    0.001 P eps  1.2e-14     3.0e-15  0.001 P eps
# grid_j64_k6      (5, 3)   | (3, 2)          0/1/-1/1         4.8e-15    0.003 P eps  4.8e-15     -
# shuffled         (13, 4)  | (5, 3)          0/1/-1/1         4.6e-15    0.001 P eps  1.6e-14     3.1e-15  0.001 P eps
# islands          (15, 4)  | (7, 3)          0/1/-1/1         3.1e-15    0.001 P eps  7.2e-15     3.2e-15  0.001 P eps
# hub              (13, 4)  | (5, 3)          0/1/-1/1         1.9e-15    0.000 P eps  1.4e-14     1.6e-15  0.000 P eps
# coincident       (11, 4)  | (5, 3)          0/1/-1/1         4.8e-15    0.001 P eps  1.7e-14     4.6e-15  0.001 P eps
# random_dense     (1, 1)   | (1, 1)          0/1/-1/1         2.4e-15    0.003 P eps  4.0e-15     -
# random_dense_k4  (1, 1)   | (1, 1)          0/1/-1/1         2.8e-15    0.003 P eps  3.0e-15     9.1e-16  0.003 P eps
# self_and_dup     (13, 4)  | (5, 3)          0/1/-1/1         3.3e-15    0.001 P eps  1.1e-14     2.5e-15  0.001 P eps
# batch=deep sp=0 form=1 levels=[2, 2, 3, 3, 3, 3, 3, 3] fronts=[3, 3, 5, 5, 7, 5, 5, 5]
# batch=deep sp=4 form=2 levels=[4, 4, 4, 4, 4, 4, 4, 4] fronts=[15, 11, 13, 13, 15, 13, 11, 13]
# batch=deep sp=2 form=1 levels=[2, 2, 3, 3, 3, 3, 3, 3] fronts=[3, 3, 5, 5, 7, 5, 5, 5]
# batch=deep sp=3 form=0 levels=[4, 4, 4, 4, 4, 4, 4, 4] fronts=[15, 11, 13, 13, 15, 13, 11, 13]
# batch=mixed sp=0 form=1 levels=[3, 3, 3, 1, 1, 1, 2, 2] fronts=[5, 7, 5, 1, 1, 1, 3, 3]
# batch=mixed sp=4 form=0 levels=[4, 4, 4, 1, 1, 2, 3, 3] fronts=[13, 15, 13, 1, 1, 3, 5, 7]
# batch=mixed sp=2 form=1 levels=[3, 3, 3, 1, 1, 1, 2, 2] fronts=[5, 7, 5, 1, 1, 1, 3, 3]
# batch=mixed sp=3 form=0 levels=[4, 4, 4, 1, 1, 2, 3, 3] fronts=[13, 15, 13, 1, 1, 3, 5, 7]
# split_column (J = 384, P = 2 688, eight slots, SLM_COMPACT_MIN=1000000, sp 3, form 0): levels (n_fronts, max_npt, max_nt) =
#   [(6, 2, 5), (16, 2, 6), (8, 2, 6), (4, 2, 6), (2, 2, 5), (1, 3, 3)], fused panel workgroups per tile column = [240, 192, 768, 640,
#   384, 320, 192, 160, 80, 64, 24, 16, 8] (768 and 640 run k_fpotrf + k_ftrsm); every slot forward 3.8e-15, backward 0.000 P eps
#   (1.7e-16).  With it the file has 126 tests (10.6 s on the MI355X).
#
# What the file sees of a wrong factorisation.  On a scratch build the extend-add of child 1 was skipped in the last tile row of
# every parent tile gathered by the per-level launches (pull_tile in slm_front.hip): 25 of the 125 tests failed, every one of
# them on the per-level form and none on another -- solver_path 3 of grid_j50, j51, j64, j97, j100, j128, grid_j64_k6, shuffled,
# islands, hub, coincident and self_and_dup (forward error 3e-3 .. 6e-2, backward 2e9 .. 4e10 P eps; the cases of one front, and
# grid_j19 whose root is a single tile, have no such tile), the generic-beta solves of grid_j128 and hub on path 3, the batches
# deep-3, mixed-3 and mixed-4 (the fall-back to per-level launches), and the u = 0.37 solves of all failure frames on path 3.
