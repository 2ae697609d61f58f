"""The node graphs of tests/solver_graph_cases.py on the CPU: every frame is admissible for a bind, the oracle alone stays far
inside the tolerances that tests/test_gpu_solver_graphs.py holds the solver to, the failure frames fail where they are meant to,
and the symbolic plans (the host analysis of csrc/slm_nd_host.hip, compiled for the host) have the shapes the cases are for."""
import numpy as np
import pytest
from scipy.linalg import cho_factor

import solver_graph_cases as sgc
from oracle import lm_oracle as orc

EPS = np.finfo(np.float64).eps


def _all_scenes():
    return ([(n, sgc.case(n)) for n in sgc.CASES] + [(n, sgc.failure_case(n)) for n in sgc.FAILURES_ALL]
            + [(f"healthy{k}", sgc.healthy_case(k)) for k in range(7)])


def test_every_frame_is_admissible():
    """what slm_bind_frame demands (and the reference's top-k guarantees): ids in [0, J), K distinct ids per surfel row, J >= K;
    and weight rows that sum to 1 (float32 storage: K roundings of at most 2^-24 each)"""
    for name, sc in _all_scenes():
        J, K = sc.J, sc.sf_knn_idx.shape[1]
        assert 1500 <= sc.N <= 3000 and J >= K, name
        assert sc.sf_knn_idx.dtype == np.int64 and sc.ed_knn_idx.dtype == np.int64, name
        assert sc.sf_knn_idx.min() >= 0 and sc.sf_knn_idx.max() < J, name
        assert sc.ed_knn_idx.min() >= 0 and sc.ed_knn_idx.max() < J, name
        assert sc.ed_knn_idx.shape == (J, min(sc.ed_knn_idx.shape[1], J - 1)) and sc.ed_knn_w.shape == sc.ed_knn_idx.shape, name
        srt = np.sort(sc.sf_knn_idx, axis=1)
        assert (srt[:, 1:] != srt[:, :-1]).all(), (name, "a surfel row repeats an id")
        for w in (sc.sf_knn_w, sc.ed_knn_w):
            assert w.dtype == np.float32 and (w > 0).all(), name
            np.testing.assert_allclose(w.astype(np.float64).sum(axis=1), 1.0, rtol=0, atol=w.shape[1] * 2.0 ** -24, err_msg=name)
        for a in (sc.sf_points, sc.ed_points, sc.ed_norms, sc.ed_radii):
            assert a.dtype == np.float32 and np.isfinite(a).all(), name


def test_the_named_topologies_are_what_they_say():
    grid = sgc._scene(128, 3000, 310)                       # the scene `shuffled` relabels
    sh = sgc.case("shuffled")
    p = sh.meta["new_of_old"]
    assert not (p == np.arange(128)).all()
    np.testing.assert_array_equal(sh.ed_points[p], grid.ed_points)
    np.testing.assert_array_equal(sh.ed_knn_idx[p], p[grid.ed_knn_idx])
    np.testing.assert_array_equal(sh.ed_knn_w[p], grid.ed_knn_w)
    np.testing.assert_array_equal(sh.sf_knn_idx, p[grid.sf_knn_idx])
    # ... so the oracle's system is the grid's, symmetrically permuted
    A, b, d, _ = sgc.reference("shuffled")
    JtJ, jtl, _ = orc.normal_equations(orc.Frame.from_scene(grid), sgc.perturbed_beta(128)[p], orc.default_opt())
    rows = (7 * p[:, None] + np.arange(7)).reshape(-1)
    np.testing.assert_allclose(A[np.ix_(rows, rows)] - sgc.U_SOLVE * np.eye(len(b)), JtJ, rtol=0, atol=1e-12 * np.abs(JtJ).max())
    np.testing.assert_allclose(b[rows], jtl, rtol=0, atol=1e-12 * np.abs(jtl).max())

    isl = sgc.case("islands")
    node_side, sf_side = sgc.island_sides(isl)
    assert node_side.sum() == 64 and 0.3 < sf_side.mean() < 0.7
    assert (node_side[isl.sf_knn_idx] == sf_side[:, None]).all() and (node_side[isl.ed_knn_idx] == node_side[:, None]).all()
    A = sgc.reference("islands")[0]
    rows = (7 * np.nonzero(node_side)[0][:, None] + np.arange(7)).reshape(-1)
    other = np.setdiff1d(np.arange(A.shape[0]), rows)
    assert (A[np.ix_(rows, other)] == 0).all()              # block diagonal: no pair crosses the cut

    hub = sgc.case("hub")
    assert (hub.ed_knn_idx[1:] == 0).any(axis=1).all()
    co = sgc.case("coincident")
    assert (co.ed_points[:32] == co.ed_points[0]).all() and len(np.unique(co.ed_points, axis=0)) == 128 - 31
    rd = sgc.case("random_dense")
    assert rd.sf_knn_idx.shape[1] == 8 and rd.ed_knn_idx.shape == (64, 8)
    assert (rd.ed_knn_idx == np.arange(64)[:, None]).any()                     # it lists a node as its own neighbour somewhere
    np.testing.assert_array_equal(rd.ed_knn_idx, sgc.case("random_dense_k4").ed_knn_idx)
    sd = sgc.case("self_and_dup")
    assert (sd.ed_knn_idx[:, 0] == np.arange(128)).all() and (sd.ed_knn_idx[:, 2] == sd.ed_knn_idx[:, 1]).all()
    assert sgc.case("grid_j97").meta["grid"] == (1, 97) and sgc.case("grid_j64_k6").sf_knn_idx.shape[1] == 6
    assert sgc.case("grid_j64_k6").ed_knn_idx.shape[1] == 8 and sgc.case("grid_j4").ed_knn_idx.shape[1] == 3


@pytest.mark.parametrize("name", sgc.CASES)
def test_the_reference_alone_stays_inside_the_caps(name):
    A, b, d, norm2 = sgc.reference(name)
    P = len(b)
    assert P == 7 * sgc.case(name).J
    np.testing.assert_allclose(A, A.T, rtol=0, atol=P * EPS * np.abs(A).max())
    ev = np.linalg.eigvalsh(A)
    assert ev[0] > 0 and ev[-1] / ev[0] <= 1e6, (name, ev[-1] / ev[0])
    assert abs(ev[-1] - norm2) <= 1e-12 * norm2
    np.testing.assert_allclose(d, np.linalg.solve(A, b), rtol=0, atol=1e-12)
    assert sgc.backward_error(A, b, d, norm2) <= P * EPS
    assert 0.005 < np.abs(d).max() < 0.1                    # a step of ordinary size: the absolute tolerances mean something


def test_failure_frames_fail_at_the_chosen_node_only():
    for name in sgc.FAILURES_ALL:
        sc, node = sgc.failure_case(name), sgc.FAIL_NODE[name]
        fr = orc.Frame.from_scene(sc)
        rows = np.arange(7 * node, 7 * node + 7)
        rest = np.setdiff1d(np.arange(7 * sc.J), rows)
        # the data term alone: the node's rows and columns are exactly zero; Cholesky fails, and solves once u is added
        JtJ, _, _ = orc.normal_equations(fr, sgc.identity_beta(sc.J), orc.default_opt(**dict(sgc.FAIL_OPT_DATA)))
        assert (JtJ[rows] == 0).all() and (JtJ[:, rows] == 0).all()
        with pytest.raises(np.linalg.LinAlgError):
            cho_factor(JtJ, lower=True)
        cho_factor(JtJ + sgc.U_SOLVE * np.eye(7 * sc.J), lower=True)
        # ... but without that node it is singular too (the qw column of every node is zero at the identity): see solver_graph_cases
        assert np.abs(JtJ[0::7]).max() == 0.0
        assert np.linalg.eigvalsh(JtJ[np.ix_(rest, rest)])[0] < 1e-12
        # data + Rot: the node's block is diag(4, 0 ...), everything else is positive definite
        JtJ, _, _ = orc.normal_equations(fr, sgc.identity_beta(sc.J), orc.default_opt(**dict(sgc.FAIL_OPT_ROT)))
        blk = np.zeros((7, 7))
        blk[0, 0] = 4.0
        np.testing.assert_array_equal(JtJ[np.ix_(rows, rows)], blk)
        assert (JtJ[np.ix_(rows, rest)] == 0).all() and (JtJ[np.ix_(rest, rows)] == 0).all()
        cho_factor(JtJ[np.ix_(rest, rest)], lower=True)
        assert np.linalg.cond(JtJ[np.ix_(rest, rest)]) < 1e8
        with pytest.raises(np.linalg.LinAlgError):
            cho_factor(JtJ, lower=True)
        cho_factor(JtJ + sgc.U_SOLVE * np.eye(7 * sc.J), lower=True)


def test_healthy_frames_of_the_failure_batches_solve_at_u0_zero():
    opt = orc.default_opt(num_optimize_iterations=4, **dict(sgc.FAIL_OPT_ROT))
    for k in range(7):
        trace = []
        orc.lm(orc.Frame.from_scene(sgc.healthy_case(k)), opt, u=0.0, trace=trace)
        assert len(trace) == 4 and all("loss" in t for t in trace), (k, trace)


def _plan(sc, leaf):
    return sgc.host_plan(sc, leaf)


def test_the_plan_table_is_written_for_the_leaf_sizes_of_the_library():
    assert (sgc.LEAF, sgc.LEAF_LATENCY) == (18, 50)


@pytest.mark.parametrize("name", sgc.CASES)
def test_symbolic_plans_have_the_shapes_the_cases_are_for(name):
    sc = sgc.case(name)
    got = []
    for leaf in (sgc.LEAF, sgc.LEAF_LATENCY):
        p = _plan(sc, leaf)
        got.append((p["fronts"], p["levels"]))
        assert (np.bincount(p["node_front"], minlength=p["fronts"]) == p["front_nv"]).all()      # every node is a pivot once
        assert p["front_depth"][-1] == 0 and (p["front_depth"][:-1] > 0).all()                   # the root is the last front
        if name == "islands":
            assert p["front_nv"][-1] == 0            # two islands: an EMPTY root separator, a root front without pivots
        if name.startswith("random_dense"):
            assert p["front_nv"].tolist() == [64]    # could not split: one dense front, far above either leaf size
    assert tuple(got) == sgc.PLANS[name], (name, got)


def test_batches_have_the_tree_depths_their_solver_forms_need():
    deep = {_plan(sgc.case(n), sgc.LEAF)["levels"] for n in sgc.DEEP_BATCH}
    assert deep == {4}                               # equal depth, more than one level: solver_path 4 runs the hybrid form
    mixed = {_plan(sgc.case(n), sgc.LEAF)["levels"] for n in sgc.MIXED_BATCH}
    assert mixed == {1, 2, 3, 4}                     # different depths: solver_path 4 falls back to the per-level launches
    for batch in (sgc.DEEP_BATCH, sgc.MIXED_BATCH):
        assert len(set(batch)) == 8 and {sgc.case(n).sf_knn_idx.shape[1] for n in batch} == {4}
        assert sum(sgc.case(n).J for n in batch) <= 8000           # solver_path 0: one task graph (slots x J <= 8 000)
    assert {"shuffled", "islands", "hub", "random_dense_k4"} <= set(sgc.MIXED_BATCH)
    fail = [_plan(sgc.failure_case(n), sgc.LEAF)["levels"] for n in sgc.FAILURES] + [_plan(sgc.healthy_case(k), sgc.LEAF)["levels"] for k in range(7)]
    assert set(fail) == {3}                          # the failure batches run the hybrid form under solver_path 4


def test_the_zero_pivot_sits_in_the_first_leaf_and_in_the_root_front():
    a = _plan(sgc.failure_case("fail_corner"), sgc.LEAF)
    f = a["node_front"][sgc.FAIL_NODE["fail_corner"]]
    assert a["fronts"] == 5 and a["front_is_leaf"][f] and a["front_depth"][f] > 0          # a leaf: nothing is eliminated before its front
    b = _plan(sgc.failure_case("fail_root"), sgc.LEAF)
    assert b["fronts"] == 5 and b["node_front"][sgc.FAIL_NODE["fail_root"]] == b["fronts"] - 1      # the root: the last front
    assert 0 < b["node_pos"][sgc.FAIL_NODE["fail_root"]] < b["front_nv"][-1] - 1                    # and inside its pivot chain
    for name in sgc.FAILURES:                        # 50-node leaves: one front, pivots in id order
        p = _plan(sgc.failure_case(name), sgc.LEAF_LATENCY)
        assert p["fronts"] == 1 and p["node_pos"][sgc.FAIL_NODE[name]] == sgc.FAIL_NODE[name]
    # the 8 x 16 grid: the node is a pivot of the root front of a tree of several levels at EITHER leaf size
    for leaf, shape in ((sgc.LEAF, (13, 4)), (sgc.LEAF_LATENCY, (5, 3))):
        p = _plan(sgc.failure_case("fail_root_j128"), leaf)
        node = sgc.FAIL_NODE["fail_root_j128"]
        assert (p["fronts"], p["levels"]) == shape and p["node_front"][node] == p["fronts"] - 1
        assert 0 < p["node_pos"][node] < p["front_nv"][-1] - 1
