"""The float64 model of the LM path's triangle-area face term (tests/lm_face_model.py) checked on the CPU: its Jacobian
against central differences, its loss against ``graphfit_oracle.face`` at a translation-only deformation, a degenerate
triangle, and the properties the GPU tests (tests/test_gpu_lm_face.py) rely on -- the weight rule that makes the term a
visible part of the system, traces without a rounding-level tie, and the small frame whose mesh supplies coupling that
neither the surfels nor the node graph have.  The scenes, meshes and weights of the GPU tests are defined here."""
import numpy as np
import pytest
import torch

import lm_face_model as lfm
from oracle import graphfit_oracle as gfo
from oracle import lm_oracle as orc
from super_amd import synth

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the scenes of the GPU tests ---------------------------------------------------------------------------------------
CLASSES = {4: 4, 6: 2}
SMALL_TRI = [(5, 0, 2), (5, 2, 10), (5, 10, 8), (5, 8, 0), (5, 3, 11), (5, 7, 0),   # node 5 in six triangles
             (1, 6, 11)]                                                              # collinear (node 6 is moved)
SMALL_EXTRA = (3, 8, 10)          # mesh B = mesh A + this far-apart triangle
SMALL_UNREFERENCED = 0            # no surfel references it (in the mesh: its diagonal block is the mesh's and the regularisers')
SMALL_IN_NO_TRIANGLE = (4, 9)


def scene_k(K):
    """1200 surfels, 40 nodes, ``num_neighbors`` K, with its grid mesh and semantic inputs (geometry as without them)"""
    return _cached(("k", K), lambda: synth.make_scene(N=1200, J=40, H=60, W=80, seed=60 + K, n_neighbors=K, src_border=4,
                                                      tgt_border=3, tgt_holes=0.01, semantic=True, num_classes=CLASSES[K]))


def small_scene():
    """N = 37, J = 12, one surfel neighbour and one node neighbour: no surfel couples two nodes and the node graph couples
    twelve adjacent pairs, so every cross pair of SMALL_TRI (none of them adjacent) is coupling only the mesh supplies"""
    def make():
        sc = synth.make_scene(N=37, J=12, H=60, W=80, seed=3, n_neighbors=1, n_ed_neighbors=1, src_border=6, tgt_border=3)
        idx = sc.sf_knn_idx.copy()
        idx[idx == SMALL_UNREFERENCED] = 1
        sc.sf_knn_idx = idx
        ed = sc.ed_points.copy()
        ed[6] = (0.5 * (ed[1].astype(np.float64) + ed[11].astype(np.float64))).astype(np.float32)
        sc.ed_points = ed
        return sc
    return _cached("small", make)


def small_mesh(extra=False):
    sc = small_scene()
    tri = np.array(SMALL_TRI + ([SMALL_EXTRA] if extra else []), dtype=np.int64).T
    e = sc.ed_points.astype(np.float64)
    c = np.cross(e[tri[1]] - e[tri[0]], e[tri[2]] - e[tri[0]])
    areas = (0.5 * np.sqrt((c ** 2).sum(1) + 1e-13)).astype(np.float32).astype(np.float64)
    return tri, areas


def mesh_of(K, kind):
    """the meshes of the GPU tests: the scene's own; its first half with areas 10 % larger; every third triangle with areas
    10 % smaller; the scene's own with a quarter of the areas (a strongly non-linear start: the trace holds rejects)"""
    tri, areas = lfm.scene_mesh(scene_k(K))
    if kind == "full":
        return tri, areas
    if kind == "half":
        return tri[:, :tri.shape[1] // 2].copy(), 1.1 * areas[:tri.shape[1] // 2]
    if kind == "third":
        return tri[:, ::3].copy(), 0.9 * areas[::3]
    if kind == "quarter":
        return tri, 0.25 * areas
    raise ValueError(kind)


def frame_of(sc):
    return orc.Frame.from_scene(sc)


def ref_beta(J):
    return lfm.random_beta(J, 17, rot=0.01, trans=0.002)


def pair_keys(sc, mesh=None):
    """the distinct keys max * J + min of a frame's surfel pairs and, with ``mesh``, of its triangles' pairs"""
    J, idx = sc.J, np.asarray(sc.sf_knn_idx)
    a, b = idx[:, :, None], idx[:, None, :]
    keys = set((np.maximum(a, b) * J + np.minimum(a, b)).reshape(-1).tolist())
    if mesh is not None:
        t = np.asarray(mesh[0])
        for x in range(3):
            for y in range(3):
                keys |= set((np.maximum(t[x], t[y]) * J + np.minimum(t[x], t[y])).tolist())
    return keys


def weight_of(K, kind="full"):
    """the weight rule of the GPU tests: lambda from the model such that the largest face entry of J^T J equals the largest
    entry of the data term's at the reference beta"""
    sc = scene_k(K)
    return _cached(("lam", K, kind), lambda: lfm.visible_weight(frame_of(sc), mesh_of(K, kind), ref_beta(sc.J), orc.default_opt()))


# (scene, mesh, weight factor, u0, v) of every GPU trace: the weight is factor x weight_of.  From the default damping
# (10, 7.5) these scenes converge in six iterations and the rest of the trace is rounding-level ties; from (100, 2) every
# one of the ten steps still lowers the loss by more than 1 %.  The last case starts far from its rest areas with little
# damping: three accepts, then seven decisive rejects.
DAMPING = (100.0, 2.0)
TRACE_CASES = [(4, "full", 3.0) + DAMPING, (6, "full", 3.0) + DAMPING, (4, "half", 1.0) + DAMPING, (4, "third", 1.0) + DAMPING,
               (4, "quarter", 3.0, 0.01, 2.0)]


# The eight-slot test runs ONE solver, so one weight, over unlike meshes: 3 x weight_of(4) of the scene's own mesh on every
# slot, the slots' meshes these kinds (None: a slot without a mesh), damping DAMPING.  Its single-slot runs are GPU traces too.
BATCH_K, BATCH_FACTOR = 4, 3.0
BATCH_KINDS = ["full", "half", "third", None, "third", "full", "half", "full"]


def batch_weight():
    return BATCH_FACTOR * weight_of(BATCH_K, "full")


def batch_trace_of(kind):
    def make():
        sc = scene_k(BATCH_K)
        trace, (u, v) = [], DAMPING
        mesh = None if kind is None else mesh_of(BATCH_K, kind)
        beta = lfm.lm_with_face(frame_of(sc), orc.default_opt(), mesh, batch_weight(), u=u, v=v, trace=trace)
        return beta, trace
    return _cached(("batch trace", kind), make)


def trace_of(K, kind, factor, u, v):
    def make():
        sc = scene_k(K)
        trace = []
        beta = lfm.lm_with_face(frame_of(sc), orc.default_opt(), mesh_of(K, kind), factor * weight_of(K, kind), u=u, v=v,
                                trace=trace)
        return beta, trace
    return _cached(("trace", K, kind, factor, u, v), make)


# ---- the model itself --------------------------------------------------------------------------------------------------
def test_jacobian_matches_central_differences():
    sc = scene_k(4)
    fr, mesh, lam = frame_of(sc), mesh_of(4, "third"), 37.0
    beta = lfm.random_beta(sc.J, 5)
    Jd, r = lfm.face_jacobian(fr, mesh, beta, lam)
    assert Jd.shape == (mesh[0].shape[1], 7 * sc.J) and np.abs(r).max() > 0
    assert not Jd.reshape(len(r), sc.J, 7)[:, :, :4].any()          # rotations do not enter
    h = 1e-6
    cols = [7 * j + 4 + i for j in range(sc.J) for i in range(3)]
    for col in cols[::3]:
        d = np.zeros(7 * sc.J)
        d[col] = h
        rp = lfm.face_term(fr, mesh[0], mesh[1], beta + d.reshape(-1, 7), lam).r
        rm = lfm.face_term(fr, mesh[0], mesh[1], beta - d.reshape(-1, 7), lam).r
        np.testing.assert_allclose(Jd[:, col], (rp - rm) / (2 * h), rtol=0, atol=1e-8 * max(1.0, np.abs(Jd).max()))
    assert (Jd != 0).sum(1).max() <= 9


@pytest.mark.parametrize("K", [4, 6])
def test_loss_equals_graphfit_oracle_with_the_squared_weight(K):
    sc = scene_k(K)
    fr, mesh, lam = frame_of(sc), lfm.scene_mesh(sc), 3.5
    rng = np.random.default_rng(2)
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (sc.J, 1))
    beta[:, 4:7] = rng.normal(0, 0.003, (sc.J, 3))                   # translation only, no global row
    mine, n = lfm.face_loss(fr, mesh, beta, lam)
    pb = gfo.Problem(sc)
    dv = torch.zeros((sc.J + 1, 7), dtype=torch.float64)
    dv[:, 0] = 1.0
    dv[:-1] = torch.from_numpy(beta)
    opt = gfo.default_opt(mesh_face=True, mesh_face_weight=lam ** 2)
    ref = gfo.total_loss(pb, dv, opt)[1]["face_losses"]
    assert n == sc.ed_triangles.shape[1] and mine > 0
    np.testing.assert_allclose(mine, float(ref), rtol=1e-12)


def test_collinear_triangle_gives_a_finite_row():
    sc = small_scene()
    fr, (tri, areas) = frame_of(sc), small_mesh()
    ident = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (sc.J, 1))
    t = lfm.face_term(fr, tri, areas, ident, 1.0, grad=True)
    k = len(SMALL_TRI) - 1
    assert tuple(tri[:, k]) == (1, 6, 11)
    assert np.isfinite(t.Jrow).all() and np.isfinite(t.r).all()
    assert t.A[k] < 1e-6 and t.A[k] >= 0.5 * np.sqrt(1e-13) and np.abs(t.Jrow[k]).max() < 1e-3
    # exactly degenerate: the area is the constant's, the gradient zero
    fr0 = frame_of(sc)
    fr0.ed_points = np.asarray(fr.ed_points, dtype=np.float64).copy()
    fr0.ed_points[[1, 6, 11]] = [[0, 0, 1], [0.5, 0, 1], [1, 0, 1]]
    t0 = lfm.face_term(fr0, tri[:, k:k + 1], areas[k:k + 1], ident, 1.0, grad=True)
    np.testing.assert_allclose(t0.A, 0.5 * np.sqrt(1e-13), rtol=1e-12)
    assert not t0.Jrow.any()


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,kind,factor,u,v", TRACE_CASES)
def test_weight_rule_makes_the_term_visible(K, kind, factor, u, v):
    sc = scene_k(K)
    fr, mesh, beta = frame_of(sc), mesh_of(K, kind), ref_beta(sc.J)
    lam = factor * weight_of(K, kind)
    only_data = orc.default_opt(mesh_arap=False, mesh_rot=False)
    data_max = np.abs(orc.normal_equations(fr, beta, only_data)[0]).max()
    face_max = np.abs(lfm.face_system(fr, mesh, beta, lam)[0]).max()
    invisible = np.abs(lfm.face_system(fr, mesh, beta, 1.0)[0]).max()
    print("lambda", lam, "largest entries: data", data_max, "face", face_max, "face at weight 1", invisible)
    assert invisible < 1e-2 * data_max                                # at weight 1 the term is lost beside the data term
    assert 0.1 * data_max <= face_max <= 10.0 * data_max


@pytest.mark.parametrize("K,kind,factor,u,v", TRACE_CASES)
def test_no_accept_decision_of_the_gpu_traces_is_a_tie(K, kind, factor, u, v):
    beta, trace = trace_of(K, kind, factor, u, v)
    assert len(trace) == 10 and all("loss" in t for t in trace)
    m = lfm.decision_margins(trace)
    acc = [t["accepted"] for t in trace]
    print("accepted", acc, "margins", m)
    assert (m > 1e-6).all()
    assert all(acc) or kind == "quarter"
    if kind == "quarter":
        assert acc == [True] * 3 + [False] * 7
    sc = scene_k(K)
    without = orc.lm(frame_of(sc), orc.default_opt(), u=u, v=v)
    assert np.abs(beta - without).max() > 1e-6                        # the term moves the solution


@pytest.mark.parametrize("kind", ["full", "half", "third", None])
def test_no_accept_decision_of_the_batch_traces_is_a_tie(kind):
    """the eight-slot GPU test's slots: every mesh kind at the batch's one weight, and the slot without a mesh"""
    assert set(BATCH_KINDS) == {"full", "half", "third", None}
    beta, trace = batch_trace_of(kind)
    m = lfm.decision_margins(trace)
    print(kind, "accepted", [t["accepted"] for t in trace], "margins", m)
    assert len(trace) == 10 and (m > 1e-6).all()
    if kind is not None:                                              # within 10x of the data term at this weight too
        sc = scene_k(BATCH_K)
        fr, b = frame_of(sc), ref_beta(sc.J)
        data_max = np.abs(orc.normal_equations(fr, b, orc.default_opt(mesh_arap=False, mesh_rot=False))[0]).max()
        face_max = np.abs(lfm.face_system(fr, mesh_of(BATCH_K, kind), b, batch_weight())[0]).max()
        assert 0.1 * data_max <= face_max <= 10.0 * data_max


def test_combined_traces_have_no_tie_either():
    import lm_corr_model as lcm
    import lm_weight_model as lwm
    sc = scene_k(4)
    fr, mesh, lam, opt = frame_of(sc), mesh_of(4, "full"), weight_of(4), orc.default_opt()
    flow = synth.smooth_flow(sc.H, sc.W, 24, amp=(2.0, 1.5))
    tg = lcm.targets_from_flow(fr, flow)
    assert 0.5 * sc.N < tg[2].sum() < sc.N
    trace = []
    u, v = DAMPING
    lfm.lm_with_face(fr, opt, mesh, lam, u=u, v=v, trace=trace, base=lfm.base_corr(fr, opt, tg, 2, 0.5))
    assert (lfm.decision_margins(trace) > 1e-6).all()
    sem, trace = lwm.sem_of(sc), []
    ne, tl = lfm.base_weighted(fr, opt, sem, 1)

    def checked(beta):
        lwm.check_conditions(lwm.weights(fr, sem, beta, 1, 0.0), 1, 0.0)
        return tl(beta)
    lfm.lm_with_face(fr, opt, mesh, lam, u=u, v=v, trace=trace, base=(ne, checked))
    assert (lfm.decision_margins(trace) > 1e-6).all()


def test_small_frame_gets_its_coupling_from_the_mesh_alone():
    sc = small_scene()
    tri, _ = small_mesh()
    assert sc.sf_knn_idx.shape == (37, 1) and sc.ed_knn_idx.shape == (12, 1)
    assert SMALL_UNREFERENCED not in sc.sf_knn_idx and SMALL_UNREFERENCED in tri
    assert (tri == 5).sum() == 6 and not np.isin(SMALL_IN_NO_TRIANGLE, tri).any()
    node_pairs = {(max(j, int(k)), min(j, int(k))) for j, k in enumerate(sc.ed_knn_idx[:, 0])}
    cross = set()
    for t in np.concatenate([tri.T, [SMALL_EXTRA]]):
        cross |= {(max(a, b), min(a, b)) for a in t for b in t if a != b}
    assert not (cross & node_pairs)
    base, with_a, with_b = pair_keys(sc), pair_keys(sc, small_mesh()), pair_keys(sc, small_mesh(True))
    assert len(base) == len(np.unique(sc.sf_knn_idx)) and len(with_a) > len(base) + 10 and len(with_b) == len(with_a) + 2
    # the mesh's blocks are a visible part of the small system too
    fr, beta = frame_of(sc), ref_beta(sc.J)
    lam = small_weight()
    A0 = orc.normal_equations(fr, beta, orc.default_opt())[0]
    Af = lfm.face_system(fr, small_mesh(), beta, lam)[0]
    assert np.abs(Af).max() > 1e-2 * np.abs(A0).max()
    off = [(7 * a + 4, 7 * b + 4) for a, b in cross if (a, b) not in {(8, 3), (10, 3)}]      # (those two: mesh B only)
    assert all(A0[i, j] == 0.0 for i, j in off) and any(Af[i, j] != 0.0 for i, j in off)


def small_weight():
    sc = small_scene()
    return _cached("lam_small", lambda: lfm.visible_weight(frame_of(sc), small_mesh(), ref_beta(sc.J), orc.default_opt()))
