"""The LM entry points of the C ABI -- ``slm_assemble``, ``slm_loss``, ``slm_solve`` -- at every ``num_neighbors`` (K = 1 .. 8)
against the float64 NumPy oracle (``oracle.lm_oracle``), and the binds' refusal of KNN tables the reference can never
produce.

* K != 4 runs the K-generic pair path on the nested-dissection (multifrontal) solver.  ``slm_solve`` there assembles the
  data term through the pair records (``k_data_grad_pairs<K>`` + ``k_pair_scatter``), as ``slm_run`` does; ``slm_assemble``
  goes through the block-banded kernels (``k_data_grad<K>``) instead, so it is never the reference of ``slm_solve``: every
  check below compares with the oracle's own JtJ / jtl.
* Shape edges: J just above K (K = 8 with J = 10 and 12: every surfel couples almost every node, the plan has one or very
  few fronts) and J = 300 at K = 3 and 6 (several levels of the tree).
* The reference takes its KNN ids from a top-k: K distinct ids in [0, J) per surfel, and a top-k of K among J < K nodes
  raises.  ``slm_bind_frame`` and ``slm_gf_bind_frame`` refuse any other table (SLM_ERR_INVALID) before a kernel indexes
  with it, on every data path, and the context works on afterwards.

Needs an MI355X (-m gpu)."""
import numpy as np
import pytest

from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

_CACHE = {}

# name -> (K, make_scene arguments); every scene has J > n_ed_neighbors (4) and J >= K, as the oracle needs
SCENES = {f"k{K}": (K, dict(N=2500, J=60, H=60, W=80, seed=40 + K, src_border=5, tgt_border=3)) for K in range(1, 9)}
SCENES.update({
    "k8_j10": (8, dict(N=1500, J=10, H=60, W=80, seed=77, src_border=5, tgt_border=3)),
    "k8_j12": (8, dict(N=1500, J=12, H=60, W=80, seed=78, src_border=5, tgt_border=3)),
    "k3_j300": (3, dict(N=12000, J=300, H=240, W=320, seed=93, src_border=8, tgt_border=4)),
    "k6_j300": (6, dict(N=12000, J=300, H=240, W=320, seed=96, src_border=8, tgt_border=4)),
})
DAMPINGS = (10.0, 10.0 / 7.5 ** 5)   # the first iteration's damping and a late one (4e-4)


def _perturbed_beta(J, seed):
    import torch
    rng = np.random.default_rng(seed)
    beta = np.tile([1.0, 0, 0, 0, 0, 0, 0], (J, 1)) + np.concatenate(
        [rng.normal(0, 0.01, (J, 4)), rng.normal(0, 0.002, (J, 3))], axis=1)
    return torch.from_numpy(beta).cuda()


def _scene(name):
    key = ("scene", name)
    if key not in _CACHE:
        from super_amd import synth
        K, kw = SCENES[name]
        sc = synth.make_scene(n_neighbors=K, **kw)
        assert sc.sf_knn_idx.shape[1] == K and sc.J > sc.ed_knn_idx.shape[1] and sc.J >= K
        _CACHE[key] = sc
    return _CACHE[key]


def _beta(name):
    return _perturbed_beta(_scene(name).J, 17)


def _oracle_system(name):
    """JtJ (dense), jtl and the matched count of the oracle at the perturbed beta."""
    key = ("system", name)
    if key not in _CACHE:
        _CACHE[key] = orc.normal_equations(orc.Frame.from_scene(_scene(name)), _beta(name).cpu().numpy(), orc.default_opt())
    return _CACHE[key]


def _oracle_system_rot32(name):
    """The same system with the Rot term's products J^T J and J^T r rounded to float32 as the reference forms them (its
    Rot Jacobian and residual are float32 tensors; the oracle's normal_equations multiplies them in float64).  The data
    and ARAP parts are the oracle's float64 ones.  What the solve is held to at 1e-9: the float32 rounding of the Rot
    products alone moves delta by ~1e-8 relative."""
    key = ("system_rot32", name)
    if key not in _CACHE:
        opt = orc.default_opt()
        bt = _beta(name).cpu().numpy()
        A, b, M = orc.normal_equations(orc.Frame.from_scene(_scene(name)), bt, orc.default_opt(mesh_rot=False))
        t = orc.rot_term(bt, opt.mesh_rot_weight, grad=True)
        jv, r = t.Jq.astype(np.float32), t.r.astype(np.float32)        # (exact: float32 values held in float64)
        jtj = (jv[:, :, None] * jv[:, None, :]).astype(np.float64)      # (J,4,4) float32 products
        jtr = (jv * r[:, None]).astype(np.float64)
        base = 7 * np.arange(len(jv))
        for c in range(4):
            b[base + c] -= jtr[:, c]
            for d in range(4):
                A[base + c, base + d] += jtj[:, c, d]
        _CACHE[key] = (A, b, M)
    return _CACHE[key]


def _engine(name, **kw):
    """A one-slot solver with the scene bound and its beta set to the perturbed one."""
    import torch
    from super_amd import _lib
    from super_amd.engine import DeviceFrame, Engine
    dev = torch.device("cuda", 0)
    e = Engine(dev, **kw)
    e.bind(0, DeviceFrame.from_scene(_scene(name), dev))
    bt = _beta(name)
    _lib.check(e.lib.slm_set_beta(e.h, 0, bt.data_ptr(), e.stream), "slm_set_beta")
    return e


@pytest.mark.parametrize("name", list(SCENES))
def test_assemble_matches_the_oracle(name):
    import torch
    from super_amd import _lib
    sc = _scene(name)
    P = 7 * sc.J
    A_ref, b_ref, _ = _oracle_system(name)
    e = _engine(name)
    A = torch.empty((P, P), dtype=torch.float64, device="cuda")
    b = torch.empty(P, dtype=torch.float64, device="cuda")
    _lib.check(e.lib.slm_assemble(e.h, 0, A.data_ptr(), b.data_ptr(), e.stream), "slm_assemble")
    A, b = A.cpu().numpy(), b.cpu().numpy()
    e.close()
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))


@pytest.mark.parametrize("name", list(SCENES))
def test_loss_terms_match_the_oracle(name):
    import torch
    from super_amd import _lib
    sc = _scene(name)
    opt = orc.default_opt()
    fr, bt = orc.Frame.from_scene(sc), _beta(name).cpu().numpy()
    d = orc.data_term(fr, bt, opt.sf_point_plane_weight)
    want = [float((d.r ** 2).sum()), float((orc.arap_term(fr, bt, opt.mesh_arap_weight).r ** 2).sum()),
            float((orc.rot_term(bt, opt.mesh_rot_weight).r ** 2).sum())]
    total, M = orc.total_loss(fr, bt, opt)
    assert M == len(d.r) > 0
    e = _engine(name)
    out = torch.empty(4, dtype=torch.float64, device="cuda")
    _lib.check(e.lib.slm_loss(e.h, 0, out.data_ptr(), e.stream), "slm_loss")
    got = out.cpu().numpy()
    e.close()
    np.testing.assert_allclose(got[0], want[0], rtol=1e-9)        # data
    np.testing.assert_allclose(got[1], want[1], rtol=1e-9)        # ARAP
    np.testing.assert_allclose(got[2], want[2], rtol=1e-6)        # Rot: float32 residuals and squares, like the reference
    assert int(got[3]) == M
    np.testing.assert_allclose(got[:3].sum(), total, rtol=1e-8)


def _expected_form(e, solver_path):
    """slm_debug_last_solver_form of a one-frame slm_solve (enqueue_front_solve): the task graph (1) for solver_path 2 and
    for 0 (one frame is always few enough), the per-level launches (0) for 3; for 4 the hybrid (2) when the tree has a
    level below the cut -- the top levels of at most 4 fronts run as tasks, and at least the deepest level stays with the
    launches -- and otherwise (a one-level tree) the per-level launches."""
    if solver_path in (0, 2):
        return 1
    if solver_path == 3:
        return 0
    return 2 if e.plan_info(0)["levels"] >= 2 else 0


@pytest.mark.parametrize("name", list(SCENES))
def test_solve_on_every_solver_path_matches_the_oracle(name):
    """(A + uI) delta = b with A, b the oracle's (Rot products in float32, _oracle_system_rot32): the residual of the
    device's delta and its distance to the oracle's Cholesky solution, on every solver path at two dampings.  Paths
    0 / 2 / 3 / 4 must have run a multifrontal form."""
    import torch
    from super_amd import _lib
    sc = _scene(name)
    P = 7 * sc.J
    A, b, _ = _oracle_system_rot32(name)
    bn = float(np.abs(b).max())
    assert bn > 0
    for sp in (2, 3, 4, 0, 1):   # task graph, per-level, hybrid, default, block-banded
        e = _engine(name, solver_path=sp)
        info = e.plan_info(0)
        assert info["solver"] == ("band" if sp == 1 else "nested-dissection multifrontal"), (name, sp)
        for u in DAMPINGS:
            d = torch.zeros(P, dtype=torch.float64, device="cuda")
            s = torch.full((1,), -1, dtype=torch.int32, device="cuda")
            _lib.check(e.lib.slm_solve(e.h, 0, u, d.data_ptr(), s.data_ptr(), e.stream), "slm_solve")
            form = e.lib.slm_debug_last_solver_form(e.h)
            assert form == (-1 if sp == 1 else _expected_form(e, sp)), (name, sp, form, info["levels"])
            assert int(s.item()) == 0, (name, sp, u)
            delta = d.cpu().numpy()
            rel = float(np.abs(A @ delta + u * delta - b).max()) / bn
            x = orc.solve_damped(A, b, u)
            err = float(np.abs(delta - x).max()) / float(np.abs(x).max())
            print(f"[{name} path {sp} u={u:.3g} form {form}] |(A+uI)d - b|_inf / |b|_inf = {rel:.2e}, "
                  f"|d - d_oracle|_inf / |d_oracle|_inf = {err:.2e}")
            assert rel <= 1e-9, (name, sp, u, rel)
            assert err <= 1e-9, (name, sp, u, err)
        e.close()


# ---------------------------------------------------------------------------------- tables the reference never produces
def _bad_tables(sc, defect):
    """(sf_knn_idx, ed_knn_idx) of `sc` with one defect edited in on the host."""
    sf, ed = sc.sf_knn_idx.copy(), sc.ed_knn_idx.copy()
    i = sc.N // 2
    if defect == "sf_repeat":
        sf[i, -1] = sf[i, 0]
    elif defect == "sf_repeat_first_rows":
        sf[: min(64, sc.N), 1] = sf[: min(64, sc.N), 0]
    elif defect == "sf_J":
        sf[i, -1] = sc.J
    elif defect == "sf_neg":
        sf[i, 0] = -1
    elif defect == "ed_J":
        ed[sc.J // 2, -1] = sc.J
    elif defect == "ed_neg":
        ed[sc.J - 1, 0] = -3
    else:
        raise ValueError(defect)
    return sf, ed


DEFECTS = ("sf_repeat", "sf_repeat_first_rows", "sf_J", "sf_neg", "ed_J", "ed_neg")
# (K, Engine arguments): the tuple-sorted preparation (K = 4, binned then hinted), the K-generic pair plan, the
# per-entry atomics path (data_path 1) and a frame without the data term (the block-banded pass over the tables)
LM_BIND_CONFIGS = {"k4": (4, {}), "k6": (6, {}), "k1": (1, {}), "k6_atomics": (6, dict(data_path=1)),
                   "k4_band": (4, dict(solver_path=1)), "k5_no_data": (5, dict(use_data=False))}


def _small_scene(K, seed):
    from super_amd import synth
    return synth.make_scene(N=1500, J=40, H=60, W=80, seed=seed, src_border=5, tgt_border=3, n_neighbors=K)


def _frame_with(sc, sf_knn_idx, ed_knn_idx):
    import torch
    from super_amd.engine import DeviceFrame
    f = DeviceFrame.from_scene(sc, torch.device("cuda", 0))
    f.sf_knn_idx = torch.from_numpy(np.ascontiguousarray(sf_knn_idx)).to("cuda", torch.int32)
    f.ed_knn_idx = torch.from_numpy(np.ascontiguousarray(ed_knn_idx)).to("cuda", torch.int32)
    if f.sf_knn_idx.shape[1] != f.sf_knn_w.shape[1]:   # (J < K: a weight per id, the same table twice over)
        w = f.sf_knn_w.repeat(1, 2) * 0.5
        f.sf_knn_w = w.contiguous()
    return f


@pytest.mark.parametrize("config", list(LM_BIND_CONFIGS))
def test_lm_bind_refuses_tables_the_reference_never_produces(config):
    import ctypes as C
    import torch
    from super_amd import _lib
    from super_amd.engine import DeviceFrame, Engine
    K, kw = LM_BIND_CONFIGS[config]
    sc = _small_scene(K, 60 + K)
    dev = torch.device("cuda", 0)
    n_it = 2
    opt = orc.default_opt(num_optimize_iterations=n_it, sf_point_plane=kw.get("use_data", True))
    want = orc.lm(orc.Frame.from_scene(sc), opt)
    e = Engine(dev, num_iterations=n_it, **kw)
    good = DeviceFrame.from_scene(sc, dev)
    e.bind(0, good)                                        # (the next preparation is a hinted one)
    e.run(1)
    np.testing.assert_allclose(e.beta(0).cpu().numpy(), want, rtol=0, atol=1e-8)
    for defect in DEFECTS:
        if K == 1 and "repeat" in defect:   # (one id per row: nothing to repeat)
            continue
        bad = _frame_with(sc, *_bad_tables(sc, defect))
        torch.cuda.synchronize()
        c = bad.c_struct()
        rc = e.lib.slm_bind_frame(e.h, 0, C.byref(c), e.stream)
        msg = e.lib.slm_last_error()
        assert rc == _lib.SLM_ERR_INVALID and b"knn_idx" in msg, (config, defect, rc, msg)
        assert e.lib.slm_run(e.h, 1, e.stream) == _lib.SLM_ERR_UNBOUND, (config, defect)
        e.bind(0, good)                                    # the context works on: a good frame reproduces the oracle
        e.run(1)
        np.testing.assert_allclose(e.beta(0).cpu().numpy(), want, rtol=0, atol=1e-8, err_msg=f"{config} after {defect}")
        assert all(r["status"] == 0 for r in e.records(0))
    e.close()


def test_lm_bind_refuses_fewer_nodes_than_neighbours():
    """J < K: no table of K distinct ids exists (the reference's top-k raises).  Refused on the host, before any launch."""
    import ctypes as C
    import torch
    from super_amd import _lib, synth
    from super_amd.engine import DeviceFrame, Engine
    sc = synth.make_scene(N=800, J=6, H=60, W=80, seed=5, src_border=5, tgt_border=3, n_neighbors=4)
    dev = torch.device("cuda", 0)
    e = Engine(dev, num_iterations=2)
    bad = _frame_with(sc, np.concatenate([sc.sf_knn_idx, sc.sf_knn_idx], axis=1), sc.ed_knn_idx)   # K = 8 > J = 6
    torch.cuda.synchronize()
    c = bad.c_struct()
    assert c.K == 8 and c.J == 6
    assert e.lib.slm_bind_frame(e.h, 0, C.byref(c), e.stream) == _lib.SLM_ERR_INVALID
    assert b"num_neighbors" in e.lib.slm_last_error()
    assert e.lib.slm_run(e.h, 1, e.stream) == _lib.SLM_ERR_UNBOUND
    e.bind(0, DeviceFrame.from_scene(sc, dev))
    e.run(1)
    want = orc.lm(orc.Frame.from_scene(sc), orc.default_opt(num_optimize_iterations=2))
    np.testing.assert_allclose(e.beta(0).cpu().numpy(), want, rtol=0, atol=1e-8)
    e.close()


@pytest.mark.parametrize("K", [4, 6])
def test_graphfit_bind_refuses_tables_the_reference_never_produces(K):
    """slm_gf_bind_frame: the same refusals (k_gf_data's row pass gives every id of a row an LDS slot of its own and
    indexes the nodes with them); afterwards the context reproduces the oracle's optimiser."""
    import torch
    from helpers import torch_frame
    from oracle import graphfit_oracle as gfo
    from super_amd._lib import SuperLMError
    from super_amd.deform_mesh import GraphFit
    sc = _small_scene(K, 80 + K)
    opt = gfo.default_opt(optimizer="Adam")
    opt.deform_udpate_method = "super_edg"
    want = gfo.graphfit(gfo.Problem(sc), opt)
    gf = GraphFit(opt)
    sf, inputs, new_data = torch_frame(sc)
    np.testing.assert_allclose(gf(inputs, sf, new_data, None).cpu().numpy(), want, rtol=0, atol=1e-9)
    cases = [(d, *_bad_tables(sc, d)) for d in DEFECTS]
    cases.append(("J_lt_K", None, None))
    for defect, bad_sf, bad_ed in cases:
        bsc = sc
        if defect == "J_lt_K":   # 8 ids per row among J = 6 nodes (every id twice over)
            from super_amd import synth
            bsc = synth.make_scene(N=800, J=6, H=60, W=80, seed=7, src_border=5, tgt_border=3, n_neighbors=4)
            bad_sf = np.concatenate([bsc.sf_knn_idx, bsc.sf_knn_idx], axis=1)
            bad_ed = bsc.ed_knn_idx
        bsf, binputs, bnew = torch_frame(bsc)
        bsf.knn_indices = torch.from_numpy(bad_sf).cuda()
        if bad_sf.shape[1] != bsc.sf_knn_w.shape[1]:
            w = np.concatenate([bsc.sf_knn_w, bsc.sf_knn_w], axis=1)
            bsf.knn_w = torch.from_numpy(w / w.sum(1, keepdims=True)).cuda().double()
        bsf.ED_nodes.knn_indices = torch.from_numpy(bad_ed).cuda()
        with pytest.raises(SuperLMError, match=r"slm_gf_bind_frame failed with status 1\b.*(knn_idx|num_neighbors)"):
            gf(binputs, bsf, bnew, None)
        got = gf(inputs, sf, new_data, None).cpu().numpy()
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9, err_msg=f"K={K} after {defect}")
