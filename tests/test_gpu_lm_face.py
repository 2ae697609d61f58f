"""The triangle-area face term of the LM path (``slm_enable_face``, include/super_lm.h) on the GPU, through the C ABI and the
Python surface, against the float64 model of tests/lm_face_model.py.  Needs an MI355X (-m gpu).

Tolerances are the project's own for these quantities (tests/test_gpu_parity.py, tests/test_gpu_lm_corr.py): JtJ 1e-7 of its
largest entry, jtl 1e-8, loss 1e-8 relative (the term alone, in float64 throughout: 1e-9), ``slm_solve`` 1e-9 of the largest
component against the model's system with the Rot products in float32, traces 1e-6 relative on the loss with EVERY accept
flag compared (tests/test_lm_face_model.py asserts that no decision of these traces is a rounding-level tie), final beta
1e-4.  Runs that assemble the same system in another summation order agree to 1e-11 on the step; a batch of eight against
single frames to 1e-7 on beta.  Scenes, meshes and weights come from tests/test_lm_face_model.py, where the weight rule is
asserted: the face term is lost beside the data term at weight 1 (areas 2e-2 m^2 on these 0.2 m grids), so lambda is computed from the model such that the largest
face entry of J^T J is within 10x of the largest data entry."""
import ctypes as C

import numpy as np
import pytest

import lm_face_model as lfm
import test_lm_face_model as cases
from helpers import ref_opt, torch_frame
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

TOL_BETA = 1e-4
INVALID, UNBOUND, UNSUPPORTED = 1, 4, 5
BAD_MESH = (b"slm_bind_frame: a triangle of the slot's face mesh (slm_set_face_mesh) has a node id outside [0, J) or repeats "
            b"an id")


def _rot32(A, b, beta, opt):
    """adds the Rot products rounded to float32 as the reference (and the library) forms them"""
    t = orc.rot_term(beta, opt.mesh_rot_weight, grad=True)
    jv, r = t.Jq.astype(np.float32), t.r.astype(np.float32)
    jtj = (jv[:, :, None] * jv[:, None, :]).astype(np.float64)
    jtr = (jv * r[:, None]).astype(np.float64)
    base = 7 * np.arange(len(jv))
    for c in range(4):
        b[base + c] -= jtr[:, c]
        for d in range(4):
            A[base + c, base + d] += jtj[:, c, d]
    return A, b


def _system_rot32(fr, beta, mesh, lam):
    A, b, _ = lfm.normal_equations_with_face(fr, beta, orc.default_opt(mesh_rot=False), mesh, lam)
    return _rot32(A, b, beta, orc.default_opt())


class Run:
    """an Engine with the term enabled (``lam`` None: never enabled); meshes and frames are bound by the test"""

    def __init__(self, lam, state_f64=True, slots=1, corr=None, seg_mode=0, **kw):
        import torch
        from super_amd import _lib
        from super_amd.engine import Engine
        self.torch, self._lib = torch, _lib
        self.dev = torch.device("cuda", 0)
        self.e = Engine(self.dev, max_frames=slots, **kw)
        self.lib, self.h = self.e.lib, self.e.h
        if lam is not None:
            _lib.check(self.lib.slm_enable_face(self.h, lam), "slm_enable_face")
        if corr is not None:
            _lib.check(self.lib.slm_enable_corr(self.h, corr[0], corr[1]), "slm_enable_corr")
        if seg_mode:
            _lib.check(self.lib.slm_enable_data_weights(self.h, seg_mode, 0.0), "slm_enable_data_weights")
        self.state_f64 = state_f64
        self.keep = []

    def t(self, a, dt):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dt)

    def mesh_args(self, slot, mesh):
        if mesh is None:
            return (self.h, slot, 0, None, None, self.e.stream)
        tri, areas = self.t(mesh[0], self.torch.int32), self.t(mesh[1], self.torch.float64)
        self.keep += [tri, areas]
        return (self.h, slot, int(tri.shape[1]), tri.data_ptr(), areas.data_ptr(), self.e.stream)

    def set_mesh(self, slot, mesh):
        self._lib.check(self.lib.slm_set_face_mesh(*self.mesh_args(slot, mesh)), "slm_set_face_mesh")
        self.torch.cuda.synchronize()
        self.keep.clear()                  # the library copied the mesh: the caller's tensors may go

    def frame(self, sc):
        from super_amd.engine import DeviceFrame
        return DeviceFrame.from_scene(sc, self.dev, state_f64=self.state_f64)

    def bind(self, slot, sc, mesh="keep"):
        if mesh != "keep":
            self.set_mesh(slot, mesh)
        self.e.bind(slot, self.frame(sc))

    def bind_points(self, targets, slot=0):
        o, n, valid = targets
        o, n, valid = self.t(o, self.torch.float64), self.t(n, self.torch.float64), self.t(valid, self.torch.uint8)
        self._lib.check(self.lib.slm_bind_corr_points(self.h, slot, o.data_ptr(), n.data_ptr(), valid.data_ptr(), self.e.stream),
                        "slm_bind_corr_points")

    def bind_sem(self, sem, slot=0):
        seg, sc, tc = self.t(sem.sf_seg, self.torch.int32), self.t(sem.sf_seg_conf, self.torch.float32), self.t(sem.tgt_seg_conf, self.torch.float32)
        self.sem_keep = (seg, sc, tc)      # read in place while the slot is used
        self._lib.check(self.lib.slm_bind_data_semantic(self.h, slot, sc.shape[1], seg.data_ptr(), sc.data_ptr(), tc.data_ptr(),
                                                        self.e.stream), "slm_bind_data_semantic")

    def set_beta(self, beta, slot=0):
        b = self.t(beta, self.torch.float64)
        self._lib.check(self.lib.slm_set_beta(self.h, slot, b.data_ptr(), self.e.stream), "slm_set_beta")
        self.torch.cuda.synchronize()

    def face_loss(self, slot=0):
        out = self.torch.empty(2, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_face_loss(self.h, slot, out.data_ptr(), self.e.stream), "slm_face_loss")
        o = out.cpu().numpy()
        return float(o[0]), int(o[1])

    def loss(self, slot=0):
        out = self.torch.empty(4, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_loss(self.h, slot, out.data_ptr(), self.e.stream), "slm_loss")
        return out.cpu().numpy()

    def assemble(self, slot=0):
        P = 7 * self.e._frames[slot].J
        A = self.torch.empty((P, P), dtype=self.torch.float64, device=self.dev)
        b = self.torch.empty(P, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_assemble(self.h, slot, A.data_ptr(), b.data_ptr(), self.e.stream), "slm_assemble")
        return A.cpu().numpy(), b.cpu().numpy()

    def solve(self, u, slot=0):
        P = 7 * self.e._frames[slot].J
        d = self.torch.zeros(P, dtype=self.torch.float64, device=self.dev)
        st = self.torch.zeros(1, dtype=self.torch.int32, device=self.dev)
        self._lib.check(self.lib.slm_solve(self.h, slot, u, d.data_ptr(), st.data_ptr(), self.e.stream), "slm_solve")
        assert int(st.item()) == 0
        return d.cpu().numpy()

    def run(self, n=1):
        self.e.run(n)
        return [(self.e.beta(i).cpu().numpy(), self.e.records(i)) for i in range(n)]

    def pairs(self, slot=0):
        return int(self.e.plan_info(slot)["pairs"])

    def close(self):
        self.e.close()


def _check_system(r, fr, beta, mesh, lam, us=(10.0, 10.0 / 7.5 ** 5), slot=0):
    """slm_assemble, slm_face_loss, slm_loss and slm_solve of a bound slot at beta against the model"""
    r.set_beta(beta, slot)
    A, b = r.assemble(slot)
    loss, n = r.face_loss(slot)
    parts = r.loss(slot)
    opt = orc.default_opt()
    A_ref, b_ref, M = lfm.normal_equations_with_face(fr, beta, opt, mesh, lam)
    want_loss, want_n = lfm.face_loss(fr, mesh, beta, lam)
    print("face loss", loss, "model", want_loss, "triangles", n, "largest JtJ entry", np.abs(A_ref).max(),
          "largest differences: JtJ", np.abs(A - A_ref).max(), "jtl", np.abs(b - b_ref).max())
    assert n == want_n
    np.testing.assert_allclose(loss, want_loss, rtol=1e-9, atol=0)
    np.testing.assert_allclose(parts[:3].sum() + loss, lfm.total_loss_with_face(fr, beta, opt, mesh, lam)[0], rtol=1e-8)
    assert int(parts[3]) == M                                        # the counts stay the ICP term's
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    A32, b32 = _system_rot32(fr, beta, mesh, lam)
    for u in us:
        ref = orc.solve_damped(A32, b32, u)
        got = r.solve(u, slot)
        print("u", u, "largest step component", np.abs(ref).max(), "largest difference", np.abs(got - ref).max())
        np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9 * max(1.0, np.abs(ref).max()))
    return A_ref


def _check_trace(recs, beta, trace, want_beta):
    assert all(x["status"] == 0 for x in recs)
    loss = np.array([x["loss"] for x in recs])
    want = np.array([t["loss"] for t in trace])
    print("loss", loss, "\nwant", want, "\naccepted", [x["accepted"] for x in recs])
    np.testing.assert_allclose(loss, want, rtol=1e-6, atol=1e-12)
    assert [x["accepted"] for x in recs] == [t["accepted"] for t in trace]          # every flag: none is a tie (CPU test)
    np.testing.assert_allclose([x["u"] for x in recs], [t["u"] for t in trace], rtol=1e-12)
    assert [x["M_loss"] for x in recs] == [t["M_loss"] for t in trace]              # M_grad / M_loss stay the ICP counts
    assert [x["M_grad"] for x in recs] == [t["M_grad"] for t in trace]
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=TOL_BETA)


# ---- 1. assemble / loss / solve at a random small beta -----------------------------------------------------------------
@pytest.mark.parametrize("solver_path", [2, 3])
@pytest.mark.parametrize("state_f64", [0, 1])
@pytest.mark.parametrize("K", [4, 6])
def test_assemble_loss_and_solve_match_the_model(K, state_f64, solver_path):
    sc = cases.scene_k(K)
    fr, mesh, lam, beta = cases.frame_of(sc), lfm.scene_mesh(sc), cases.weight_of(K), cases.ref_beta(sc.J)
    r = Run(lam, bool(state_f64), solver_path=solver_path)
    r.bind(0, sc, mesh)
    A_ref = _check_system(r, fr, beta, mesh, lam)
    r.close()
    A0 = orc.normal_equations(fr, beta, orc.default_opt())[0]
    data_max = np.abs(orc.normal_equations(fr, beta, orc.default_opt(mesh_arap=False, mesh_rot=False))[0]).max()
    assert np.abs(A_ref - A0).max() > 0.1 * data_max                 # the term is as visible a part of the system as the data term


# ---- 2. coupling that only the mesh supplies ---------------------------------------------------------------------------
@pytest.mark.parametrize("solver_path", [0, 3])
def test_coupling_that_only_the_mesh_supplies(solver_path):
    """num_neighbors 1 and one node neighbour (N = 37, J = 12): no triangle cross pair is a surfel or a node pair.  The mesh
    holds a node no surfel references, a node in six triangles, nodes in none and one collinear triangle."""
    sc, mesh, lam = cases.small_scene(), cases.small_mesh(), cases.small_weight()
    fr, beta = cases.frame_of(sc), cases.ref_beta(sc.J)
    r = Run(lam, solver_path=solver_path)
    r.bind(0, sc)                                                    # no mesh yet
    without = r.pairs()
    assert r.face_loss() == (0.0, 0)
    r.bind(0, sc, mesh)
    with_mesh = r.pairs()
    print("coupled pairs", without, "->", with_mesh)
    assert without == len(cases.pair_keys(sc)) and with_mesh == len(cases.pair_keys(sc, mesh)) > without
    _check_system(r, fr, beta, mesh, lam, us=(10.0, 0.37))
    got_beta, recs = r.run()[0]                                      # (the run continues from the random beta: finite, no failure)
    assert all(x["status"] == 0 for x in recs) and np.isfinite(got_beta).all()
    r.close()


# ---- 3. mesh change under a cached plan --------------------------------------------------------------------------------
def test_a_changed_mesh_never_meets_a_stale_plan():
    sc, A, B, lam = cases.small_scene(), cases.small_mesh(), cases.small_mesh(True), cases.small_weight()
    fr, beta = cases.frame_of(sc), cases.ref_beta(sc.J)
    r = Run(lam)
    r.bind(0, sc, A)
    pairs_a = r.pairs()
    _check_system(r, fr, beta, A, lam, us=(0.37,))
    r.bind(0, sc, B)                                                 # the same frame: same surfel pairs, same node graph
    assert r.pairs() == pairs_a + 2 == len(cases.pair_keys(sc, B))
    _check_system(r, fr, beta, B, lam, us=(0.37,))
    sys_a, sys_b = _system_rot32(fr, beta, A, lam), _system_rot32(fr, beta, B, lam)
    assert np.abs(orc.solve_damped(*sys_a, 0.37) - orc.solve_damped(*sys_b, 0.37)).max() > 1e-6
    r.bind(0, sc, A)                                                 # back: the plan covers more pairs than the frame has
    assert r.pairs() == pairs_a
    _check_system(r, fr, beta, A, lam, us=(0.37,))
    r.bind(0, sc)                                                    # the mesh stays with the slot over a later bind
    assert r.face_loss()[1] == A[0].shape[1]
    r.close()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------
def _refused(lib, name, args, code, text):
    rc = getattr(lib, name)(*args)
    got = lib.slm_last_error()
    print(name, rc, got)
    assert rc == code, (name, rc, got)
    assert got == text, (name, got)


def test_refusals():
    import torch
    from super_amd.engine import Engine
    sc, mesh, lam = cases.small_scene(), cases.small_mesh(), cases.small_weight()
    pre = b"slm_enable_face: "
    r = Run(None)
    lib, h = r.lib, r.h
    out = torch.zeros(2, dtype=torch.float64, device=r.dev)
    _refused(lib, "slm_enable_face", (None, 1.0), INVALID, pre + b"null argument")
    for w in (float("nan"), float("inf")):
        _refused(lib, "slm_enable_face", (h, w), INVALID, pre + b"weight must be finite")
    for kw, text in ((dict(data_path=1), b"needs the pair-record data path (data_path 0 or 2)"),
                     (dict(solver_path=1), b"needs a nested-dissection solver_path (0, 2, 3 or 4)"),
                     (dict(use_data=False), b"needs the data term (use_data 1)")):
        e = Engine(r.dev, **kw)
        _refused(lib, "slm_enable_face", (e.h, 1.0), UNSUPPORTED, pre + text)
        e.close()
    e = Engine(r.dev)
    assert lib.slm_set_shard(e.h, 0, 1) == 0
    _refused(lib, "slm_enable_face", (e.h, 1.0), UNSUPPORTED,
             pre + b"the solver is sharded (slm_set_shard); the term's mesh is not sharded")
    e.close()
    # before slm_enable_face, and after a weight of 0 switched it off again
    assert lib.slm_enable_face(h, 2.0) == 0 and lib.slm_enable_face(h, 0.0) == 0
    _refused(lib, "slm_set_face_mesh", r.mesh_args(0, mesh), UNSUPPORTED, b"slm_set_face_mesh: slm_enable_face first")
    _refused(lib, "slm_face_loss", (h, 0, out.data_ptr(), None), UNSUPPORTED, b"slm_face_loss: slm_enable_face first")
    e = Engine(r.dev)                                                # the options combine
    assert lib.slm_enable_face(e.h, lam) == 0 and lib.slm_enable_corr(e.h, 2, 0.5) == 0 and lib.slm_enable_data_weights(e.h, 0, 2e-5) == 0
    e.close()
    assert lib.slm_enable_face(h, lam) == 0, lib.slm_last_error()
    _refused(lib, "slm_set_shard", (h, 0, 1), UNSUPPORTED,
             b"slm_set_shard: the face term is enabled (slm_enable_face); its mesh is not sharded")
    args = r.mesh_args(0, mesh)
    _refused(lib, "slm_set_face_mesh", (None,) + args[1:], INVALID, b"slm_set_face_mesh: null argument")
    _refused(lib, "slm_set_face_mesh", args[:3] + (None, args[4], None), INVALID, b"slm_set_face_mesh: null argument")
    _refused(lib, "slm_set_face_mesh", args[:4] + (None, None), INVALID, b"slm_set_face_mesh: null argument")
    _refused(lib, "slm_set_face_mesh", (h, 1) + args[2:], INVALID, b"slm_set_face_mesh: bad slot")
    _refused(lib, "slm_set_face_mesh", (h, -1) + args[2:], INVALID, b"slm_set_face_mesh: bad slot")
    _refused(lib, "slm_set_face_mesh", (h, 0, -1) + args[3:], INVALID, b"slm_set_face_mesh: n_triangles must be >= 0")
    _refused(lib, "slm_face_loss", (None, 0, out.data_ptr(), None), INVALID, b"slm_face_loss: null argument")
    _refused(lib, "slm_face_loss", (h, 0, None, None), INVALID, b"slm_face_loss: null argument")
    _refused(lib, "slm_face_loss", (h, 3, out.data_ptr(), None), INVALID, b"slm_face_loss: bad slot")
    _refused(lib, "slm_face_loss", (h, 0, out.data_ptr(), None), UNBOUND, b"slm_face_loss: slm_bind_frame first")
    fr = r.frame(sc)
    cs = fr.c_struct()
    cs.J = 65536
    _refused(lib, "slm_bind_frame", (h, 0, C.byref(cs), None), UNSUPPORTED,
             b"slm_bind_frame: the face term (slm_enable_face) needs J < 65536")
    # the two bad meshes: an id = J, a repeated id; by a bind and by a model prepared ahead; the slot is left unbound
    r.bind(0, sc, mesh)
    for bad in ((0, 0, sc.J), (1, 2, int(mesh[0][0, 2]))):          # (vertex, triangle, id): id = J; vertex 1 repeats vertex 0
        tri = mesh[0].copy()
        tri[bad[0], bad[1]] = bad[2]
        r.set_mesh(0, (tri, mesh[1]))
        cs = fr.c_struct()
        _refused(lib, "slm_bind_frame", (h, 0, C.byref(cs), r.e.stream), INVALID, BAD_MESH)
        assert lib.slm_run(h, 1, r.e.stream) == UNBOUND
        assert lib.slm_prepare_model(h, 0, C.byref(cs), r.e.stream) == 0
        _refused(lib, "slm_bind_frame", (h, 0, C.byref(cs), r.e.stream), INVALID, BAD_MESH)
        assert lib.slm_face_loss(h, 0, out.data_ptr(), r.e.stream) == UNBOUND
    r.bind(0, sc, mesh)                                              # a good mesh binds again
    assert r.face_loss()[1] == mesh[0].shape[1]
    for w in (1.0, 0.0):
        _refused(lib, "slm_enable_face", (h, w), INVALID, pre + b"a slot is already bound; call it after slm_create and before the first bind")
    r.close()


def test_an_empty_mesh_gives_the_system_of_an_enabled_solver_without_one():
    sc = cases.scene_k(4)
    mesh, lam, beta = lfm.scene_mesh(sc), cases.weight_of(4), cases.ref_beta(sc.J)
    steps = {}
    for kind in ("cleared", "never set", "never enabled"):
        r = Run(None if kind == "never enabled" else lam)
        if kind == "cleared":
            r.bind(0, sc, mesh)
            assert r.face_loss()[1] == mesh[0].shape[1]
            r.bind(0, sc, None)                                      # n_triangles = 0 clears it
        else:
            r.bind(0, sc)
        if kind != "never enabled":
            assert r.face_loss() == (0.0, 0)
        r.set_beta(beta)
        steps[kind] = r.solve(0.37)
        r.close()
    np.testing.assert_allclose(steps["cleared"], steps["never set"], rtol=0, atol=1e-11)
    np.testing.assert_allclose(steps["cleared"], steps["never enabled"], rtol=0, atol=1e-11)    # (tuple-sorted form there)


# ---- 5. ten iterations on a single slot --------------------------------------------------------------------------------
@pytest.mark.parametrize("K,kind,factor,u,v", cases.TRACE_CASES)
def test_ten_iterations_match_the_models_loop(K, kind, factor, u, v):
    sc = cases.scene_k(K)
    want_beta, trace = cases.trace_of(K, kind, factor, u, v)
    r = Run(factor * cases.weight_of(K, kind), u0=u, v=v)
    r.bind(0, sc, cases.mesh_of(K, kind))
    (got_beta, recs), = r.run()
    r.close()
    _check_trace(recs, got_beta, trace, want_beta)


# ---- 6. eight slots ----------------------------------------------------------------------------------------------------
def test_batch_of_eight_slots_with_unlike_meshes_and_one_without():
    sc, lam = cases.scene_k(cases.BATCH_K), cases.batch_weight()
    u, v = cases.DAMPING
    kinds = cases.BATCH_KINDS                                        # (tie-free in the model at this weight: CPU test)
    mesh = lambda kind: None if kind is None else cases.mesh_of(cases.BATCH_K, kind)
    single = {}
    for kind in set(kinds):
        r = Run(lam, u0=u, v=v)
        r.bind(0, sc, mesh(kind))
        single[kind] = r.run()[0]
        r.close()
    r = Run(None, u0=u, v=v)                                         # a solver on which the term was never enabled
    r.bind(0, sc)
    never = r.run()[0]
    r.close()
    r = Run(lam, slots=8, u0=u, v=v)
    for i, kind in enumerate(kinds):
        r.set_mesh(i, mesh(kind))
    r.e.bind_batch([r.frame(sc) for _ in kinds])                     # slm_bind_frames: each slot's own mesh
    out = r.run(8)
    tris = [r.face_loss(i)[1] for i in range(8)]
    r.close()
    for i, kind in enumerate(kinds):
        beta, recs = out[i]
        print(i, kind, "largest difference to the single-slot run", np.abs(beta - single[kind][0]).max())
        np.testing.assert_allclose(beta, single[kind][0], rtol=0, atol=1e-7)
        np.testing.assert_allclose([x["loss"] for x in recs], [x["loss"] for x in single[kind][1]], rtol=1e-9)
        assert tris[i] == (0 if kind is None else mesh(kind)[0].shape[1])
        if kind is None:
            np.testing.assert_allclose(beta, never[0], rtol=0, atol=1e-7)
        else:
            assert np.abs(beta - never[0]).max() > 1e-6
    for kind in set(kinds):                                          # and the single-slot runs are the model's
        want_beta, trace = cases.batch_trace_of(kind)
        _check_trace(single[kind][1], single[kind][0], trace, want_beta)


def test_combined_with_the_correspondence_term_and_with_hard_semantic_weights():
    import lm_corr_model as lcm
    import lm_weight_model as lwm
    from super_amd import synth
    sc = cases.scene_k(4)
    fr, mesh, lam, opt = cases.frame_of(sc), cases.mesh_of(4, "full"), cases.weight_of(4), orc.default_opt()
    u, v = cases.DAMPING
    tg = lcm.targets_from_flow(fr, synth.smooth_flow(sc.H, sc.W, 24, amp=(2.0, 1.5)))
    trace = []
    want = lfm.lm_with_face(fr, opt, mesh, lam, u=u, v=v, trace=trace, base=lfm.base_corr(fr, opt, tg, 2, 0.5))
    r = Run(lam, corr=(2, 0.5), u0=u, v=v)
    r.bind(0, sc, mesh)
    r.bind_points(tg)
    (beta, recs), = r.run()
    r.close()
    _check_trace(recs, beta, trace, want)
    sem, trace = lwm.sem_of(sc), []
    want = lfm.lm_with_face(fr, opt, mesh, lam, u=u, v=v, trace=trace, base=lfm.base_weighted(fr, opt, sem, 1))
    r = Run(lam, seg_mode=1, u0=u, v=v)
    r.bind(0, sc, mesh)
    r.bind_sem(sem)
    (beta, recs), = r.run()
    r.close()
    _check_trace(recs, beta, trace, want)


# ---- 7. a model prepared ahead -----------------------------------------------------------------------------------------
def test_prepare_model_then_bind_equals_a_plain_bind():
    sc = cases.scene_k(6)
    mesh, lam = cases.mesh_of(6, "full"), 3.0 * cases.weight_of(6)
    u, v = cases.DAMPING
    outs = []
    for prepared in (False, True):
        r = Run(lam, u0=u, v=v)
        r.set_mesh(0, mesh)
        fr = r.frame(sc)
        if prepared:
            cs = fr.c_struct()
            r._lib.check(r.lib.slm_prepare_model(r.h, 0, C.byref(cs), r.e.stream), "slm_prepare_model")
        r.e.bind(0, fr)
        assert r.face_loss()[1] == mesh[0].shape[1]
        r.set_beta(cases.ref_beta(sc.J))
        step = r.solve(0.37)
        if prepared:
            cs = fr.c_struct()
            r._lib.check(r.lib.slm_prepare_model(r.h, 0, C.byref(cs), r.e.stream), "slm_prepare_model")
        r.e.bind(0, fr)
        outs.append((step, r.run()[0]))
        r.close()
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-11)
    np.testing.assert_allclose(outs[0][1][1][0]["loss"], outs[1][1][1][0]["loss"], rtol=1e-11)
    np.testing.assert_allclose([x["loss"] for x in outs[0][1][1]], [x["loss"] for x in outs[1][1][1]], rtol=1e-9)
    np.testing.assert_allclose(outs[0][1][0], outs[1][1][0], rtol=0, atol=1e-9)


# ---- 8. Python surface --------------------------------------------------------------------------------------------------
def _with_mesh(sc, mesh, device="cuda"):
    import torch
    sf, inputs, new_data = torch_frame(sc, device)
    sf.ED_nodes.triangles = torch.from_numpy(np.ascontiguousarray(mesh[0])).to(device)
    sf.ED_nodes.triangles_areas = torch.from_numpy(np.ascontiguousarray(mesh[1])).to(device)
    return sf, inputs, new_data


def test_python_surface():
    from super_amd.LM import LM_Solver
    K, kind, factor, u, v = cases.TRACE_CASES[3]                    # every third triangle, areas 10 % smaller
    sc, mesh = cases.scene_k(K), cases.mesh_of(K, kind)
    want_beta, trace = cases.trace_of(K, kind, factor, u, v)
    opt = ref_opt(orc.default_opt())
    with pytest.raises(ValueError):
        LM_Solver(opt, face_term=True)                               # needs opt.mesh_face
    opt.mesh_face, opt.mesh_face_weight = True, factor * cases.weight_of(K, kind)
    with pytest.raises(NotImplementedError):
        LM_Solver(opt, face_term=True, rank=0, world=1)
    lm = LM_Solver(opt, face_term=True)
    sf, inputs, new_data = _with_mesh(sc, mesh)
    beta = lm.LM(sf, inputs, new_data, u=u, v=v).cpu().numpy()
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=TOL_BETA)
    np.testing.assert_allclose([x["loss"] for x in lm.last_records[0]], [t["loss"] for t in trace], rtol=1e-6)
    assert lm.last_face_loss[0][1] == mesh[0].shape[1]
    np.testing.assert_allclose(lm.last_face_loss[0][0], lfm.face_loss(cases.frame_of(sc), mesh, beta, opt.mesh_face_weight)[0], rtol=1e-8)
    # the same tensors again, and a model prepared ahead: the mesh is kept, the result the same
    again = lm.LM(sf, inputs, new_data, u=u, v=v).cpu().numpy()
    np.testing.assert_allclose(again, beta, rtol=0, atol=1e-9)
    lm.prepare_model(sf, u=u, v=v)
    ahead = lm.LM(sf, inputs, new_data, u=u, v=v).cpu().numpy()
    np.testing.assert_allclose(ahead, beta, rtol=0, atol=1e-9)
    # a changed tensor is sent again: other areas in a new tensor, then an in-place write
    other = (mesh[0], 1.2 * mesh[1])
    fresh = LM_Solver(opt, face_term=True)
    want_other = fresh.LM(*_with_mesh(sc, other), u=u, v=v).cpu().numpy()
    assert np.abs(want_other - beta).max() > 1e-6
    sf.ED_nodes.triangles_areas = sf.ED_nodes.triangles_areas * 1.2
    np.testing.assert_allclose(lm.LM(sf, inputs, new_data, u=u, v=v).cpu().numpy(), want_other, rtol=0, atol=1e-9)
    sf.ED_nodes.triangles_areas.div_(1.2)
    np.testing.assert_allclose(lm.LM(sf, inputs, new_data, u=u, v=v).cpu().numpy(), beta, rtol=0, atol=1e-9)
    # without the flag opt.mesh_face is ignored exactly as today
    plain_opt = ref_opt(orc.default_opt())
    plain = LM_Solver(plain_opt).LM(*torch_frame(sc), u=u, v=v).cpu().numpy()
    ignored = LM_Solver(opt).LM(sf, inputs, new_data, u=u, v=v).cpu().numpy()
    np.testing.assert_allclose(ignored, plain, rtol=0, atol=1e-12)
    assert np.abs(beta - plain).max() > 1e-6
