"""The semantic boundary-morph term of the LM path (``slm_enable_morph``, include/super_lm.h) on the GPU, through the C ABI and
the Python surface, against the float64 model of tests/lm_morph_model.py.  Needs an MI355X (-m gpu).

Tolerances are the project's own for these quantities (tests/test_gpu_lm_face.py): JtJ 1e-7 of its largest entry, jtl 1e-8 x
max(1, largest model entry) (the term's entries are pixel-sized), the term's loss 1e-9 relative, the total loss 1e-8,
``slm_solve`` 1e-9 of the largest component against the model's system with the Rot products in float32, traces 1e-6 relative
on the loss with EVERY accept flag compared, final beta 1e-4.  Runs that assemble the same system in another summation order
agree to 1e-11 on the step; a batch of eight against single frames to 1e-7 on beta.  The selection itself is compared array
for array: kept exactly, the targets exactly (half-integers), l_i to 1e-12.  Scenes, inputs and weights come from
tests/test_lm_morph_model.py, which asserts on the CPU that the model's decisions at every beta visited here are not
rounding-level ties (``check_conditions``, ``decision_margins``) and that the weight rule holds: in pixel units the term
swamps the data term at weight 1, so lambda is computed from the model such that the term's largest J^T J entry is within 10x
of the data term's."""
import ctypes as C
import re

import numpy as np
import pytest

import lm_morph_model as lmm
import test_lm_morph_model as cases
from helpers import ref_opt, torch_frame
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

TOL_BETA = 1e-4
INVALID, UNBOUND, UNSUPPORTED = 1, 4, 5


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


def _system_rot32(fr, beta, sem, lam):
    A, b, _ = lmm.normal_equations_with_morph(fr, beta, orc.default_opt(mesh_rot=False), sem, lam)
    return _rot32(A, b, beta, orc.default_opt())


class Run:
    """an Engine with the term enabled (``lam`` None: never enabled); frames and inputs are bound by the test"""

    def __init__(self, lam, state_f64=True, slots=1, corr=None, seg_mode=0, face=None, **kw):
        import torch
        from super_amd import _lib
        from super_amd.engine import Engine
        self.torch, self._lib = torch, _lib
        self.dev = torch.device("cuda", 0)
        self.e = Engine(self.dev, max_frames=slots, **kw)
        self.lib, self.h = self.e.lib, self.e.h
        if lam is not None:
            _lib.check(self.lib.slm_enable_morph(self.h, lam), "slm_enable_morph")
        if corr is not None:
            _lib.check(self.lib.slm_enable_corr(self.h, corr[0], corr[1]), "slm_enable_corr")
        if seg_mode:
            _lib.check(self.lib.slm_enable_data_weights(self.h, seg_mode, 0.0), "slm_enable_data_weights")
        if face is not None:
            _lib.check(self.lib.slm_enable_face(self.h, face), "slm_enable_face")
        self.state_f64 = state_f64
        self.keep = {}

    def t(self, a, dt):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dt)

    def frame(self, sc):
        from super_amd.engine import DeviceFrame
        return DeviceFrame.from_scene(sc, self.dev, state_f64=self.state_f64)

    def morph_args(self, slot, sem):
        seg, conf, sf = self.t(sem.img_seg, self.torch.int32), self.t(sem.img_seg_conf, self.torch.float32), self.t(sem.sf_seg, self.torch.int32)
        self.keep[slot] = (seg, conf, sf)                          # read in place while the slot is used
        self.counts = (C.c_int32 * 4)()
        return (self.h, slot, sem.C, seg.data_ptr(), conf.data_ptr(), sf.data_ptr(), self.counts, self.e.stream)

    def bind_morph(self, slot, sem):
        self._lib.check(self.lib.slm_bind_morph(*self.morph_args(slot, sem)), "slm_bind_morph")
        return list(self.counts)[:sem.C]

    def bind(self, slot, sc, sem=None):
        self.e.bind(slot, self.frame(sc))
        if sem is not None:
            assert self.bind_morph(slot, sem) == [len(e) for e in sem.edges]

    def set_mesh(self, slot, mesh):
        tri, areas = self.t(mesh[0], self.torch.int32), self.t(mesh[1], self.torch.float64)
        self._lib.check(self.lib.slm_set_face_mesh(self.h, slot, int(tri.shape[1]), tri.data_ptr(), areas.data_ptr(), self.e.stream),
                        "slm_set_face_mesh")
        self.torch.cuda.synchronize()

    def bind_points(self, targets, slot=0):
        o, n, valid = targets
        o, n, valid = self.t(o, self.torch.float64), self.t(n, self.torch.float64), self.t(valid, self.torch.uint8)
        self._lib.check(self.lib.slm_bind_corr_points(self.h, slot, o.data_ptr(), n.data_ptr(), valid.data_ptr(), self.e.stream),
                        "slm_bind_corr_points")

    def bind_sem(self, sem, slot=0):
        seg, sc, tc = self.t(sem.sf_seg, self.torch.int32), self.t(sem.sf_seg_conf, self.torch.float32), self.t(sem.tgt_seg_conf, self.torch.float32)
        self.sem_keep = (seg, sc, tc)
        self._lib.check(self.lib.slm_bind_data_semantic(self.h, slot, sc.shape[1], seg.data_ptr(), sc.data_ptr(), tc.data_ptr(),
                                                        self.e.stream), "slm_bind_data_semantic")

    def set_beta(self, beta, slot=0):
        b = self.t(beta, self.torch.float64)
        self._lib.check(self.lib.slm_set_beta(self.h, slot, b.data_ptr(), self.e.stream), "slm_set_beta")
        self.torch.cuda.synchronize()

    def morph_loss(self, slot=0):
        out = self.torch.full((3,), -1.0, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_morph_loss(self.h, slot, out.data_ptr(), self.e.stream), "slm_morph_loss")
        o = out.cpu().numpy()
        return float(o[0]), int(o[1]), int(o[2])

    def targets(self, slot=0):
        N = self.e._frames[slot].N
        kept = self.torch.full((N,), 7, dtype=self.torch.uint8, device=self.dev)
        tgt = self.torch.full((N, 2), -1.0, dtype=self.torch.float64, device=self.dev)
        li = self.torch.full((N,), -1.0, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_morph_targets(self.h, slot, kept.data_ptr(), tgt.data_ptr(), li.data_ptr(), self.e.stream),
                        "slm_morph_targets")
        return kept.cpu().numpy(), tgt.cpu().numpy(), li.cpu().numpy()

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

    def close(self):
        self.e.close()


def _check_selection(r, fr, sem, beta, slot=0):
    """slm_morph_targets of a bound slot at its current beta (= ``beta``) against the model, array for array"""
    s = lmm.select(fr, sem, beta)
    kept, tgt, li = r.targets(slot)
    print("kept", int(kept.sum()), "model", s.n, "candidates", int(s.cand.sum()), "selection differs at", np.nonzero(kept != s.kept)[0][:8],
          "largest l_i difference", np.abs(li - s.li).max())
    assert set(np.unique(kept)) <= {0, 1}
    np.testing.assert_array_equal(kept.astype(bool), s.kept)
    np.testing.assert_array_equal(tgt, s.target)                      # half-integers: exact
    np.testing.assert_allclose(li, s.li, rtol=1e-12, atol=0)
    return s


def _check_system(r, fr, beta, sem, lam, us=(10.0, 10.0 / 7.5 ** 5), slot=0):
    """slm_morph_targets, slm_assemble, slm_morph_loss, slm_loss and slm_solve of a bound slot at beta against the model"""
    r.set_beta(beta, slot)
    s = _check_selection(r, fr, sem, beta, slot)
    A, b = r.assemble(slot)
    loss, n, cand = r.morph_loss(slot)
    parts = r.loss(slot)
    opt = orc.default_opt()
    A_ref, b_ref, M = lmm.normal_equations_with_morph(fr, beta, opt, sem, lam)
    want_loss, want_n, want_cand = lmm.morph_loss(fr, sem, beta, lam)
    print("term loss", loss, "model", want_loss, "kept", n, "candidates", cand, "largest entries: JtJ", np.abs(A_ref).max(), "jtl",
          np.abs(b_ref).max(), "largest differences: JtJ", np.abs(A - A_ref).max(), "jtl", np.abs(b - b_ref).max())
    assert (n, cand) == (want_n, want_cand) == (s.n, int(s.cand.sum()))
    np.testing.assert_allclose(loss, want_loss, rtol=1e-9, atol=0)
    np.testing.assert_allclose(parts[:3].sum() + loss, lmm.total_loss_with_morph(fr, beta, opt, sem, lam)[0], rtol=1e-8)
    assert int(parts[3]) == M                                        # the counts stay the ICP term's
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8 * max(1.0, np.abs(b_ref).max()))
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    if us:
        A32, b32 = _system_rot32(fr, beta, sem, lam)
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


# ---- 1. the selection and the system at a random small beta -------------------------------------------------------------
@pytest.mark.parametrize("solver_path", [2, 3])
@pytest.mark.parametrize("state_f64", [0, 1])
@pytest.mark.parametrize("K", [4, 6])
def test_selection_assemble_loss_and_solve_match_the_model(K, state_f64, solver_path):
    sc = cases.scene_k(K)
    fr, sem, lam, beta = cases.frame_of(sc), cases.sem_k(K), cases.weight_of(K), cases.ref_beta(sc.J)
    r = Run(lam, bool(state_f64), solver_path=solver_path)
    r.bind(0, sc, sem)
    A_ref = _check_system(r, fr, beta, sem, lam)
    r.close()
    A0 = orc.normal_equations(fr, beta, orc.default_opt())[0]
    data_max = np.abs(orc.normal_equations(fr, beta, orc.default_opt(mesh_arap=False, mesh_rot=False))[0]).max()
    assert np.abs(A_ref - A0).max() > 0.1 * data_max                 # the term is as visible a part of the system as the data term


def test_one_neighbour_on_the_default_solver_path():
    sc = cases.scene_k(1)
    fr, sem, beta = cases.frame_of(sc), cases.sem_k(1), cases.ref_beta(sc.J)
    lam = lmm.visible_weight(fr, sem, beta, orc.default_opt())
    r = Run(lam, solver_path=0)
    r.bind(0, sc, sem)
    _check_system(r, fr, beta, sem, lam)
    r.close()


# ---- 2. edge shapes of the search ---------------------------------------------------------------------------------------
def test_search_edge_shapes():
    """the short-list scene of tests/gf_shape_cases.py (a boundary list shorter than a wave, a workgroup whose 256 threads are
    all candidates); a class with exactly one boundary pixel, a class absent from the image and an eight-pixel list; surfels
    that project outside the image (tests/test_lm_morph_model.py asserts those properties of the inputs)"""
    import gf_shape_cases as shapes
    short = shapes.short_list_scene()
    sc = cases.scene_k(4)
    for name, scene, sem, beta in (("short list", short, lmm.sem_of(short), cases.identity(short.J)),
                                   ("ring", sc, cases.sem_k(4, "ring"), cases.ref_beta(sc.J)),
                                   ("outside", sc, cases.sem_k(4), cases.outside_beta(4))):
        fr = cases.frame_of(scene)
        lam = lmm.visible_weight(fr, sem, beta, orc.default_opt())
        print(name, "lambda", lam)
        r = Run(lam)
        r.bind(0, scene, sem)
        _check_system(r, fr, beta, sem, lam, us=(10.0,))
        r.close()


# ---- 3. n = 0 -----------------------------------------------------------------------------------------------------------
def test_no_kept_surfel_gives_the_system_of_an_enabled_solver_without_inputs():
    sc = cases.scene_k(4)
    sem, lam, beta = cases.sem_k(4, "none"), cases.weight_of(4), cases.ref_beta(sc.J)
    u, v = cases.DAMPING
    steps, runs = {}, {}
    for kind in ("no candidates", "no inputs", "never enabled"):
        r = Run(None if kind == "never enabled" else lam, u0=u, v=v)
        r.bind(0, sc, sem if kind == "no candidates" else None)
        if kind != "never enabled":
            assert r.morph_loss() == (0.0, 0, 0)                     # (at identity)
        r.set_beta(beta)
        steps[kind] = r.solve(0.37)
        r.bind(0, sc, sem if kind == "no candidates" else None)
        runs[kind] = r.run()[0]
        if kind == "no candidates":
            assert r.morph_loss()[:2] == (0.0, 0) and not r.targets()[0].any()
        r.close()
    for kind in ("no inputs", "never enabled"):                       # (never enabled: the tuple-sorted form)
        np.testing.assert_allclose(steps["no candidates"], steps[kind], rtol=0, atol=1e-11)
        np.testing.assert_allclose(runs["no candidates"][0], runs[kind][0], rtol=0, atol=1e-7)
        np.testing.assert_allclose([x["loss"] for x in runs["no candidates"][1]], [x["loss"] for x in runs[kind][1]], rtol=1e-9)
    want_beta, trace = cases.trace_of(4, 1.0, u, v, kind="none")
    _check_trace(runs["no candidates"][1], runs["no candidates"][0], trace, want_beta)


# ---- 4. ten iterations on a single slot --------------------------------------------------------------------------------
@pytest.mark.parametrize("K,factor,u,v", cases.TRACE_CASES)
def test_ten_iterations_match_the_models_loop(K, factor, u, v):
    sc = cases.scene_k(K)
    fr, sem, lam = cases.frame_of(sc), cases.sem_k(K), factor * cases.weight_of(K)
    want_beta, trace = cases.trace_of(K, factor, u, v)
    r = Run(lam, u0=u, v=v)
    r.bind(0, sc, sem)
    (got_beta, recs), = r.run()
    end = r.morph_loss()
    r.close()
    _check_trace(recs, got_beta, trace, want_beta)
    want_end = lmm.morph_loss(fr, sem, want_beta, lam)
    assert end[1:] == want_end[1:]
    np.testing.assert_allclose(end[0], want_end[0], rtol=1e-6, atol=1e-12)


# ---- 5. eight slots ----------------------------------------------------------------------------------------------------
def test_batch_of_eight_slots_with_unlike_inputs_and_one_without():
    sc, lam = cases.scene_k(cases.BATCH_K), cases.weight_of(cases.BATCH_K)
    u, v = cases.DAMPING
    kinds = cases.BATCH_KINDS                                        # (decided in the model at this weight: CPU test)
    sem = lambda kind: None if kind is None else cases.sem_k(cases.BATCH_K, kind)
    single = {}
    for kind in set(kinds):
        r = Run(lam, u0=u, v=v)
        r.bind(0, sc, sem(kind))
        single[kind] = r.run()[0]
        r.close()
    r = Run(None, u0=u, v=v)                                         # a solver on which the term was never enabled
    r.bind(0, sc)
    never = r.run()[0]
    r.close()
    r = Run(lam, slots=8, u0=u, v=v)
    r.e.bind_batch([r.frame(sc) for _ in kinds])                     # slm_bind_frames, then each slot's own inputs
    for i, kind in enumerate(kinds):
        if kind is not None:
            r.bind_morph(i, sem(kind))
    out = r.run(8)
    r.close()
    for i, kind in enumerate(kinds):
        beta, recs = out[i]
        print(i, kind, "largest difference to the single-slot run", np.abs(beta - single[kind][0]).max())
        np.testing.assert_allclose(beta, single[kind][0], rtol=0, atol=1e-7)
        np.testing.assert_allclose([x["loss"] for x in recs], [x["loss"] for x in single[kind][1]], rtol=1e-9)
        assert [x["accepted"] for x in recs] == [x["accepted"] for x in single[kind][1]]
        if kind is None:
            np.testing.assert_allclose(beta, never[0], rtol=0, atol=1e-7)
        else:
            assert np.abs(beta - never[0]).max() > 1e-6
    for kind in set(kinds):                                          # and the single-slot runs are the model's
        want_beta, trace = cases.batch_trace_of(kind)
        _check_trace(single[kind][1], single[kind][0], trace, want_beta)


# ---- 6. combinations ---------------------------------------------------------------------------------------------------
def test_combined_with_correspondences_hard_semantic_weights_and_the_face_term():
    import lm_face_model as lfm
    import lm_weight_model as lwm
    sc = cases.scene_k(4)
    fr, sem, lam, opt = cases.frame_of(sc), cases.sem_k(4), cases.weight_of(4), orc.default_opt()
    u, v = cases.DAMPING
    bases = cases.combined_bases(sc)
    for name in ("corr", "hard", "face"):
        trace = []
        want = lmm.lm_with_morph(fr, opt, sem, lam, u=u, v=v, trace=trace, base=bases[name])
        r = Run(lam, u0=u, v=v, corr=(2, 0.5) if name == "corr" else None, seg_mode=1 if name == "hard" else 0,
                face=cases.face_weight(sc) if name == "face" else None)
        if name == "face":
            r.set_mesh(0, lfm.scene_mesh(sc))
        r.bind(0, sc, sem)
        if name == "corr":
            r.bind_points(cases.corr_targets(sc))
        if name == "hard":
            r.bind_sem(lwm.sem_of(sc))
        (beta, recs), = r.run()
        r.close()
        print(name)
        _check_trace(recs, beta, trace, want)


# ---- 7. a model prepared ahead; a later bind clears the inputs ---------------------------------------------------------
def test_prepare_model_then_bind_equals_a_plain_bind_and_a_bind_clears_the_inputs():
    sc = cases.scene_k(6)
    sem, lam = cases.sem_k(6), cases.weight_of(6)
    u, v = cases.DAMPING
    outs = []
    for prepared in (False, True):
        r = Run(lam, u0=u, v=v)
        fr = r.frame(sc)
        if prepared:
            cs = fr.c_struct()
            r._lib.check(r.lib.slm_prepare_model(r.h, 0, C.byref(cs), r.e.stream), "slm_prepare_model")
        r.e.bind(0, fr)
        assert r.morph_loss() == (0.0, 0, 0)                         # no inputs yet
        r.bind_morph(0, sem)
        r.set_beta(cases.ref_beta(sc.J))
        step, at = r.solve(0.37), r.morph_loss()
        if prepared:
            cs = fr.c_struct()
            r._lib.check(r.lib.slm_prepare_model(r.h, 0, C.byref(cs), r.e.stream), "slm_prepare_model")
        r.e.bind(0, fr)                                              # a later bind clears the inputs: the term is off ...
        assert r.morph_loss() == (0.0, 0, 0)
        rc = r.lib.slm_morph_targets(r.h, 0, None, None, None, r.e.stream)
        assert rc == UNBOUND and r.lib.slm_last_error() == b"slm_morph_targets: slm_bind_morph first"
        r.set_beta(cases.ref_beta(sc.J))
        off = r.solve(0.37)
        r.e.bind(0, fr)
        r.bind_morph(0, sem)                                         # ... until they are bound again
        outs.append((step, at, off, r.run()[0]))
        r.close()
    (s0, a0, o0, r0), (s1, a1, o1, r1) = outs
    assert a0 == a1 and a0[1] > 0
    np.testing.assert_allclose(s0, s1, rtol=0, atol=1e-11)
    np.testing.assert_allclose(o0, o1, rtol=0, atol=1e-11)
    assert np.abs(s0 - o0).max() > 1e-6
    np.testing.assert_allclose([x["loss"] for x in r0[1]], [x["loss"] for x in r1[1]], rtol=1e-9)
    np.testing.assert_allclose(r0[0], r1[0], rtol=0, atol=1e-9)
    want_beta, trace = cases.trace_of(6, 1.0, u, v)
    _check_trace(r0[1], r0[0], trace, want_beta)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def _refused(lib, name, args, code, text):
    rc = getattr(lib, name)(*args)
    got = lib.slm_last_error()
    print(name, rc, got)
    assert rc == code, (name, rc, got)
    assert got == text, (name, got)


def test_refusals():
    import torch
    from super_amd.engine import Engine
    sc, sem, lam = cases.scene_k(3), cases.sem_k(3), 0.2
    pre = b"slm_enable_morph: "
    sharded = b"the solver is sharded (slm_set_shard); the term needs every surfel of the frame on one device"
    r = Run(None)
    lib, h = r.lib, r.h
    out = torch.zeros(3, dtype=torch.float64, device=r.dev)
    _refused(lib, "slm_enable_morph", (None, 1.0), INVALID, pre + b"null argument")
    for w in (float("nan"), float("inf")):
        _refused(lib, "slm_enable_morph", (h, w), INVALID, pre + b"weight must be finite")
    for kw, text in ((dict(data_path=1), b"needs the pair-record data path (data_path 0 or 2)"),
                     (dict(solver_path=1), b"needs a nested-dissection solver_path (0, 2, 3 or 4)"),
                     (dict(use_data=False), b"needs the data term (use_data 1)")):
        e = Engine(r.dev, **kw)
        _refused(lib, "slm_enable_morph", (e.h, 1.0), UNSUPPORTED, pre + text)
        e.close()
    e = Engine(r.dev)
    assert lib.slm_set_shard(e.h, 0, 1) == 0
    _refused(lib, "slm_enable_morph", (e.h, 1.0), UNSUPPORTED, pre + sharded)
    e.close()
    # before slm_enable_morph, and after a weight of 0 switched it off again
    assert lib.slm_enable_morph(h, 2.0) == 0 and lib.slm_enable_morph(h, 0.0) == 0
    args = r.morph_args(0, sem)
    _refused(lib, "slm_bind_morph", args, UNSUPPORTED, b"slm_bind_morph: slm_enable_morph first")
    _refused(lib, "slm_morph_loss", (h, 0, out.data_ptr(), None), UNSUPPORTED, b"slm_morph_loss: slm_enable_morph first")
    _refused(lib, "slm_morph_targets", (h, 0, None, None, None, None), UNSUPPORTED, b"slm_morph_targets: slm_enable_morph first")
    e = Engine(r.dev)                                                # the options combine
    assert (lib.slm_enable_morph(e.h, lam) == 0 and lib.slm_enable_face(e.h, 1.0) == 0 and lib.slm_enable_corr(e.h, 2, 0.5) == 0
            and lib.slm_enable_data_weights(e.h, 0, 2e-5) == 0)
    e.close()
    assert lib.slm_enable_morph(h, lam) == 0, lib.slm_last_error()
    _refused(lib, "slm_set_shard", (h, 0, 1), UNSUPPORTED,
             b"slm_set_shard: the boundary-morph term is enabled (slm_enable_morph); it needs every surfel of the frame on one device")
    _refused(lib, "slm_bind_morph", (None,) + args[1:], INVALID, b"slm_bind_morph: null argument")
    for k in (3, 4, 5):
        _refused(lib, "slm_bind_morph", args[:k] + (None,) + args[k + 1:], INVALID, b"slm_bind_morph: null argument")
    _refused(lib, "slm_bind_morph", (h, 1) + args[2:], INVALID, b"slm_bind_morph: bad slot")
    _refused(lib, "slm_bind_morph", (h, -1) + args[2:], INVALID, b"slm_bind_morph: bad slot")
    _refused(lib, "slm_bind_morph", args, UNBOUND, b"slm_bind_morph: slm_bind_frame first")
    _refused(lib, "slm_morph_loss", (None, 0, out.data_ptr(), None), INVALID, b"slm_morph_loss: null argument")
    _refused(lib, "slm_morph_loss", (h, 0, None, None), INVALID, b"slm_morph_loss: null argument")
    _refused(lib, "slm_morph_loss", (h, 3, out.data_ptr(), None), INVALID, b"slm_morph_loss: bad slot")
    _refused(lib, "slm_morph_loss", (h, 0, out.data_ptr(), None), UNBOUND, b"slm_morph_loss: slm_bind_frame first")
    _refused(lib, "slm_morph_targets", (None, 0, None, None, None, None), INVALID, b"slm_morph_targets: null argument")
    _refused(lib, "slm_morph_targets", (h, 2, None, None, None, None), INVALID, b"slm_morph_targets: bad slot")
    _refused(lib, "slm_morph_targets", (h, 0, None, None, None, None), UNBOUND, b"slm_morph_targets: slm_bind_frame first")
    fr = r.frame(sc)
    cs = fr.c_struct()
    cs.J = 65536
    _refused(lib, "slm_bind_frame", (h, 0, C.byref(cs), None), UNSUPPORTED,
             b"slm_bind_frame: the boundary-morph term (slm_enable_morph) needs J < 65536")
    r.bind(0, sc)
    _refused(lib, "slm_morph_targets", (h, 0, None, None, None, r.e.stream), UNBOUND, b"slm_morph_targets: slm_bind_morph first")
    for nc in (0, 5):
        _refused(lib, "slm_bind_morph", args[:2] + (nc,) + args[3:], UNSUPPORTED,
                 b"slm_bind_morph: num_classes must be in 1..SLM_MAX_CLASSES (4)")
    assert r.bind_morph(0, sem) == [len(e) for e in sem.edges]       # good inputs bind; every output of the read-out may be null
    assert lib.slm_morph_targets(h, 0, None, None, None, r.e.stream) == 0
    assert lib.slm_bind_morph(*(r.morph_args(0, sem)[:6] + (None, r.e.stream))) == 0     # and the counts' array too
    for w in (1.0, 0.0):
        _refused(lib, "slm_enable_morph", (h, w), INVALID, pre + b"a slot is already bound; call it after slm_create and before the first bind")
    r.close()


# ---- 9. Python surface --------------------------------------------------------------------------------------------------
def _with_sem(sc, sem, device="cuda"):
    import torch
    sf, inputs, new_data = torch_frame(sc, device)
    sf.seg = torch.from_numpy(np.ascontiguousarray(sem.sf_seg)).to(device)
    inputs[("seg", 0)] = torch.from_numpy(np.ascontiguousarray(sem.img_seg))[None, None].to(device)
    inputs[("seg_conf", 0)] = torch.from_numpy(np.ascontiguousarray(sem.img_seg_conf))[None].to(device)
    return sf, inputs, new_data


def test_python_surface():
    from super_amd.LM import LM_Solver
    K, factor, u, v = cases.TRACE_CASES[0]
    sc, sem = cases.scene_k(K), cases.sem_k(K)
    fr = cases.frame_of(sc)
    want_beta, trace = cases.trace_of(K, factor, u, v)
    opt = ref_opt(orc.default_opt())
    opt.num_classes = sem.C
    with pytest.raises(ValueError):
        LM_Solver(opt, morph_term=True)                              # needs opt.sf_bn_morph
    opt.sf_bn_morph, opt.sf_bn_morph_weight = True, factor * cases.weight_of(K)
    with pytest.raises(NotImplementedError):
        LM_Solver(opt, morph_term=True, rank=0, world=1)
    lm = LM_Solver(opt, morph_term=True, max_frames=2)
    sf, inputs, new_data = _with_sem(sc, sem)
    beta = lm.LM(sf, inputs, new_data, u=u, v=v).cpu().numpy()
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=TOL_BETA)
    np.testing.assert_allclose([x["loss"] for x in lm.last_records[0]], [t["loss"] for t in trace], rtol=1e-6)
    assert [x["accepted"] for x in lm.last_records[0]] == [t["accepted"] for t in trace]
    assert lm.last_edge_counts == [[len(e) for e in sem.edges]]
    want = lmm.morph_loss(fr, sem, want_beta, opt.sf_bn_morph_weight)
    got, = lm.last_morph_loss
    assert got[1:] == want[1:]
    np.testing.assert_allclose(got[0], want[0], rtol=1e-6, atol=1e-12)
    kept, tgt, li = lm.morph_targets(0, u, v)
    s = lmm.select(fr, sem, beta)
    np.testing.assert_array_equal(kept.cpu().numpy(), s.kept)
    # LM_batch: two slots with unlike inputs
    other = cases.sem_k(K, 9.0)
    b2 = lm.LM_batch([_with_sem(sc, sem), _with_sem(sc, other)], u=u, v=v)
    np.testing.assert_allclose(b2[0].cpu().numpy(), beta, rtol=0, atol=1e-7)
    want9, trace9 = cases.trace_of(K, factor, u, v, kind=9.0)
    np.testing.assert_allclose(b2[1].cpu().numpy(), want9, rtol=0, atol=TOL_BETA)
    np.testing.assert_allclose([x["loss"] for x in lm.last_records[1]], [t["loss"] for t in trace9], rtol=1e-6)
    assert len(lm.last_morph_loss) == 2 and lm.last_edge_counts[1] == [len(e) for e in other.edges]
    # a missing or mis-shaped field is named
    for key, name in ((("seg", 0), 'inputs[("seg",0)]'), (("seg_conf", 0), 'inputs[("seg_conf",0)]')):
        broken = dict(inputs)
        del broken[key]
        with pytest.raises(ValueError, match=re.escape(name + " is missing")):
            lm.LM(sf, broken, new_data, u=u, v=v)
        broken[key] = inputs[key][..., :-1]
        with pytest.raises(ValueError, match="must be"):
            lm.LM(sf, broken, new_data, u=u, v=v)
    seg = sf.seg
    del sf.seg
    with pytest.raises(ValueError, match="sf.seg is missing"):
        lm.LM(sf, inputs, new_data, u=u, v=v)
    sf.seg = seg[:-1]
    with pytest.raises(ValueError, match="sf.seg must be"):
        lm.LM(sf, inputs, new_data, u=u, v=v)
    sf.seg = seg
    # without the flag opt.sf_bn_morph is ignored exactly as today
    plain_opt = ref_opt(orc.default_opt())
    plain = LM_Solver(plain_opt).LM(*torch_frame(sc), u=u, v=v).cpu().numpy()
    ignored = LM_Solver(opt).LM(sf, inputs, new_data, u=u, v=v).cpu().numpy()
    np.testing.assert_allclose(ignored, plain, rtol=0, atol=1e-12)
    assert np.abs(beta - plain).max() > 1e-6
