"""The flow-correspondence term of the LM path (``slm_enable_corr``, include/super_lm.h) on the GPU, through the C ABI and the
Python surface, against the float64 model of tests/lm_corr_model.py.  Needs an MI355X (-m gpu).

Tolerances are those of tests/test_gpu_parity.py for the same quantities: JtJ 1e-7 of its largest entry, jtl 1e-8, loss 1e-8
relative (the term alone, in float64 throughout: 1e-9), ``slm_solve`` 1e-9 of the largest component against the model's
system with the Rot products in float32 (tests/test_gpu_lm_abi_num_neighbors.py), traces 1e-6 relative on the loss with the
accept flags compared where the decision is no rounding-level tie, final beta 1e-4 (north star).  Runs that assemble the
same system in another summation order agree to 1e-11 on the step and 1e-9 on beta after ten iterations (1e-7 where the
solver form differs too: a batch of eight against single frames).  Targets built from a flow agree with the model to
float32 rounding of the flow sample, 2e-7 of the largest coordinate (tests/test_gpu_graphfit_corr.py)."""
import ctypes as C

import numpy as np
import pytest

import lm_corr_model as lcm
import test_lm_corr_model as cases
from helpers import GF_CORR_VARIANTS, load_corr_golden, load_golden, ref_opt, torch_frame
from oracle import graphfit_oracle as gfo
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

TOL_BETA = 1e-4
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _scene(name):
    """name -> a Scene with a flow"""
    def make():
        from super_amd import synth
        if name == "golden":
            return load_corr_golden()[1]
        if name == "scene2":
            return cases.scene2()
        if name == "reject":
            return cases.reject_case_scene()[0]
        if name == "j108":
            sc = load_golden("s120x160_j108")[1]
            sc.flow = synth.smooth_flow(sc.H, sc.W, 11, amp=(2.0, 1.5))
            return sc
        if name == "n37":
            sc = synth.make_scene(N=37, J=12, H=60, W=80, seed=3, src_border=6, tgt_border=3)
            sc.flow = synth.smooth_flow(sc.H, sc.W, 5, amp=(1.0, 1.0))
            return sc
        K = int(name[1:])      # "k6": the scenes of the num_neighbors cases
        sc = synth.make_scene(N=1200, J=40, H=60, W=80, seed=60 + K, n_neighbors=K, src_border=4, tgt_border=3, tgt_holes=0.01)
        sc.flow = synth.smooth_flow(sc.H, sc.W, 20 + K, amp=(2.0, 1.5))
        return sc
    return _cached(("scene", name), make)


def _frame(name):
    return _cached(("frame", name), lambda: orc.Frame.from_scene(_scene(name)))


def _targets(name):
    return _cached(("targets", name), lambda: lcm.targets_from_flow(_frame(name), _scene(name).flow))


def _beta(name):
    return lcm.random_beta(_scene(name).J, 17, rot=0.01, trans=0.002)


def _system_rot32(name, beta, targets, mode, lam):
    """the model's normal equations with the Rot products rounded to float32 as the reference (and the library) forms them"""
    opt = orc.default_opt()
    A, b, M = lcm.normal_equations_with_corr(_frame(name), beta, orc.default_opt(mesh_rot=False), targets, mode, lam)
    t = orc.rot_term(beta, opt.mesh_rot_weight, grad=True)
    jv, r = t.Jq.astype(np.float32), t.r.astype(np.float32)
    jtj = (jv[:, :, None] * jv[:, None, :]).astype(np.float64)
    jtr = (jv * r[:, None]).astype(np.float64)
    base = 7 * np.arange(len(jv))
    for c in range(4):
        b[base + c] -= jtr[:, c]
        for d in range(4):
            A[base + c, base + d] += jtj[:, c, d]
    return A, b, M


class Run:
    """an Engine with the term enabled (mode 0: never enabled), its scene bound to every slot asked for"""

    def __init__(self, name, mode, lam, state_f64=True, slots=1, **kw):
        import torch
        from super_amd import _lib
        from super_amd.engine import DeviceFrame, Engine
        self.torch, self._lib = torch, _lib
        self.dev = torch.device("cuda", 0)
        self.e = Engine(self.dev, max_frames=slots, **kw)
        self.lib, self.h = self.e.lib, self.e.h
        if mode:
            _lib.check(self.lib.slm_enable_corr(self.h, mode, lam), "slm_enable_corr")
        self.name, self.mode, self.lam, self.state_f64 = name, mode, lam, state_f64
        self.keep = []
        if name is not None:
            self.bind(0, name)

    def bind(self, slot, name):
        from super_amd.engine import DeviceFrame
        self.e.bind(slot, DeviceFrame.from_scene(_scene(name), self.dev, state_f64=self.state_f64))

    def bind_flow(self, slot=0, name=None):
        fl = self.torch.from_numpy(np.ascontiguousarray(_scene(name or self.name).flow, dtype=np.float32)).to(self.dev)
        self.keep.append(fl)
        self._lib.check(self.lib.slm_bind_corr_flow(self.h, slot, fl.data_ptr(), self.e.stream), "slm_bind_corr_flow")

    def bind_points(self, targets, slot=0):
        o, n, valid = targets
        t = lambda a, dt: self.torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dt)
        o, n, valid = t(o, self.torch.float64), t(n, self.torch.float64), t(valid, self.torch.uint8)
        self.keep += [o, n, valid]
        self._lib.check(self.lib.slm_bind_corr_points(self.h, slot, o.data_ptr(), n.data_ptr(), valid.data_ptr(), self.e.stream),
                        "slm_bind_corr_points")

    def targets(self, slot=0):
        N = self.e._frames[slot].N
        o = self.torch.empty((N, 3), dtype=self.torch.float64, device=self.dev)
        n = self.torch.empty((N, 3), dtype=self.torch.float64, device=self.dev)
        v = self.torch.empty(N, dtype=self.torch.uint8, device=self.dev)
        self._lib.check(self.lib.slm_corr_get_targets(self.h, slot, o.data_ptr(), n.data_ptr(), v.data_ptr(), self.e.stream),
                        "slm_corr_get_targets")
        return o.cpu().numpy(), n.cpu().numpy(), v.cpu().numpy().astype(bool)

    def set_beta(self, beta, slot=0):
        b = self.torch.from_numpy(np.ascontiguousarray(beta)).to(self.dev)
        self._lib.check(self.lib.slm_set_beta(self.h, slot, b.data_ptr(), self.e.stream), "slm_set_beta")

    def corr_loss(self, slot=0):
        out = self.torch.empty(2, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_corr_loss(self.h, slot, out.data_ptr(), self.e.stream), "slm_corr_loss")
        o = out.cpu().numpy()
        return float(o[0]), int(o[1])

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


def _check_trace(recs, beta, trace, want_beta):
    assert all(r["status"] == 0 for r in recs)
    loss = np.array([r["loss"] for r in recs])
    want = np.array([t["loss"] for t in trace])
    print("loss", loss, "\nwant", want)
    np.testing.assert_allclose(loss, want, rtol=1e-6, atol=1e-12)
    dec = cases.decisive(want)
    acc = np.array([r["accepted"] for r in recs])
    np.testing.assert_array_equal(acc[dec], np.array([t["accepted"] for t in trace])[dec])
    if dec.all():
        np.testing.assert_allclose([r["u"] for r in recs], [t["u"] for t in trace], rtol=1e-12)
    assert [r["M_loss"] for r in recs] == [t["M_loss"] for t in trace]      # M_grad / M_loss stay the ICP match counts
    assert [r["M_grad"] for r in recs] == [t["M_grad"] for t in trace]
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=TOL_BETA)


# ---- 1. construction ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["golden", "scene2"])
def test_targets_from_a_flow_match_the_model(name):
    sc = _scene(name)
    o, n, valid = _targets(name)
    r = Run(name, 1, 1.0)
    r.bind_flow()
    go, gn, gv = r.targets()
    loss, kept = r.corr_loss()
    r.close()
    tie = lcm.tie_distance(_frame(name), sc.flow) <= 1e-4
    print("kept", kept, "model", int(valid.sum()), "of", sc.N, "excluded", int(tie.sum()))
    assert tie.mean() <= 0.01
    np.testing.assert_array_equal(gv[~tie], valid[~tie])
    both = gv & valid
    assert both.sum() > 0.7 * sc.N and kept == int(gv.sum()) < sc.N
    np.testing.assert_allclose(go[both], o[both], rtol=0, atol=2e-7 * np.abs(o).max())
    np.testing.assert_allclose(gn[both], n[both], rtol=0, atol=2e-7 * np.abs(n).max())
    assert not go[~gv].any() and not gn[~gv].any()


@pytest.mark.parametrize("tag,mode", [("corr", 1), ("corrpp", 2)])
@pytest.mark.parametrize("name", ["golden", "scene2"])
def test_loss_at_identity_equals_graphfit_on_the_same_device(name, tag, mode):
    import torch
    from types import SimpleNamespace
    from super_amd.deform_mesh import GraphFit
    sc = _scene(name)
    opt = gfo.default_opt(**GF_CORR_VARIANTS[tag])
    opt.deform_udpate_method = "super_edg"
    sf, inputs, new_data = torch_frame(sc)
    sf.rgb = torch.zeros(1, 3, sc.H, sc.W, device="cuda")
    models = SimpleNamespace(optical_flow=lambda a, b: [torch.from_numpy(sc.flow).cuda()])
    gf = GraphFit(opt)
    dv = torch.zeros((sc.J + 1, 7), dtype=torch.float64, device="cuda")
    dv[:, 0] = 1.0
    terms, _, _ = gf.loss_and_grad(inputs, sf, new_data, dv, models)
    lam = 0.7
    r = Run(name, mode, lam)
    r.bind_flow()
    loss, kept = r.corr_loss()
    r.close()
    print(loss / lam ** 2, terms["corr_loss"] / opt.sf_corr_weight, kept, gf.last_corr_kept)
    assert kept == gf.last_corr_kept
    np.testing.assert_allclose(loss / lam ** 2, terms["corr_loss"] / opt.sf_corr_weight, rtol=1e-12)


# ---- 2. downstream, fed the read-back targets --------------------------------------------------------------------------
def _shared_targets(name, mode, lam, state_f64):
    """the device's own targets of a flow (so that model and device share inputs exactly), read back once"""
    def make():
        r = Run(name, mode, lam, state_f64)
        r.bind_flow()
        t = r.targets()
        r.close()
        return t
    return _cached(("dev_targets", name, state_f64), make)


@pytest.mark.parametrize("state_f64", [0, 1])
@pytest.mark.parametrize("K", [1, 3, 4, 6, 8])
@pytest.mark.parametrize("mode", [1, 2])
def test_assemble_loss_solve_and_trace_match_the_model(mode, K, state_f64):
    name, lam = f"k{K}", 0.5
    fr, tg = _frame(name), _shared_targets(f"k{K}", mode, lam, bool(state_f64))
    assert 0.5 * len(tg[2]) < tg[2].sum() < len(tg[2])
    beta = _beta(name)
    r = Run(name, mode, lam, bool(state_f64))
    r.bind_points(tg)
    r.set_beta(beta)
    A, b = r.assemble()
    loss, kept = r.corr_loss()
    A_ref, b_ref, _ = lcm.normal_equations_with_corr(fr, beta, orc.default_opt(), tg, mode, lam)
    want_loss, want_kept = lcm.corr_loss(fr, beta, tg, mode, lam)
    assert kept == want_kept
    np.testing.assert_allclose(loss, want_loss, rtol=1e-9)
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    # the term is a visible part of the system
    A0, _, _ = orc.normal_equations(fr, beta, orc.default_opt())
    assert np.abs(A_ref - A0).max() > 1e-3 * np.abs(A0).max()
    A32, b32, _ = _system_rot32(name, beta, tg, mode, lam)
    for u in (10.0, 10.0 / 7.5 ** 5):
        ref = orc.solve_damped(A32, b32, u)
        np.testing.assert_allclose(r.solve(u), ref, rtol=0, atol=1e-9 * max(1.0, np.abs(ref).max()))
    r.close()
    # the ten-iteration loop from identity
    r = Run(name, mode, lam, bool(state_f64))
    r.bind_points(tg)
    (got_beta, recs), = r.run()
    r.close()
    trace = []
    want_beta = lcm.lm_with_corr(fr, orc.default_opt(), tg, mode, lam, trace=trace)
    _check_trace(recs, got_beta, trace, want_beta)


@pytest.mark.parametrize("state_f64", [0, 1])
def test_trace_with_a_reject_followed_by_an_accept(state_f64):
    c = cases.REJECT_CASE
    sc, opt = cases.reject_case_scene()
    fr = _frame("reject")
    tg = _shared_targets("reject", c["mode"], c["lam"], bool(state_f64))
    trace = []
    want_beta = lcm.lm_with_corr(fr, opt, tg, c["mode"], c["lam"], u=c["u"], v=c["v"], trace=trace)
    acc, dec = [t["accepted"] for t in trace], cases.decisive([t["loss"] for t in trace])
    assert any((not a) and b and da and db for a, b, da, db in zip(acc, acc[1:], dec, dec[1:]))
    r = Run("reject", c["mode"], c["lam"], bool(state_f64), u0=c["u"], v=c["v"])
    r.bind_points(tg)
    (got_beta, recs), = r.run()
    r.close()
    _check_trace(recs, got_beta, trace, want_beta)
    assert [x["accepted"] for x in recs] == acc


# ---- 3. edge shapes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("n37", 1), ("n37", 2), ("golden", 1), ("scene2", 2)])
def test_sizes_below_a_wave_and_off_the_wave_multiple(name, mode):
    """N = 37 (less than one wave), 1500 and 3000 (no multiple of 64): the loop against the model"""
    lam = 0.4
    fr, tg = _frame(name), _shared_targets(name, mode, lam, True)
    assert tg[2].sum() > 0 and len(tg[2]) in (37, 1500, 3000)
    r = Run(name, mode, lam)
    r.bind_points(tg)
    (got_beta, recs), = r.run()
    r.close()
    trace = []
    want_beta = lcm.lm_with_corr(fr, orc.default_opt(), tg, mode, lam, trace=trace)
    _check_trace(recs, got_beta, trace, want_beta)


def test_no_valid_correspondence_equals_the_run_without_the_term():
    name, mode, lam = "golden", 1, 0.5
    o, n, valid = _shared_targets(name, mode, lam, True)
    outs = []
    for bound in (True, False):
        r = Run(name, mode, lam)
        if bound:
            r.bind_points((o, n, np.zeros_like(valid)))
            assert r.corr_loss() == (0.0, 0)
        r.set_beta(_beta(name))
        step = r.solve(0.37)
        r.bind(0, name)
        if bound:
            r.bind_points((o, n, np.zeros_like(valid)))
        outs.append((step, r.run()[0]))
        r.close()
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-11)
    np.testing.assert_allclose(outs[0][1][0], outs[1][1][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose([x["loss"] for x in outs[0][1][1]], [x["loss"] for x in outs[1][1][1]], rtol=1e-12)


@pytest.mark.parametrize("mode", [1, 2])
def test_exactly_one_valid_correspondence(mode):
    name, lam = "golden", 2.0
    o, n, valid = _shared_targets(name, mode, lam, True)
    one = np.zeros_like(valid)
    one[np.nonzero(valid)[0][len(valid) // 3]] = True
    tg = (o, n, one)
    fr, beta = _frame(name), _beta(name)
    r = Run(name, mode, lam)
    r.bind_points(tg)
    r.set_beta(beta)
    A, b = r.assemble()
    assert r.corr_loss()[1] == 1
    np.testing.assert_allclose(r.corr_loss()[0], lcm.corr_loss(fr, beta, tg, mode, lam)[0], rtol=1e-9)
    A_ref, b_ref, _ = lcm.normal_equations_with_corr(fr, beta, orc.default_opt(), tg, mode, lam)
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    A32, b32, _ = _system_rot32(name, beta, tg, mode, lam)
    ref = orc.solve_damped(A32, b32, 0.37)
    got = r.solve(0.37)
    r.close()
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-9 * max(1.0, np.abs(ref).max()))
    # the one row is visible in the step
    A0, b0, _ = _system_rot32(name, beta, None, mode, lam)
    assert np.abs(ref - orc.solve_damped(A0, b0, 0.37)).max() > 1e-6


@pytest.mark.parametrize("mode", [1, 2])
def test_targets_on_a_known_warp_give_zero_loss_there(mode):
    name, lam = "golden", 1.5
    fr = _frame(name)
    star = lcm.random_beta(fr.J, 23)
    T, _ = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, star)
    nrm = np.tile([0.0, 0.6, 0.8], (len(T), 1))
    valid = np.ones(len(T), bool)
    r = Run(name, mode, lam)
    r.bind_points((T, nrm, valid))
    at_identity, kept = r.corr_loss()
    r.set_beta(star)
    at_star, _ = r.corr_loss()
    r.close()
    print(at_identity, at_star)
    assert kept == len(T) and at_identity > 1e-6
    assert at_star < 1e-24        # |T - o| is rounding, 1e-16 per coordinate, squared and summed over 1500 surfels


# ---- 4. solver forms ---------------------------------------------------------------------------------------------------
def test_solver_forms_agree_with_each_other_and_the_model():
    name, mode, lam = "j108", 1, 0.5
    fr, tg = _frame(name), _shared_targets(name, mode, lam, True)
    opt = load_golden("s120x160_j108")[2]
    trace = []
    want_beta = lcm.lm_with_corr(fr, opt, tg, mode, lam, trace=trace)
    betas = {}
    for path in (0, 2, 3, 4):
        r = Run(name, mode, lam, solver_path=path)
        r.bind_points(tg)
        (betas[path], recs), = r.run()
        r.close()
        _check_trace(recs, betas[path], trace, want_beta)
    for path in (2, 3, 4):
        np.testing.assert_allclose(betas[path], betas[0], rtol=0, atol=1e-9)


# ---- 5. batches and prepared models ------------------------------------------------------------------------------------
def test_batch_of_eight_slots_with_flows_points_and_none():
    mode, lam = 2, 0.5
    names = ["golden", "scene2", "reject", "golden", "scene2", "reject", "golden", "scene2"]
    kinds = ["flow", "points", "none", "points", "none", "flow", "none", "flow"]
    single = {}
    for name, kind in set(zip(names, kinds)):
        r = Run(name, mode if kind != "never" else 0, lam)
        if kind == "flow":
            r.bind_flow()
        elif kind == "points":
            r.bind_points(_shared_targets(name, mode, lam, True))
        single[(name, kind)] = r.run()[0]
        r.close()
    for name in set(names):                          # a solver on which the term was never enabled
        r = Run(name, 0, 0.0)
        single[(name, "never")] = r.run()[0]
        r.close()
    r = Run(None, mode, lam, slots=8)
    for i, name in enumerate(names):
        r.bind(i, name)
    for i, (name, kind) in enumerate(zip(names, kinds)):
        if kind == "flow":
            r.bind_flow(i, name)
        elif kind == "points":
            r.bind_points(_shared_targets(name, mode, lam, True), i)
    out = r.run(8)
    kept = [r.corr_loss(i)[1] for i in range(8)]
    r.close()
    for i, (name, kind) in enumerate(zip(names, kinds)):
        beta, recs = out[i]
        np.testing.assert_allclose(beta, single[(name, kind)][0], rtol=0, atol=1e-7)
        np.testing.assert_allclose([x["loss"] for x in recs], [x["loss"] for x in single[(name, kind)][1]], rtol=1e-9)
        assert (kept[i] > 0) == (kind != "none")
        if kind == "none":
            np.testing.assert_allclose(beta, single[(name, "never")][0], rtol=0, atol=1e-7)
            np.testing.assert_allclose([x["loss"] for x in recs], [x["loss"] for x in single[(name, "never")][1]], rtol=1e-9)
        else:
            assert np.abs(beta - single[(name, "never")][0]).max() > 1e-6
    # a flow and the points read back from it are the same term
    np.testing.assert_allclose(single[("golden", "flow")][0], single[("golden", "points")][0], rtol=0, atol=1e-9)


def test_enabled_solver_without_correspondences_solves_the_default_system():
    """the pair form at num_neighbors 4 against the default tuple-sorted form: the same step"""
    name = "golden"
    steps = []
    for mode in (1, 0):
        r = Run(name, mode, 0.5)
        r.set_beta(_beta(name))
        steps.append(r.solve(0.37))
        r.close()
    np.testing.assert_allclose(steps[0], steps[1], rtol=0, atol=1e-11)


def test_rebinding_a_slot_drops_its_correspondences():
    name, mode, lam = "golden", 1, 0.5
    r = Run(name, mode, lam)
    r.bind_flow()
    assert r.corr_loss()[1] > 0
    with_term = r.run()[0][0]
    r.bind(0, name)
    assert r.corr_loss() == (0.0, 0)
    without = r.run()[0][0]
    r.close()
    r = Run(name, mode, lam)
    plain = r.run()[0][0]
    r.close()
    np.testing.assert_allclose(without, plain, rtol=0, atol=1e-9)
    assert np.abs(with_term - plain).max() > 1e-6


# ---- 6. Python surface --------------------------------------------------------------------------------------------------
def _lm_solver(tag, **kw):
    from super_amd.LM import LM_Solver
    opt = ref_opt(orc.default_opt())
    for k, v in GF_CORR_VARIANTS[tag].items():
        if k.startswith("sf_corr"):
            setattr(opt, k, v)
    return LM_Solver(opt, corr_term=True, **kw), opt


@pytest.mark.parametrize("tag,mode", [("corr", 1), ("corrpp", 2)])
def test_python_surface_returns_the_c_abi_runs(tag, mode):
    import torch
    names = ["golden", "scene2", "reject"]
    lm, opt = _lm_solver(tag)
    lam = opt.sf_corr_weight
    want = {}
    for name in names:
        r = Run(name, mode, lam)
        r.bind_flow()
        want[name] = r.run()[0]
        r.close()
    r = Run("golden", 0, 0.0)
    never = r.run()[0][0]
    r.close()
    flow = lambda name: torch.from_numpy(_scene(name).flow).cuda()
    sc = _scene("golden")
    beta = lm.LM(*torch_frame(sc), flow=flow("golden")).cpu().numpy()
    np.testing.assert_allclose(beta, want["golden"][0], rtol=0, atol=1e-9)
    assert lm.last_corr_kept == [int(lm.corr_targets()[2].sum())] and lm.last_corr_kept[0] > 1000
    np.testing.assert_allclose([x["loss"] for x in lm.last_records[0]], [x["loss"] for x in want["golden"][1]], rtol=1e-9)
    # the targets handed in directly, and a prepared model
    pts, nrm, valid = lm.corr_targets()
    beta2 = lm.LM(*torch_frame(sc), corr_points=(pts, nrm, valid)).cpu().numpy()
    np.testing.assert_allclose(beta2, beta, rtol=0, atol=1e-9)
    sf, inputs, new_data = torch_frame(sc)
    lm.prepare_model(sf)
    beta3 = lm.LM(sf, inputs, new_data, flow=flow("golden")).cpu().numpy()
    np.testing.assert_allclose(beta3, beta, rtol=0, atol=1e-9)
    # prepareCostTerm includes the term
    bt = torch.from_numpy(_beta("golden")).cuda()
    total = float(lm.prepareCostTerm(sf, inputs, new_data, bt, flow=flow("golden")))
    base = orc.total_loss(_frame("golden"), _beta("golden"), orc.default_opt())[0]
    tg = tuple(t.cpu().numpy() for t in (pts, nrm, valid))
    np.testing.assert_allclose(total, base + lcm.corr_loss(_frame("golden"), _beta("golden"), tg, mode, lam)[0], rtol=1e-8)
    jtj, jtl = lm.prepareCostTerm(sf, inputs, new_data, bt, grad=True, flow=flow("golden"))
    A_ref, b_ref, _ = lcm.normal_equations_with_corr(_frame("golden"), _beta("golden"), orc.default_opt(), tg, mode, lam)
    np.testing.assert_allclose(jtl.cpu().numpy().reshape(-1), b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(jtj.cpu().numpy(), A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    # a batch: a flow, a triple, none
    lmb, _ = _lm_solver(tag, max_frames=3)
    tg2 = _shared_targets("scene2", mode, lam, True)
    tri = tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in tg2)
    betas = lmb.LM_batch([torch_frame(_scene("reject")) + (flow("reject"),), torch_frame(_scene("scene2")) + (tri,),
                          torch_frame(sc) + (None,)])
    np.testing.assert_allclose(betas[0].cpu().numpy(), want["reject"][0], rtol=0, atol=1e-7)
    np.testing.assert_allclose(betas[1].cpu().numpy(), want["scene2"][0], rtol=0, atol=1e-7)
    np.testing.assert_allclose(betas[2].cpu().numpy(), never, rtol=0, atol=1e-7)
    assert lmb.last_corr_kept[2] is None and lmb.last_corr_kept[0] > 0 and lmb.last_corr_kept[1] == int(tg2[2].sum())
