"""The per-residual weights of the LM path's point-to-plane term (``slm_enable_data_weights``, include/super_lm.h) on the
GPU, through the C ABI and the Python surface, against the float64 model of tests/lm_weight_model.py.  Needs an MI355X
(-m gpu).

Tolerances are the project's own for the same quantities (docstring of tests/test_gpu_lm_corr.py): JtJ 1e-7 of its largest
entry, jtl 1e-8, loss 1e-8 relative, ``slm_solve`` 1e-9 of the largest component against the model's system with the Rot
products in float32, traces 1e-6 relative on the loss with the accept flags compared where the decision is no rounding-level
tie, final beta 1e-4; runs that differ only in summation order 1e-11 on the step and 1e-9 on beta.  Weights from
``slm_data_weights`` against the model: 1e-12 absolute (both sides float64; a JSD over at most four classes is a handful of
exp / log calls a few ulp apart).  Largest difference observed on an MI355X: see OBSERVED_MAX_WEIGHT_DIFF below.

Conditions, asserted on the model at every beta a comparison is made at (``lm_weight_model.check_conditions``): no matched
surfel with a top-two gap of conf below 1e-9 (hard), none with |s / pp_max - 1| below 1e-9 (truncation).  No surfel is
excluded."""
import ctypes as C

import numpy as np
import pytest

import lm_corr_model as lcm
import lm_weight_model as lwm
from helpers import ref_opt, torch_frame
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

OBSERVED_MAX_WEIGHT_DIFF = 1.2e-16     # soft weights, over every case of this file (hard and truncation weights are exact)
TOL_W = 1e-12
TOL_BETA = 1e-4
PP = 2e-5
CONFIGS = {"hard": (1, 0.0), "soft": (2, 0.0), "trunc": (0, PP)}
CLASSES = {1: 2, 4: 4, 6: 2, 8: 4}          # num_neighbors -> classes of the 1200-surfel scenes
UNBOUND = 4
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _scene(name):
    def make():
        from super_amd import synth
        if name == "n37":       # one partial wave
            return synth.make_scene(N=37, J=12, H=60, W=80, seed=3, n_neighbors=4, src_border=6, tgt_border=3, tgt_holes=0.0,
                                    semantic=True, num_classes=2)
        if name == "n65":       # a wave and one lane
            return synth.make_scene(N=65, J=12, H=60, W=80, seed=4, n_neighbors=4, src_border=6, tgt_border=3, tgt_holes=0.0,
                                    semantic=True, num_classes=3)
        if name == "n65c1":     # one class
            return synth.make_scene(N=65, J=12, H=60, W=80, seed=5, n_neighbors=6, src_border=6, tgt_border=3, tgt_holes=0.0,
                                    semantic=True, num_classes=1)
        K = int(name[1:])       # "k6": more than one block, holes in the target
        return synth.make_scene(N=1200, J=40, H=60, W=80, seed=60 + K, n_neighbors=K, src_border=4, tgt_border=3,
                                tgt_holes=0.01, semantic=True, num_classes=CLASSES[K])
    return _cached(("scene", name), make)


def _frame(name):
    return _cached(("frame", name), lambda: orc.Frame.from_scene(_scene(name)))


def _sem(name):
    return _cached(("sem", name), lambda: lwm.sem_of(_scene(name)))


def _beta(name):
    return lcm.random_beta(_scene(name).J, 17, rot=0.01, trans=0.002)


def _system_rot32(name, sem, beta, seg_mode, pp_max, corr=None):
    """the model's normal equations with the Rot products rounded to float32 as the reference (and the library) forms them"""
    opt = orc.default_opt()
    A, b, M = lwm.normal_equations(_frame(name), sem, beta, orc.default_opt(mesh_rot=False), seg_mode, pp_max, corr)
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


def decisive(losses):
    """iterations whose accept decision is not a rounding-level tie (tests/test_gpu_parity.py)"""
    losses = np.asarray(losses)
    best = np.minimum.accumulate(np.concatenate([[1e10], losses]))[:-1]
    return np.abs(losses - best) > 1e-9 * np.abs(best)


class Run:
    """an Engine with the weights enabled (``cfg`` None: never enabled), scenes bound with their semantic inputs"""

    def __init__(self, name, cfg, state_f64=True, slots=1, corr=None, shard=False, sem=None, **kw):
        import torch
        from super_amd import _lib
        from super_amd.engine import Engine
        self.torch, self._lib = torch, _lib
        self.dev = torch.device("cuda", 0)
        self.e = Engine(self.dev, max_frames=slots, **kw)
        self.lib, self.h = self.e.lib, self.e.h
        self.cfg = CONFIGS[cfg] if isinstance(cfg, str) else cfg
        if self.cfg is not None:
            _lib.check(self.lib.slm_enable_data_weights(self.h, self.cfg[0], self.cfg[1]), "slm_enable_data_weights")
        if corr is not None:
            _lib.check(self.lib.slm_enable_corr(self.h, corr[0], corr[1]), "slm_enable_corr")
        if shard:
            _lib.check(self.lib.slm_set_shard(self.h, 0, 1), "slm_set_shard")
        self.state_f64, self.keep = state_f64, {}
        if name is not None:
            self.bind(0, name, sem)

    def bind(self, slot, name, sem=None, semantic=True):
        from super_amd.engine import DeviceFrame
        self.e.bind(slot, DeviceFrame.from_scene(_scene(name), self.dev, state_f64=self.state_f64))
        if semantic and self.cfg is not None and self.cfg[0]:
            self.bind_sem(slot, sem or _sem(name))

    def bind_sem(self, slot, sem):
        t = lambda a, dt: self.torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dt)
        seg, sc, tc = t(sem.sf_seg, self.torch.int32), t(sem.sf_seg_conf, self.torch.float32), t(sem.tgt_seg_conf, self.torch.float32)
        self.keep[slot] = (seg, sc, tc)
        self._lib.check(self.lib.slm_bind_data_semantic(self.h, slot, sc.shape[1], seg.data_ptr(), sc.data_ptr(), tc.data_ptr(),
                                                        self.e.stream), "slm_bind_data_semantic")

    def bind_points(self, targets, slot=0):
        o, n, valid = targets
        t = lambda a, dt: self.torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dt)
        o, n, valid = t(o, self.torch.float64), t(n, self.torch.float64), t(valid, self.torch.uint8)
        self.keep[("corr", slot)] = (o, n, valid)
        self._lib.check(self.lib.slm_bind_corr_points(self.h, slot, o.data_ptr(), n.data_ptr(), valid.data_ptr(), self.e.stream),
                        "slm_bind_corr_points")

    def set_beta(self, beta, slot=0):
        b = self.torch.from_numpy(np.ascontiguousarray(beta)).to(self.dev)
        self._lib.check(self.lib.slm_set_beta(self.h, slot, b.data_ptr(), self.e.stream), "slm_set_beta")

    def weights(self, slot=0):
        w = self.torch.full((self.e._frames[slot].N,), -1.0, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_data_weights(self.h, slot, w.data_ptr(), self.e.stream), "slm_data_weights")
        return w.cpu().numpy()

    def loss(self, slot=0):
        out = self.torch.zeros(4, dtype=self.torch.float64, device=self.dev)
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

    def run_sharded(self, n=1, iters=10):
        lib, h, st, chk = self.lib, self.h, self.e.stream, self._lib.check
        for _ in range(iters):          # world = 1: the exchanges are the identity
            chk(lib.slm_lm_grad_local(h, n, st), "slm_lm_grad_local")
            chk(lib.slm_lm_solve(h, n, st), "slm_lm_solve")
            chk(lib.slm_lm_loss_local(h, n, st), "slm_lm_loss_local")
            chk(lib.slm_lm_accept(h, n, st), "slm_lm_accept")
        return [(self.e.beta(i).cpu().numpy(), self.e.records(i)) for i in range(n)]

    def close(self):
        self.e.close()


def _check_weights(got, name, sem, beta, seg_mode, pp_max):
    want, ww = lwm.weights_all(_frame(name), sem, beta, seg_mode, pp_max)
    lwm.check_conditions(ww, seg_mode, pp_max)
    diff = np.abs(got - want).max()
    print(name, "seg_mode", seg_mode, "pp_max", pp_max, "matched", len(ww.t.match), "of", len(want), "zero weights",
          int((ww.w == 0).sum()), "largest weight difference", diff)
    np.testing.assert_allclose(got, want, rtol=0, atol=TOL_W)
    return ww


def _model_trace(name, sem, seg_mode, pp_max, corr=None, opt=None):
    fr, trace = _frame(name), []
    cond = lambda b: lwm.check_conditions(lwm.weights(fr, sem, b, seg_mode, pp_max), seg_mode, pp_max)
    beta = lwm.lm(fr, sem, opt or orc.default_opt(), seg_mode, pp_max, corr, trace=trace, on_beta=cond)
    return beta, trace


def _check_trace(recs, beta, trace, want_beta):
    assert all(r["status"] == 0 for r in recs)
    loss = np.array([r["loss"] for r in recs])
    want = np.array([t["loss"] for t in trace])
    print("loss", loss, "\nwant", want)
    np.testing.assert_allclose(loss, want, rtol=1e-6, atol=1e-12)
    dec = decisive(want)
    acc = np.array([r["accepted"] for r in recs])
    np.testing.assert_array_equal(acc[dec], np.array([t["accepted"] for t in trace])[dec])
    assert [r["M_loss"] for r in recs] == [t["M_loss"] for t in trace]      # M_grad / M_loss stay the match-set counts
    assert [r["M_grad"] for r in recs] == [t["M_grad"] for t in trace]
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=TOL_BETA)


def _check_point(r, name, sem, beta, seg_mode, pp_max, corr=None):
    """weights, slm_assemble, slm_loss and slm_solve of a bound Run at beta against the model"""
    fr = _frame(name)
    r.set_beta(beta)
    ww = _check_weights(r.weights(), name, sem, beta, seg_mode, pp_max)
    A, b = r.assemble()
    A_ref, b_ref, M = lwm.normal_equations(fr, sem, beta, orc.default_opt(), seg_mode, pp_max, corr)
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    out = r.loss()
    want, Mn = lwm.data_loss(fr, sem, beta, 1.0, seg_mode, pp_max)
    print("data loss", out[0], "want", want, "count", out[3], Mn)
    np.testing.assert_allclose(out[0], want, rtol=1e-8, atol=1e-300)
    assert int(out[3]) == Mn == M == len(ww.t.match)
    A32, b32, _ = _system_rot32(name, sem, beta, seg_mode, pp_max, corr)
    ref = orc.solve_damped(A32, b32, 10.0)
    np.testing.assert_allclose(r.solve(10.0), ref, rtol=0, atol=1e-9 * max(1.0, np.abs(ref).max()))
    return ww, A_ref


# ---- 1. every kernel against the model ----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["hard", "soft", "trunc"])
@pytest.mark.parametrize("K,state_f64", [(1, 1), (4, 0), (4, 1), (6, 0), (6, 1), (8, 1)])
def test_weights_assemble_loss_solve_and_trace_match_the_model(K, state_f64, cfg):
    name, (seg_mode, pp_max) = f"k{K}", CONFIGS[cfg]
    fr, sem, beta = _frame(name), _sem(name), _beta(name)
    r = Run(name, cfg, bool(state_f64))
    ww, A_ref = _check_point(r, name, sem, beta, seg_mode, pp_max)
    r.close()
    share = float((ww.w == 0).mean())
    if cfg != "soft":          # a visible share of the matched surfels weighs nothing
        assert 0.05 < share < 0.95, share
    # an assembly that ignored the weights would miss the JtJ tolerance (1e-7 of the largest entry) a hundred times over
    A0, _, _ = orc.normal_equations(fr, beta, orc.default_opt())
    assert np.abs(A_ref - A0).max() > 1e-5 * np.abs(A0).max()
    r = Run(name, cfg, bool(state_f64))
    (got_beta, recs), = r.run()
    r.close()
    want_beta, trace = _model_trace(name, sem, seg_mode, pp_max)
    _check_trace(recs, got_beta, trace, want_beta)


@pytest.mark.parametrize("cfg", ["hard", "soft", "trunc"])
@pytest.mark.parametrize("name", ["n37", "n65", "n65c1"])
def test_sizes_below_a_wave_a_wave_plus_one_lane_and_one_class(name, cfg):
    seg_mode, pp_max = CONFIGS[cfg]
    sem, beta = _sem(name), _beta(name)
    r = Run(name, cfg)
    _check_point(r, name, sem, beta, seg_mode, pp_max)
    r.bind(0, name)
    (got_beta, recs), = r.run()
    r.close()
    want_beta, trace = _model_trace(name, sem, seg_mode, pp_max)
    _check_trace(recs, got_beta, trace, want_beta)


# ---- 2. edge weights ----------------------------------------------------------------------------------------------------
def _no_data_system(name, beta):
    return orc.normal_equations(_frame(name), beta, orc.default_opt(sf_point_plane=False))


@pytest.mark.parametrize("K", [4, 6])
def test_every_hard_weight_zero(K):
    """sf_seg = (argmax + 1) % C at the point of the pass: the data blocks vanish, M_grad is still the match count"""
    from types import SimpleNamespace
    name = f"k{K}"
    fr, base = _frame(name), _sem(name)
    Cn = base.tgt_seg_conf.shape[1]
    for beta, run in ((_beta(name), False), (np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (fr.J, 1)), True)):
        ww = lwm.weights(fr, base, beta, 1)
        lwm.check_conditions(ww, 1, 0.0)
        seg = base.sf_seg.copy()
        seg[ww.t.match] = (ww.conf.argmax(1) + 1) % Cn
        sem = SimpleNamespace(sf_seg=seg, sf_seg_conf=base.sf_seg_conf, tgt_seg_conf=base.tgt_seg_conf)
        r = Run(name, "hard", sem=sem, num_iterations=1)
        if run:                                   # one iteration from identity: the Jacobian pass ran at this beta
            (_, recs), = r.run()
            assert recs[0]["M_grad"] == len(ww.t.match) > 0.5 * fr.sf_points.shape[0]
        else:
            r.set_beta(beta)
            assert not r.weights().any()
            A, b = r.assemble()
            A_ref, b_ref, _ = _no_data_system(name, beta)
            np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
            np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
            out = r.loss()
            assert out[0] == 0.0 and int(out[3]) == len(ww.t.match)
        r.close()


def test_truncation_that_drops_everything_and_one_that_drops_nothing():
    name = "k6"
    fr, sem, beta = _frame(name), _sem(name), _beta(name)
    M = len(orc.data_term(fr, beta, 1.0).match)
    r = Run(name, (0, 1e-30))
    r.set_beta(beta)
    assert not r.weights().any()
    A, b = r.assemble()
    A_ref, b_ref, _ = _no_data_system(name, beta)
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    out = r.loss()
    assert out[0] == 0.0 and int(out[3]) == M
    r.close()
    outs = []
    for cfg in ((0, 1.0), None):                  # every weight 1 against a solver without the option (K = 6: the same pair form)
        r = Run(name, cfg)
        r.set_beta(beta)
        if cfg:
            w = r.weights()
            assert w.sum() == M and set(np.unique(w)) <= {0.0, 1.0}
        step = r.solve(0.37)
        r.bind(0, name)
        outs.append((step, r.run()[0]))
        r.close()
    np.testing.assert_allclose(outs[0][0], outs[1][0], rtol=0, atol=1e-11)
    np.testing.assert_allclose(outs[0][1][0], outs[1][1][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose([x["loss"] for x in outs[0][1][1]], [x["loss"] for x in outs[1][1][1]], rtol=1e-12)


def test_one_hot_surfel_distributions_with_exact_zeros():
    from types import SimpleNamespace
    name = "k4"
    base, beta = _sem(name), _beta(name)
    Cn = base.sf_seg_conf.shape[1]
    hot = np.zeros_like(base.sf_seg_conf)
    hot[np.arange(len(hot)), base.sf_seg] = 1.0
    hot[::3] = base.sf_seg_conf[::3]              # a third keep their soft distributions
    assert (hot == 0).sum() > len(hot) and Cn == 4
    sem = SimpleNamespace(sf_seg=base.sf_seg, sf_seg_conf=hot, tgt_seg_conf=base.tgt_seg_conf)
    r = Run(name, "soft", sem=sem)
    r.set_beta(beta)
    w = r.weights()
    assert np.isfinite(w).all()
    _check_weights(w, name, sem, beta, 2, 0.0)
    r.bind(0, name, sem)
    (got_beta, recs), = r.run()
    r.close()
    assert np.isfinite(got_beta).all() and all(np.isfinite(x["loss"]) for x in recs)
    want_beta, trace = _model_trace(name, sem, 2, 0.0)
    _check_trace(recs, got_beta, trace, want_beta)


# ---- 3. batches, rebinds, combinations ----------------------------------------------------------------------------------
def test_batch_of_three_slots_and_a_rebound_slot_loses_its_inputs():
    names = ["n37", "k4", "n65"]
    single = {}
    for name in names:
        r = Run(name, "soft")
        single[name] = r.run()[0]
        r.close()
    r = Run(None, "soft", slots=3)
    for i, name in enumerate(names):
        r.bind(i, name)
    out = r.run(3)
    for i, name in enumerate(names):
        np.testing.assert_allclose(out[i][0], single[name][0], rtol=0, atol=1e-9)
        np.testing.assert_allclose([x["loss"] for x in out[i][1]], [x["loss"] for x in single[name][1]], rtol=1e-9)
    r.bind(1, "k4", semantic=False)               # slm_bind_frame clears the slot's semantic inputs
    text = b"slot 1 has no semantic inputs; call slm_bind_data_semantic after slm_bind_frame"
    st = r.e.stream
    w = r.torch.zeros(1200, dtype=r.torch.float64, device=r.dev)
    for fn, args in (("slm_run", (r.h, 3, st)), ("slm_lm_grad_local", (r.h, 3, st)), ("slm_lm_loss_local", (r.h, 3, st)),
                     ("slm_loss", (r.h, 1, w.data_ptr(), st)), ("slm_assemble", (r.h, 1, None, w.data_ptr(), st)),
                     ("slm_solve", (r.h, 1, 1.0, w.data_ptr(), None, st)), ("slm_data_weights", (r.h, 1, w.data_ptr(), st))):
        assert getattr(r.lib, fn)(*args) == UNBOUND, fn
        assert r.lib.slm_last_error() == fn.encode() + b": " + text, r.lib.slm_last_error()
    assert r.lib.slm_run(r.h, 1, st) == 0         # slot 0 alone still has its own
    r.bind(0, "n37")
    r.bind_sem(1, _sem("k4"))
    out = r.run(3)
    r.close()
    for i, name in enumerate(names):
        np.testing.assert_allclose(out[i][0], single[name][0], rtol=0, atol=1e-9)


def test_batch_bound_with_slm_bind_frames_loses_its_inputs():
    from super_amd.engine import DeviceFrame
    r = Run(None, "hard", slots=2)
    r.bind(0, "n37")
    r.bind(1, "n65")
    r.run(2)
    r.e.bind_batch([DeviceFrame.from_scene(_scene(n), r.dev, state_f64=True) for n in ("n37", "n65")])
    assert r.lib.slm_run(r.h, 2, r.e.stream) == UNBOUND
    assert r.lib.slm_last_error() == b"slm_run: slot 0 has no semantic inputs; call slm_bind_data_semantic after slm_bind_frame"
    r.close()


@pytest.mark.parametrize("cfg", ["hard", "trunc"])
def test_combined_with_the_correspondence_term(cfg):
    from super_amd import synth
    name, lam = "k6", 0.5
    seg_mode, pp_max = CONFIGS[cfg]
    sc, fr, sem, beta = _scene(name), _frame(name), _sem(name), _beta(name)
    tg = _cached(("targets", name), lambda: lcm.targets_from_flow(fr, synth.smooth_flow(sc.H, sc.W, 26, amp=(2.0, 1.5))))
    assert 0.5 * len(tg[2]) < tg[2].sum() < len(tg[2])
    corr = (tg, 2, lam)
    r = Run(name, cfg, corr=(2, lam))
    r.bind_points(tg)
    _check_point(r, name, sem, beta, seg_mode, pp_max, corr)
    r.bind(0, name)
    r.bind_points(tg)
    (got_beta, recs), = r.run()
    r.close()
    want_beta, trace = _model_trace(name, sem, seg_mode, pp_max, corr)
    _check_trace(recs, got_beta, trace, want_beta)


@pytest.mark.parametrize("cfg,K", [("hard", 4), ("soft", 6), ("trunc", 4)])
def test_sharded_protocol_at_world_one_equals_slm_run(cfg, K):
    name = f"k{K}"
    r = Run(name, cfg)
    (want_beta, want_recs), = r.run()
    r.close()
    r = Run(name, cfg, shard=True)
    (beta, recs), = r.run_sharded()
    r.close()
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=1e-9)
    np.testing.assert_allclose([x["loss"] for x in recs], [x["loss"] for x in want_recs], rtol=1e-9)
    assert [x["M_grad"] for x in recs] == [x["M_grad"] for x in want_recs]
    assert [x["accepted"] for x in recs] == [x["accepted"] for x in want_recs]


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------
def _refused(lib, name, args, code, text):
    rc = getattr(lib, name)(*args)
    got = lib.slm_last_error()
    print(name, rc, got)
    assert rc == code, (name, rc, got)
    assert got == text, (name, got)


def test_refusal_texts():
    import torch
    from super_amd import _lib
    from super_amd.engine import DeviceFrame, Engine
    INVALID, UNSUPPORTED = 1, 5
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    sc = _scene("n65")
    fr = DeviceFrame.from_scene(sc, dev, state_f64=True)
    pre = b"slm_enable_data_weights: "
    for kw, text in ((dict(data_path=1), b"needs the pair-record data path (data_path 0 or 2)"),
                     (dict(solver_path=1), b"needs a nested-dissection solver_path (0, 2, 3 or 4)"),
                     (dict(use_data=False), b"needs the data term (use_data 1)")):
        e = Engine(dev, **kw)
        _refused(lib, "slm_enable_data_weights", (e.h, 1, 0.0), UNSUPPORTED, pre + text)
        e.close()
    _refused(lib, "slm_enable_data_weights", (None, 1, 0.0), INVALID, pre + b"null argument")
    e = Engine(dev, max_frames=2)
    for m in (3, -1):
        _refused(lib, "slm_enable_data_weights", (e.h, m, 0.0), INVALID, pre + b"seg_mode must be 0 (none), 1 (hard) or 2 (soft)")
    for p in (-1e-9, float("nan"), float("inf")):
        _refused(lib, "slm_enable_data_weights", (e.h, 0, p), INVALID, pre + b"pp_max must be finite and >= 0")
    sem = _sem("n65")
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt)
    seg, scf, tcf = t(sem.sf_seg, torch.int32), t(sem.sf_seg_conf, torch.float32), t(sem.tgt_seg_conf, torch.float32)
    w = torch.zeros(sc.N, dtype=torch.float64, device=dev)
    sem_args = lambda slot, Cn=3: (e.h, slot, Cn, seg.data_ptr(), scf.data_ptr(), tcf.data_ptr(), None)
    # before slm_enable_data_weights, and after it was switched off again
    assert lib.slm_enable_data_weights(e.h, 2, 0.0) == 0 and lib.slm_enable_data_weights(e.h, 0, 0.0) == 0
    _refused(lib, "slm_bind_data_semantic", sem_args(0), UNSUPPORTED, b"slm_bind_data_semantic: slm_enable_data_weights first")
    _refused(lib, "slm_data_weights", (e.h, 0, w.data_ptr(), None), UNSUPPORTED, b"slm_data_weights: slm_enable_data_weights first")
    assert lib.slm_enable_data_weights(e.h, 1, 0.0) == 0, lib.slm_last_error()
    assert lib.slm_enable_corr(e.h, 2, 0.5) == 0, lib.slm_last_error()          # the two options combine
    _refused(lib, "slm_bind_data_semantic", sem_args(2), INVALID, b"slm_bind_data_semantic: bad slot")
    _refused(lib, "slm_data_weights", (e.h, -1, w.data_ptr(), None), INVALID, b"slm_data_weights: bad slot")
    _refused(lib, "slm_bind_data_semantic", (e.h, 0, 3, None, scf.data_ptr(), tcf.data_ptr(), None), INVALID,
             b"slm_bind_data_semantic: null argument")
    _refused(lib, "slm_data_weights", (e.h, 0, None, None), INVALID, b"slm_data_weights: null argument")
    _refused(lib, "slm_bind_data_semantic", sem_args(0), UNBOUND, b"slm_bind_data_semantic: slm_bind_frame first")
    _refused(lib, "slm_data_weights", (e.h, 0, w.data_ptr(), None), UNBOUND, b"slm_data_weights: slm_bind_frame first")
    cs = fr.c_struct()
    cs.J = 65536
    e2 = Engine(dev)
    assert lib.slm_enable_data_weights(e2.h, 0, PP) == 0
    _refused(lib, "slm_bind_frame", (e2.h, 0, C.byref(cs), None), UNSUPPORTED,
             b"slm_bind_frame: the data weights (slm_enable_data_weights) need J < 65536")
    e2.close()
    e.bind(0, fr)
    for Cn in (0, 5):
        _refused(lib, "slm_bind_data_semantic", sem_args(0, Cn), UNSUPPORTED,
                 b"slm_bind_data_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)")
    _refused(lib, "slm_run", (e.h, 1, None), UNBOUND,
             b"slm_run: slot 0 has no semantic inputs; call slm_bind_data_semantic after slm_bind_frame")
    for args in ((e.h, 2, 0.0), (e.h, 0, 0.0)):
        _refused(lib, "slm_enable_data_weights", args, INVALID,
                 pre + b"a slot is already bound; call it after slm_create and before the first bind")
    assert lib.slm_bind_data_semantic(*sem_args(0)) == 0, lib.slm_last_error()
    assert lib.slm_data_weights(e.h, 0, w.data_ptr(), None) == 0, lib.slm_last_error()
    assert lib.slm_run(e.h, 1, None) == 0, lib.slm_last_error()
    torch.cuda.synchronize()
    assert 0 < float(w.sum()) < sc.N
    e.close()
    # allowed on a sharded solver, in either order
    for first in ("shard", "weights"):
        e = Engine(dev)
        if first == "shard":
            assert lib.slm_set_shard(e.h, 0, 1) == 0 and lib.slm_enable_data_weights(e.h, 2, 0.0) == 0, lib.slm_last_error()
        else:
            assert lib.slm_enable_data_weights(e.h, 2, 0.0) == 0 and lib.slm_set_shard(e.h, 0, 1) == 0, lib.slm_last_error()
        e.close()


# ---- 5. Python surface ------------------------------------------------------------------------------------------------------
def _sem_frame(name, sem=None):
    import torch
    sc, sem = _scene(name), sem or _sem(name)
    sf, inputs, new_data = torch_frame(sc)
    sf.seg = torch.from_numpy(sem.sf_seg).cuda()
    sf.seg_conf = torch.from_numpy(sem.sf_seg_conf).cuda()
    new_data.seg_conf = torch.from_numpy(sem.tgt_seg_conf).cuda()
    return sf, inputs, new_data


def _opt(K, **kw):
    opt = ref_opt(orc.default_opt())
    opt.num_neighbors = K
    for k, v in kw.items():
        setattr(opt, k, v)
    return opt


@pytest.mark.parametrize("cfg", ["hard", "soft", "trunc"])
def test_python_surface_returns_the_c_abi_runs(cfg):
    import torch
    from super_amd.LM import LM_Solver
    seg_mode, pp_max = CONFIGS[cfg]
    # soft wins over hard; the truncation comes from the depth model and is ignored with a semantic weight
    kw = {"hard": dict(sf_hard_seg_point_plane=True, depth_model="raft_stereo"),
          "soft": dict(sf_hard_seg_point_plane=True, sf_soft_seg_point_plane=True), "trunc": dict(depth_model="raft_stereo")}[cfg]
    names = ["k4", "n65", "n37"]
    want = {}
    for name in names:
        r = Run(name, cfg)
        want[name] = r.run()[0]
        r.close()
    lm = LM_Solver(_opt(4, **kw), weighted_data=True)
    assert (lm.seg_mode, lm.pp_max) == (seg_mode, PP if cfg != "soft" else 0.0)
    beta = lm.LM(*_sem_frame("k4")).cpu().numpy()
    np.testing.assert_allclose(beta, want["k4"][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose([x["loss"] for x in lm.last_records[0]], [x["loss"] for x in want["k4"][1]], rtol=1e-9)
    # prepareCostTerm and data_weights at a given beta
    fr, sem, b0 = _frame("k4"), _sem("k4"), _beta("k4")
    bt = torch.from_numpy(b0).cuda()
    sf, inputs, new_data = _sem_frame("k4")
    total = float(lm.prepareCostTerm(sf, inputs, new_data, bt))
    np.testing.assert_allclose(total, lwm.total_loss(fr, sem, b0, orc.default_opt(), seg_mode, pp_max)[0], rtol=1e-8)
    _check_weights(lm.data_weights(0).cpu().numpy(), "k4", sem, b0, seg_mode, pp_max)
    jtj, jtl = lm.prepareCostTerm(sf, inputs, new_data, bt, grad=True)
    A_ref, b_ref, _ = lwm.normal_equations(fr, sem, b0, orc.default_opt(), seg_mode, pp_max)
    np.testing.assert_allclose(jtl.cpu().numpy().reshape(-1), b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(jtj.cpu().numpy(), A_ref, rtol=0, atol=1e-7 * max(1.0, np.abs(A_ref).max()))
    # a batch
    lmb = LM_Solver(_opt(4, **kw), max_frames=3, weighted_data=True)
    betas = lmb.LM_batch([_sem_frame(n) for n in names])
    for b, n in zip(betas, names):
        np.testing.assert_allclose(b.cpu().numpy(), want[n][0], rtol=0, atol=1e-9)
    # without the flag the options are ignored: the default solver's run
    r = Run("k4", None)
    plain = r.run()[0][0]
    r.close()
    np.testing.assert_allclose(LM_Solver(_opt(4, **kw)).LM(*_sem_frame("k4")).cpu().numpy(), plain, rtol=0, atol=1e-9)
    assert np.abs(plain - want["k4"][0]).max() > 1e-6


def test_python_value_errors_name_the_field():
    import torch
    from super_amd.LM import LM_Solver
    lm = LM_Solver(_opt(4, sf_soft_seg_point_plane=True), weighted_data=True, max_frames=2)
    for field, owner, attr in (("sf.seg", 0, "seg"), ("sf.seg_conf", 0, "seg_conf"), ("new_data.seg_conf", 2, "seg_conf")):
        fr = _sem_frame("n65")
        delattr(fr[owner], attr)
        with pytest.raises(ValueError, match=field.replace(".", r"\.") + " is missing"):
            lm.LM(*fr)
        with pytest.raises(ValueError, match=field.replace(".", r"\.") + " is missing"):
            lm.prepareCostTerm(*fr, torch.from_numpy(_beta("n65")).cuda())
        with pytest.raises(ValueError, match=field.replace(".", r"\.") + " is missing"):
            lm.LM_batch([_sem_frame("n37"), fr])
    fr = _sem_frame("n65")
    fr[0].seg = fr[0].seg[:-1]
    with pytest.raises(ValueError, match=r"sf\.seg must be"):
        lm.LM(*fr)
    fr = _sem_frame("n65")
    fr[0].seg_conf = fr[0].seg_conf[:, :2]
    with pytest.raises(ValueError, match=r"new_data\.seg_conf must be"):
        lm.LM(*fr)
    fr = _sem_frame("n65")
    fr[0].seg_conf = torch.cat([fr[0].seg_conf, fr[0].seg_conf], 1)          # six classes
    with pytest.raises(ValueError, match=r"sf\.seg_conf must be"):
        lm.LM(*fr)
    fr = _sem_frame("n65")
    fr[2].seg_conf = fr[2].seg_conf[:-1]
    with pytest.raises(ValueError, match=r"new_data\.seg_conf must be"):
        lm.LM(*fr)
