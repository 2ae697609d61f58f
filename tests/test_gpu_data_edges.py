"""Every device form of the point-to-plane term's match set on the edge fixture of tests/data_edge_cases.py, against the
oracle (which tests/test_data_edge_cases.py pins against the reference's own run).  Needs an MI355X (-m gpu).

Forms: the row-table form (``slm_data_residuals``: ``k_data_resid``), the per-pixel form of the LM loop at num_neighbors 4
(``k_data_eval``, PX: the rounded pixel's validity is read from the tap that IS that pixel), the per-entry form
(data_path 1), the pair-record forms (num_neighbors != 4, and 4 once ``slm_enable_corr`` is on), in float64 and float32
state.  Tolerances are those of tests/test_gpu_parity.py for the same quantities: residuals ``TOL_F64``, jtl 1e-8, JtJ 1e-7
of its largest entry, loss 1e-6 relative, final beta 1e-4; a batch against single frames 1e-7.

The exactly-integer groups (defect D4) have Jacobian rows a thousand times the others' (both coinciding taps carry
d/du = +1, so the "derivative" is twice the pixel's point times fx / Z): at the identity warp they set max|JtJ|, and the
tolerance that follows from it, 1.7, would hide a missing ordinary surfel.  So the identity system is assembled twice, on
the whole scene (where the D4 groups must be visible) and without the D4 groups (where every other group must be); at
``generic_beta`` nothing is exact and one assembly shows them all.

Where device and oracle may legitimately differ: a surfel within 1e-9 px of a decision boundary (``tie_distance``).  At
identity in float64 state the hand-placed surfels sit ON boundaries, but T == p bit for bit on both sides, so nothing is
excluded there."""
import numpy as np
import pytest

import data_edge_cases as dec
from oracle import lm_oracle as orc
from test_gpu_parity import TOL_BETA, TOL_F64

pytestmark = [pytest.mark.gpu, pytest.mark.filterwarnings("ignore::RuntimeWarning")]

DATA_ONLY = orc.default_opt(mesh_arap=False, mesh_rot=False)
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _scene(K, state_f64, variant="full", n_base=dec.N_BASE):
    """the scene as the device binds it and as the oracle reads it: float32 state rounds both"""
    def make():
        sc = dec.edge_scene(K, n_base)
        if variant == "no_d4":
            sc = dec.subset(sc, dec.without_groups(sc, dec.D4_GROUPS))
        return sc if state_f64 else dec.state32(sc)
    return _cached(("scene", K, bool(state_f64), variant, n_base), make)


def _frame(K, state_f64, variant="full"):
    return _cached(("frame", K, bool(state_f64), variant), lambda: orc.Frame.from_scene(_scene(K, state_f64, variant)))


def _beta(tag):
    return dec.identity() if tag == "id" else dec.generic_beta()


def _excluded(fr, beta, tag, state_f64):
    """surfels a rounding-level difference in T may put on either side of a boundary; none at identity in float64 state"""
    if tag == "id" and state_f64:
        return np.zeros(len(fr.sf_points), bool)
    return dec.tie_distance(fr, beta) <= 1e-9


def _mask(match, N):
    m = np.zeros(N, bool)
    m[match] = True
    return m


class Dev:
    """an Engine with one scene bound per slot"""

    def __init__(self, scenes, state_f64, corr=None, **kw):
        import torch
        from super_amd import _lib
        from super_amd.engine import DeviceFrame, Engine
        self.torch, self._lib = torch, _lib
        self.dev = torch.device("cuda", 0)
        self.e = Engine(self.dev, max_frames=len(scenes), **kw)
        self.lib, self.h = self.e.lib, self.e.h
        if corr:
            _lib.check(self.lib.slm_enable_corr(self.h, corr[0], corr[1]), "slm_enable_corr")
        self.state_f64 = bool(state_f64)
        self.frames = []
        for i, sc in enumerate(scenes):
            self.bind(i, sc)

    def bind(self, slot, sc):
        from super_amd.engine import DeviceFrame
        fr = DeviceFrame.from_scene(sc, self.dev, state_f64=self.state_f64)
        self.frames.append(fr)          # (kept alive: no two binds of a test see the same device pointers)
        self.e.bind(slot, fr)

    def set_beta(self, beta, slot=0):
        b = self.torch.from_numpy(np.ascontiguousarray(beta)).to(self.dev)
        self._lib.check(self.lib.slm_set_beta(self.h, slot, b.data_ptr(), self.e.stream), "slm_set_beta")

    def residuals(self, slot=0):
        t, N = self.torch, self.e._frames[slot].N
        r = t.empty(N, dtype=t.float64, device=self.dev)
        m = t.empty(N, dtype=t.uint8, device=self.dev)
        taps = t.empty((N, 4), dtype=t.int32, device=self.dev)
        self._lib.check(self.lib.slm_data_residuals(self.h, slot, r.data_ptr(), m.data_ptr(), taps.data_ptr(), self.e.stream),
                        "slm_data_residuals")
        return r.cpu().numpy(), m.cpu().numpy().astype(bool), taps.cpu().numpy()

    def assemble(self, slot=0):
        t, P = self.torch, 7 * self.e._frames[slot].J
        A = t.empty((P, P), dtype=t.float64, device=self.dev)
        b = t.empty(P, dtype=t.float64, device=self.dev)
        self._lib.check(self.lib.slm_assemble(self.h, slot, A.data_ptr(), b.data_ptr(), self.e.stream), "slm_assemble")
        return A.cpu().numpy(), b.cpu().numpy()

    def loss(self, slot=0):
        out = self.torch.empty(4, dtype=self.torch.float64, device=self.dev)
        self._lib.check(self.lib.slm_loss(self.h, slot, out.data_ptr(), self.e.stream), "slm_loss")
        o = out.cpu().numpy()
        return float(o[0]), int(o[3])

    def solve(self, u, slot=0):
        t, P = self.torch, 7 * self.e._frames[slot].J
        d = t.zeros(P, dtype=t.float64, device=self.dev)
        st = t.zeros(1, dtype=t.int32, device=self.dev)
        self._lib.check(self.lib.slm_solve(self.h, slot, u, d.data_ptr(), st.data_ptr(), self.e.stream), "slm_solve")
        assert int(st.item()) == 0
        return d.cpu().numpy()

    def run(self, n=1):
        self.e.run(n)
        return [(self.e.beta(i).cpu().numpy(), self.e.records(i)) for i in range(n)]

    def close(self):
        self.e.close()


# ---- 1. the row-table form ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("state_f64", [0, 1])
@pytest.mark.parametrize("K", dec.KS)
def test_row_table_form_match_set_taps_and_residuals(K, state_f64):
    fr = _frame(K, state_f64)
    N = len(fr.sf_points)
    d = Dev([_scene(K, state_f64)], state_f64)
    for tag in ("id", "gen"):
        beta = _beta(tag)
        d.set_beta(beta)
        r, m, taps = d.residuals()
        t = orc.data_term(fr, beta, 1.0)
        want = _mask(t.match, N)
        ex = _excluded(fr, beta, tag, state_f64)
        print(K, state_f64, tag, "matched", int(m.sum()), "oracle", int(want.sum()), "excluded", int(ex.sum()))
        assert ex.mean() <= 0.01
        for name, ix in dec.GROUPS.items():             # per group, so that a failure names its edge
            np.testing.assert_array_equal(m[ix][~ex[ix]], want[ix][~ex[ix]], err_msg=f"{name} at {tag}")
        np.testing.assert_array_equal(m[~ex], want[~ex])
        if tag == "id" and state_f64:
            np.testing.assert_array_equal(m[:dec.N_GROUPS], dec.EXPECT)
        both = np.nonzero(m & want & ~ex)[0]
        pos = np.searchsorted(t.match, both)
        np.testing.assert_array_equal(taps[both], t.taps[pos])                          # tap rows bit-exact
        np.testing.assert_allclose(r[both], t.r[pos], rtol=0, atol=TOL_F64)
        for name, ix in dec.GROUPS.items():
            sel = np.intersect1d(ix, both)
            np.testing.assert_allclose(r[sel], t.r[np.searchsorted(t.match, sel)], rtol=0, atol=TOL_F64, err_msg=f"{name} at {tag}")
        assert not r[~m].any()
    d.close()


# ---- 2. the Jacobian pass and the loss: per-pixel form (K = 4, data_path 0 / 2), per-entry form (1), pair records --------
def _oracle_system(K, state_f64, variant, tag):
    def make():
        fr, beta = _frame(K, state_f64, variant), _beta(tag)
        A, b, M = orc.normal_equations(fr, beta, DATA_ONLY)
        loss, Ml = orc.total_loss(fr, beta, DATA_ONLY)
        assert M == Ml
        sc = _scene(K, state_f64, variant)
        m = _mask(orc.data_term(fr, beta, 1.0).match, sc.N)
        moves = {}
        if variant == "full":
            groups = dec.GROUPS
        else:       # the D4 groups are the first surfels: the others moved down by their count
            shift = sum(len(dec.GROUPS[n]) for n in dec.D4_GROUPS)
            groups = {n: ix - shift for n, ix in dec.GROUPS.items() if n not in dec.D4_GROUPS}
        for name, ix in groups.items():
            if m[ix].any():
                rest = orc.Frame.from_scene(dec.subset(sc, np.setdiff1d(np.arange(sc.N), ix)))
                moves[name] = np.abs(A - orc.normal_equations(rest, beta, DATA_ONLY)[0]).max()
        return A, b, M, loss, moves, float(dec.tie_distance(fr, beta).min())
    return _cached(("system", K, bool(state_f64), variant, tag), make)


CASES = (("full", "id"), ("no_d4", "id"), ("full", "gen"))


def _check_system(d, K, state_f64, variant, tag):
    A_ref, b_ref, M, loss_ref, moves, tie = _oracle_system(K, state_f64, variant, tag)
    assert (tag == "id" and state_f64) or tie > 1e-9          # else no surfel of this case may sit on a boundary
    d.set_beta(_beta(tag))
    A, b = d.assemble()
    loss, count = d.loss()
    tol = 1e-7 * max(1.0, np.abs(A_ref).max())
    print(K, state_f64, variant, tag, "M", count, M, "max|JtJ|", np.abs(A_ref).max(), "err", np.abs(A - A_ref).max(),
          "jtl err", np.abs(b - b_ref).max(), "loss", loss, loss_ref, {n: float("%.3g" % v) for n, v in moves.items()})
    # a missed (or an extra) surfel of any matching group would show: its rows move JtJ by more than ten tolerances
    want_visible = set(dec.D4_GROUPS) if (variant, tag) == ("full", "id") else set(moves)
    if (variant, tag) == ("no_d4", "id"):
        assert want_visible == {n for n, c in dec.CLASSES.items() if c != "dropped" and n not in dec.D4_GROUPS}
    for name in want_visible:
        assert moves[name] > 10 * tol, (name, moves[name], tol)
    assert count == M
    np.testing.assert_allclose(loss, loss_ref, rtol=1e-6)
    np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
    np.testing.assert_allclose(A, A_ref, rtol=0, atol=tol)


@pytest.mark.parametrize("state_f64", [0, 1])
@pytest.mark.parametrize("data_path", [0, 1, 2])
@pytest.mark.parametrize("K", dec.KS)
def test_assemble_and_loss_on_every_data_path(K, data_path, state_f64):
    for variant, tag in CASES:
        d = Dev([_scene(K, state_f64, variant)], state_f64, use_arap=False, use_rot=False, data_path=data_path)
        _check_system(d, K, state_f64, variant, tag)
        d.close()


# ---- 3. the counts of the first LM iteration, and the tap the rounded pixel's validity is read from ---------------------
def _first_iteration(fr):
    trace = []
    orc.lm(fr, orc.default_opt(num_optimize_iterations=1), trace=trace)
    assert dec.tie_distance(fr, dec.identity() + trace[0]["delta"]).min() > 1e-9
    return trace[0]["M_grad"], trace[0]["M_loss"]


@pytest.mark.parametrize("state_f64", [0, 1])
@pytest.mark.parametrize("K", [4, 6])
def test_counts_of_the_first_iteration(K, state_f64):
    fr = _frame(K, state_f64)
    assert state_f64 or dec.tie_distance(fr, dec.identity()).min() > 1e-9
    d = Dev([_scene(K, state_f64)], state_f64, num_iterations=1, data_path=0)
    (_, recs), = d.run()
    d.close()
    want = _cached(("first", K, bool(state_f64)), lambda: _first_iteration(fr))
    print(recs[0], want)
    assert recs[0]["status"] == 0 and (recs[0]["M_grad"], recs[0]["M_loss"]) == want


@pytest.mark.parametrize("kind", ["hole", "invalid_only"])
def test_one_pixel_flipped_around_a_half_integer_surfel(kind):
    """``valid`` (and ``index_map``) flipped at each of the four pixels around the clean ``half_even`` and ``half_odd``
    surfel: the per-pixel form (``tr``: which tap is the rounded pixel) and the row-table form follow the oracle.  With
    ``valid`` alone cleared only ONE of the four flips drops the surfel -- the floor tap for even k, the ceil tap for odd."""
    sc = dec.edge_scene(4)
    frames = dec.flipped_frames(sc) if kind == "hole" else dec.invalid_only_frames(sc)
    assert len(frames) == 8
    d = Dev([sc], True, num_iterations=1, data_path=0)
    kept = []
    for label, fl in frames:
        i = dec.GROUPS[label.split("@")[0]][0]
        fr = orc.Frame.from_scene(fl)
        want = _mask(orc.data_term(fr, dec.identity(), 1.0).match, sc.N)
        d.bind(0, fl)
        d.set_beta(dec.identity())
        _, m, _ = d.residuals()                         # row-table form at identity
        (_, recs), = d.run()                            # per-pixel form: the count of the first Jacobian pass
        print(label, "surfel", i, "matched", bool(m[i]), "oracle", bool(want[i]), recs[0]["M_grad"], int(want.sum()))
        np.testing.assert_array_equal(m, want, err_msg=label)
        assert recs[0]["M_grad"] == int(want.sum()), label
        assert recs[0]["M_loss"] == _first_iteration(fr)[1], label
        kept.append(bool(m[i]))
    d.close()
    assert kept == ([False] * 8 if kind == "hole" else [False, True, True, True, True, False, True, True])


# ---- 4. the pair-record form at num_neighbors 4 -------------------------------------------------------------------------
@pytest.mark.parametrize("state_f64", [0, 1])
def test_pair_record_form_at_k4(state_f64):
    """a solver with ``slm_enable_corr`` and no correspondences bound takes the pair-record form at K = 4: the same system,
    the same counts, and the step of the default form"""
    K, corr = 4, (1, 0.5)
    for variant, tag in CASES:
        d = Dev([_scene(K, state_f64, variant)], state_f64, corr=corr, use_arap=False, use_rot=False)
        _check_system(d, K, state_f64, variant, tag)
        d.close()
    fr = _frame(K, state_f64)
    want = _cached(("first", K, bool(state_f64)), lambda: _first_iteration(fr))
    steps = []
    for c in (corr, None):
        d = Dev([_scene(K, state_f64)], state_f64, corr=c, num_iterations=1)
        d.set_beta(_beta("gen"))
        steps.append(d.solve(0.37))
        d.bind(0, _scene(K, state_f64))
        (_, recs), = d.run()
        d.close()
        assert (recs[0]["M_grad"], recs[0]["M_loss"]) == want, c
    print("step difference", np.abs(steps[0] - steps[1]).max(), "of", np.abs(steps[1]).max())
    np.testing.assert_allclose(steps[0], steps[1], rtol=0, atol=1e-11)


# ---- 5. ten LM iterations from identity, the full default terms ---------------------------------------------------------
def _oracle_trace(K, state_f64):
    def make():
        fr = _frame(K, state_f64)
        trace = []
        beta = orc.lm(fr, orc.default_opt(), trace=trace)
        cur, ok_grad, ok_loss = dec.identity(), [], []
        for t in trace:
            at_identity = state_f64 and np.array_equal(cur, dec.identity())       # exact there: never excluded
            ok_grad.append(bool(at_identity or dec.tie_distance(fr, cur).min() > 1e-9))
            ok_loss.append(bool(dec.tie_distance(fr, cur + t["delta"]).min() > 1e-9))
            cur = t["beta"]
        return beta, trace, ok_grad, ok_loss
    return _cached(("trace", K, bool(state_f64)), make)


@pytest.mark.parametrize("state_f64", [0, 1])
@pytest.mark.parametrize("K", [4, 6])
def test_ten_iterations_from_identity(K, state_f64):
    want_beta, trace, ok_grad, ok_loss = _oracle_trace(K, state_f64)
    acc = [t["accepted"] for t in trace]
    assert len(trace) == 10 and False in acc[:-1]            # a rejected step that another iteration follows: the reuse path
    assert sum(a and b for a, b in zip(ok_grad, ok_loss)) >= 8
    d = Dev([_scene(K, state_f64)], state_f64)
    (beta, recs), = d.run()
    d.close()
    loss, want = np.array([r["loss"] for r in recs]), np.array([t["loss"] for t in trace])
    print("loss", loss, "\nwant", want, "\nM_grad", [r["M_grad"] for r in recs], [t["M_grad"] for t in trace],
          "\nM_loss", [r["M_loss"] for r in recs], [t["M_loss"] for t in trace], "\nbeta err", np.abs(beta - want_beta).max())
    assert all(r["status"] == 0 for r in recs)
    for i, (r, t) in enumerate(zip(recs, trace)):
        if ok_grad[i]:
            assert r["M_grad"] == t["M_grad"], i
        if ok_loss[i]:
            assert r["M_loss"] == t["M_loss"], i
    np.testing.assert_allclose(loss, want, rtol=1e-6)
    best = np.minimum.accumulate(np.concatenate([[1e10], want]))[:-1]
    decisive = np.abs(want - best) > 1e-9 * np.abs(best)       # tests/test_gpu_parity.py: no rounding-level accept decision
    np.testing.assert_array_equal(np.array([r["accepted"] for r in recs])[decisive], np.array(acc)[decisive])
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=TOL_BETA)


# ---- 6. a batch ---------------------------------------------------------------------------------------------------------
def test_batch_of_three_sizes_equals_the_single_frames():
    scenes = [dec.edge_scene(4, n) for n in (600, 450, 300)]
    single = []
    for sc in scenes:
        d = Dev([sc], True)
        single.append(d.run()[0])
        d.close()
    d = Dev(scenes, True)
    batch = d.run(3)
    d.close()
    for (b, r), (b1, r1) in zip(batch, single):
        print("batch - single", np.abs(b - b1).max())
        np.testing.assert_allclose(b, b1, rtol=0, atol=1e-7)
        assert [x["M_grad"] for x in r] == [x["M_grad"] for x in r1] and [x["M_loss"] for x in r] == [x["M_loss"] for x in r1]
        assert [x["accepted"] for x in r] == [x["accepted"] for x in r1]
    assert len({len(s.sf_points) for s in scenes}) == 3
