"""Surfel-sharded GraphFit (slm_gf_set_shard and the stepwise entry points of slm_gf.hip, slm_sem.hip) at world 2, 3 and 4 with
every loss term, against the PyTorch-CPU oracle (oracle/graphfit_oracle.py).  Needs ONE MI355X (-m gpu).

The ranks are emulated on one device: W handles ``GraphFit(opt, rank=r, world=W)`` bound to the same frame and driven in
lock-step through the public stepwise surface (bind, eval_morph, eval_losses, step, get_partial, set_partial), the all-reduce
being ``torch.stack(partials).sum(0)`` set back into every handle -- behind pass 1 only with the morphing term, as
GraphFit._iterate has it (test_gpu_dist_procgroup.py runs _iterate itself under a process group).

  A  one evaluation away from identity: the exchanged gradient and terms against autograd on the oracle, every rank's own
     partial against the oracle on its shard; a rank other than 0 adds exactly nothing to the node terms and to the rows its
     surfels do not touch, an empty shard adds exactly nothing
  B  ten steps: every rank against the oracle, the ranks bitwise equal; the difference to an unsharded run is printed
  C  the terms every rank reports after each of the first three steps, counts exact
  D  empty shards (N = 3 at world 4) and a frame without surfels (N = 0 at world 2)
  E  a handle sharded again: unbound until the frame is bound again, then the bits of a fresh handle

The cases and the per-shard references are in gf_shard_cases.py (test_gf_shard_cases.py pins them on the CPU), the tolerances
are gf_shape_cases.py's: terms rtol 1e-9, gradient atol 1e-9 max(1, max|g_ref|), deform_verts after ten steps
min(1e-9, 1e-6 step).  Every test prints the largest error it measured (pytest -s).

The flow-correspondence loss is held to the same rtol 1e-9 as every other term.  It met it only once gf_flow_sample
(slm_gf_sample.h) spelt its float32 arithmetic out with fmaf as F.grid_sample's CPU kernel fuses it: before, the compiler fused
the sample position and the blend of one channel only, and the point-point loss of corr-N3000-J48-K4-flow was 1.84e-9 off the
oracle's in A and 1.68e-9 in C at every world, sharded or not; now 6e-16 and 4e-16."""
import functools

import numpy as np
import pytest

import gf_shape_cases as cases
import gf_shard_cases as shard

pytestmark = pytest.mark.gpu

_id = lambda c: c.id    # noqa: E731
UNBOUND = 4
NT = shard.NTERMS


def _opt(sc):
    o = cases.opt_of(sc.case.tag)
    if sc.state is not None:
        o.slm_state_dtype = sc.state
    return o


class Ranks:
    """``world`` emulated ranks of one frame on one device."""

    def __init__(self, sc, ranks=None):
        import torch
        from super_amd import _lib
        from super_amd.deform_mesh import GraphFit
        assert _lib.GF_NTERMS == NT
        self.torch, self._lib = torch, _lib
        self.case, self.world = sc.case, sc.world
        self.models = cases.FlowModels()
        self.frame = cases.case_frame(sc.case, self.models)
        self.opt = _opt(sc)
        self.gfs = [GraphFit(self.opt, rank=r, world=sc.world, all_reduce=lambda t: None)
                    for r in (range(sc.world) if ranks is None else ranks)]
        for gf in self.gfs:
            self.bind(gf)
        self.n = (sc.case.J + 1) * 7
        self.morph = bool(self.gfs[0].cfg.use_bn_morph)

    def bind(self, gf):
        gf.bind(*self.frame, self.models)

    def set_dv(self, dv):
        """``dv`` into every handle: slm_gf_loss_grad with null outputs (allowed on every sharded handle)."""
        from super_amd.LM import _dev_ptr
        t = self.torch.from_numpy(np.array(dv)).cuda()
        for gf in self.gfs:
            self._lib.check(gf.lib.slm_gf_loss_grad(gf.h, 0, _dev_ptr(t), None, None, gf._st()), "slm_gf_loss_grad")
        self.torch.cuda.synchronize()

    def partials(self):
        return [gf.get_partial(self.torch.empty(self.n + NT, dtype=self.torch.float64, device="cuda")) for gf in self.gfs]

    def exchange(self):
        """The all-reduce: the sum of the ranks' partial states, set back into every rank; returns (partials, sum)."""
        bufs = self.partials()
        total = self.torch.stack(bufs).sum(0)
        for gf in self.gfs:
            gf.set_partial(total)
        return bufs, total

    def evaluate(self):
        """One evaluation as GraphFit._iterate exchanges it; returns (every rank's partial behind pass 2, their sum)."""
        for gf in self.gfs:
            gf.eval_morph()
        if self.morph:
            self.exchange()
        for gf in self.gfs:
            gf.eval_losses()
        return self.exchange()

    def step(self):
        for gf in self.gfs:
            gf.step()

    def dvs(self):
        return [gf.deform_verts().cpu().numpy() for gf in self.gfs]

    def terms(self):
        return [p[self.n:].cpu().numpy() for p in self.partials()]


def _split(buf, case):
    a = buf.cpu().numpy()
    return a[:-NT].reshape(case.J + 1, 7).copy(), a[-NT:].copy()


def _check_terms(got, want, what, late):
    """The SLM_GF_NTERMS entries: the counts exact, asserted here; the losses as the project checks them everywhere
    (test_gpu_graphfit.py, test_gpu_graphfit_shapes.py): rtol 1e-9 with the floor atol 1e-15 -- a node term near identity is
    a sum of squares of differences of nearly equal numbers ((1 - |q|^2)^2 ~ 1e-13, (area - area0)^2 ~ 1e-18) that float64
    itself, the oracle's too, holds to about 1e-9 relative and no better.  A loss outside the bound goes to ``late``, which
    the caller asserts empty at its end, behind every other check.  Returns the largest relative error of a loss above the
    floor."""
    rel = 0.0
    for k in shard.COUNTS:
        assert got[k] == want[k], f"{what}: terms[{k}] = {got[k]!r}, the oracle has {want[k]!r}; all terms {got.tolist()}"
    for k in range(NT):
        if k in shard.COUNTS or (got[k] != got[k] and want[k] != want[k]):      # (NaN on both sides: an empty mean)
            continue
        err = abs(got[k] - want[k])
        if abs(want[k]) > 1e-6:
            rel = max(rel, err / abs(want[k]))
        if not err <= 1e-15 + 1e-9 * abs(want[k]):
            late.append(f"{what}: terms[{k}] = {got[k]!r}, the oracle has {want[k]!r} (rel {err / abs(want[k]) if want[k] else err:.3g})")
    return rel


# -------------------------------------------------------------------------------------- A. one evaluation away from identity
@pytest.mark.parametrize("sc", shard.GRAD_CASES, ids=_id)
def test_one_evaluation_exchanged_gradient_and_every_ranks_partial(sc):
    case, W = sc.case, sc.world
    terms, loss, gref, _ = cases.oracle_grad(case)
    atol = 1e-9 * max(1.0, float(np.abs(gref).max()))
    R = Ranks(sc)
    R.set_dv(cases.perturbed_dv(case))
    bufs, total = R.evaluate()
    g, t = _split(total, case)
    g[-1] /= case.J                    # (the stepwise path divides in the step)
    late = []
    rel = _check_terms(t, shard.terms_vector(case, cases.perturbed_dv(case)), "exchanged terms", late)
    worst = 0.0
    for r in range(W):
        gr, tr = _split(bufs[r], case)
        tw, gw = shard.oracle_partial(case, r, W)
        lo, hi = shard.bounds(case.N, W)[r]
        worst = max(worst, float(np.abs(gr - gw).max()))
        _check_terms(tr, tw, f"rank {r}'s own terms", late)
        np.testing.assert_allclose(gr, gw, rtol=0, atol=atol, err_msg=f"rank {r}'s own gradient")
        if r != 0:
            assert not tr[list(shard.NODE_TERMS)].any(), f"rank {r} adds to the node terms: {tr.tolist()}"
            untouched = ~shard.touched_rows(case, r, W)
            assert not gr[untouched].any(), f"rank {r} adds to rows none of its surfels touches (node terms off rank 0?)"
            if lo == hi:
                assert not gr.any() and not tr.any(), f"rank {r} has an empty shard and a non-zero partial"
        elif lo == hi:
            assert not tr[list(shard.SURFEL_TERMS)].any(), f"rank 0 has an empty shard and surfel terms {tr.tolist()}"
    print(sc.id, "exchanged grad err", np.abs(g - gref).max(), "atol", atol, "max|g|", np.abs(gref).max(), "terms rel err", rel,
          "worst rank partial err", worst, "matched", t[shard.T_PP_KEPT])
    np.testing.assert_allclose(g, gref, rtol=0, atol=atol)
    np.testing.assert_allclose(t[[k for k in range(NT) if k not in shard.COUNTS]].sum(), loss, rtol=1e-9)
    assert not late, "\n".join(late)


# ------------------------------------------------------------------------------------------------- B, C. ten steps in lock-step
@functools.lru_cache(maxsize=None)
def _ten_steps(sc):
    """(final deform_verts per rank, [(deform_verts per rank before the step, terms per rank after it)] of the first three
    steps, the unsharded run's result) -- shared by the tests below, do not modify."""
    from super_amd.deform_mesh import GraphFit
    R = Ranks(sc)
    rec = []
    for it in range(int(R.opt.num_optimize_iterations)):
        before = R.dvs() if it < 3 else None
        R.evaluate()
        R.step()
        if it < 3:
            rec.append((before, R.terms()))
    final = R.dvs()
    single = GraphFit(R.opt)(*R.frame, R.models).cpu().numpy()
    return final, rec, single


@pytest.mark.parametrize("sc", shard.SHARDED, ids=_id)
def test_ten_steps_every_rank_vs_oracle_and_ranks_bitwise_equal(sc):
    final, _, single = _ten_steps(sc)
    want, atol = cases.oracle_final(sc.case), cases.dv_atol(sc.case)
    print(sc.id, "ten steps: err", max(np.abs(f - want).max() for f in final), "atol", atol, "step", cases.step_of(want),
          "sharded - unsharded", np.abs(final[0] - single).max(), "unsharded err", np.abs(single - want).max())
    for r in range(1, sc.world):
        np.testing.assert_array_equal(final[r], final[0], err_msg=f"rank {r} against rank 0")
    for r in range(sc.world):
        np.testing.assert_allclose(final[r], want, rtol=0, atol=atol, err_msg=f"rank {r}")


@pytest.mark.parametrize("sc", shard.SHARDED, ids=_id)
def test_terms_reported_after_each_of_the_first_three_steps(sc):
    """Every rank holds the frame's terms after a step -- the true kept counts, not ``world`` times them: the second exchange
    sums the whole term block, so the morphing term's entries, global since the first, must come from one rank only."""
    _, rec, _ = _ten_steps(sc)
    rel, late = 0.0, []
    for it, (before, after) in enumerate(rec):
        for r in range(sc.world):
            want = shard.terms_vector(sc.case, before[r])
            rel = max(rel, _check_terms(after[r], want, f"step {it + 1}, rank {r}", late))
    last = rec[-1][1][0]
    print(sc.id, "terms after steps 1..3: largest rel err", rel, "counts after step 3 (pp, morph, flag, corr)",
          [int(last[k]) for k in shard.COUNTS])
    assert not late, "\n".join(late)


# ------------------------------------------------------------------------------------------------------- D. degenerate shards
@pytest.mark.parametrize("sc", shard.DEGENERATE, ids=_id)
def test_empty_shards_and_a_frame_without_surfels(sc):
    """The ranks with an empty shard hold the frame's result and report its terms; N = 0 has the node terms only."""
    case, W = sc.case, sc.world
    empty = [r for r, (lo, hi) in enumerate(shard.bounds(case.N, W)) if lo == hi]
    assert empty == ([0] if case.N == 3 else [0, 1])
    final, rec, single = _ten_steps(sc)
    want, atol = cases.oracle_final(case), cases.dv_atol(case)
    for r in empty:
        np.testing.assert_allclose(final[r], want, rtol=0, atol=atol)
        np.testing.assert_array_equal(final[r], final[W - 1])
    before, after = rec[-1]
    t, t_want = after[empty[-1]], shard.terms_vector(case, before[empty[-1]])
    print(sc.id, "empty shards", empty, "err", np.abs(final[empty[-1]] - want).max(), "atol", atol, "terms after step 3", t.tolist())
    late = []
    _check_terms(t, t_want, "an empty rank's terms after step 3", late)
    assert not late, "\n".join(late)
    assert np.isfinite(t).all() and t[shard.T_ARAP] > 0 and t[shard.T_ROT] > 0
    if case.N == 0:
        assert not t[list(shard.SURFEL_TERMS)].any()
        np.testing.assert_allclose(single, want, rtol=0, atol=atol)
    else:
        assert t[shard.T_PP_KEPT] == t_want[shard.T_PP_KEPT] > 0


# --------------------------------------------------------------------------------------------------------------- E. re-sharding
def _own_evaluation(R, gf):
    """one evaluation and one step of ``gf`` alone at the perturbed deform_verts: (its partial, deform_verts after the step)"""
    import torch
    R.gfs = [gf]
    R.set_dv(cases.perturbed_dv(R.case))
    gf.eval_morph()
    gf.eval_losses()
    part = gf.get_partial(torch.empty(R.n + NT, dtype=torch.float64, device="cuda")).cpu().numpy()
    gf.step()
    return part, gf.deform_verts().cpu().numpy()


@pytest.mark.parametrize("case,determined", [(shard.RESHARD_TINY, True), (shard.RESHARD_LARGE, False)], ids=["tiny", "large"])
def test_a_handle_sharded_again_is_unbound_and_then_a_fresh_handle(case, determined):
    """slm_gf_set_shard unbinds every slot (the bounds are fixed at the bind).  Bound again, the handle gives the bits of a
    fresh (2, 3) handle wherever the bits are determined: everything on the tiny frame, whose shard lies in one wave; on the
    large one the terms and the global row (block partials folded in a fixed order) -- its local rows add with float64
    atomics from five workgroups, two fresh handles differ there too, so they are held to the gradient tolerance."""
    from super_amd.deform_mesh import GraphFit
    R = Ranks(shard.ShardCase(case, 2), ranks=[1])
    used = R.gfs[0]
    for _ in range(2):                                   # used: optimiser state, step count, partials, semantic scratch
        used.eval_morph()
        used.eval_losses()
        used.step()
    lib = used.lib
    assert lib.slm_gf_set_shard(used.h, 2, 3) == 0
    used.rank, used.world = 2, 3
    buf = R.torch.empty(R.n + NT, dtype=R.torch.float64, device="cuda")
    from super_amd.LM import _dev_ptr
    for name, args in (("slm_gf_eval_morph", (used.h, 1, None)), ("slm_gf_eval_losses", (used.h, 1, None)),
                       ("slm_gf_step", (used.h, 1, None)), ("slm_gf_get_partial", (used.h, 0, _dev_ptr(buf), None)),
                       ("slm_gf_set_partial", (used.h, 0, _dev_ptr(buf), None)),
                       ("slm_gf_get_deform", (used.h, 0, _dev_ptr(buf), None)),
                       ("slm_gf_loss_grad", (used.h, 0, _dev_ptr(buf), None, None, None))):
        rc = getattr(lib, name)(*args)
        got = lib.slm_last_error()
        assert (rc, got) == (UNBOUND, b"slm_gf: slot used before slm_gf_bind_frame"), (name, rc, got)
    R.bind(used)
    np.testing.assert_array_equal(used.deform_verts().cpu().numpy(), shard.identity(case))
    fresh = GraphFit(R.opt, rank=2, world=3, all_reduce=lambda t: None)
    R.bind(fresh)
    p_used, dv_used = _own_evaluation(R, used)
    p_fresh, dv_fresh = _own_evaluation(R, fresh)
    n, J = R.n, case.J
    atol = 1e-9 * max(1.0, float(np.abs(p_fresh[:n]).max()))
    print(case.id, "re-sharded - fresh: local rows", np.abs(p_used[:7 * J] - p_fresh[:7 * J]).max(), "global row",
          np.abs(p_used[7 * J:n] - p_fresh[7 * J:n]).max(), "terms", np.abs(p_used[n:] - p_fresh[n:]).max(), "deform_verts",
          np.abs(dv_used - dv_fresh).max(), "max|g|", np.abs(p_fresh[:n]).max(), "terms", p_fresh[n:].tolist())
    assert p_fresh[n + shard.T_PP_KEPT] > 0 and np.abs(p_fresh[:7 * J]).max() > 0
    np.testing.assert_array_equal(p_used[n:], p_fresh[n:])
    np.testing.assert_array_equal(p_used[7 * J:n], p_fresh[7 * J:n])
    if determined:
        np.testing.assert_array_equal(p_used, p_fresh)
        np.testing.assert_array_equal(dv_used, dv_fresh)
    else:
        np.testing.assert_allclose(p_used[:7 * J], p_fresh[:7 * J], rtol=0, atol=atol)
        np.testing.assert_allclose(dv_used, dv_fresh, rtol=0, atol=cases.dv_atol(case))
