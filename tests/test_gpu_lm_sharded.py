"""Surfel-sharded LM (slm_set_shard and the stepwise entry points slm_lm_grad_local / slm_lm_solve / slm_lm_loss_local /
slm_lm_accept with slm_lm_exchange_* between them, csrc/slm_lm.hip) at world 2, 3 and 4: weighted and unweighted, every
num_neighbors family, batches, the solver forms, float32 state and the shard edges, against the float64 models
(oracle/lm_oracle.py, lm_weight_model.py) and the unsharded run on the same device.  Needs ONE MI355X (-m gpu).

The ranks are emulated on one device (lm_shard_cases.Ranks): W solver contexts with ``slm_enable_data_weights``, then
``slm_set_shard(r, W)``, bound to the same frames and driven in lock-step, the all-reduce being ``torch.stack(bufs).sum(0)``
set back into every context.  F drives ``LM_Solver._sharded_stages`` of W Python mirrors instead, with collectives that act
in place on the ranks' ``exchange_view`` tensors; test_gpu_dist_procgroup.py runs the mirror under a real process group.

  A  one evaluation per rank at identity and away from it: slm_loss (the share's loss and count), slm_assemble (the shares
     are a partition of the Jacobian), the exchanged records (bitwise the same on every rank) and the step behind them
  B  full loops: the ranks bitwise equal, equal to the unsharded run (summation order), equal to the model's trace
  C  batches of three slots of unlike N; a batch with a slot without its semantic inputs is refused, the next one runs
  D  N = 3, N = 1 (ranks without a surfel) run; N = 0 is refused at the bind, the handle takes a frame afterwards
  E  re-sharding unbinds; the refusals around slm_set_shard
  F  the Python mirror: injected collectives, and a semantic weight without ``sf_point_plane``

Tolerances are the project's own for the same quantities (docstrings of test_gpu_lm_weights.py and test_gpu_lm_corr.py): JtJ 1e-7
of its largest entry, jtl 1e-8, slm_loss 1e-8 relative; runs that differ only in summation order 1e-11 of the step's largest
component and 1e-9 on beta and on the losses; the model's trace 1e-6 relative on the loss, the accept flags where the decision
is no rounding-level tie, final beta 1e-4; counts exact.  Every test prints what it measured (pytest -s).  The model's
conditions (``lm_weight_model.check_conditions``) are asserted at every beta a comparison is made at; no surfel is excluded.

The accept flags of a sharded run are compared with the unsharded run's under the rule they are compared with the model's
under: wherever the decision is no rounding-level tie.  Measured on an MI355X: the two runs' losses differ by at most 8.8e-13
relative and their final betas by at most 3.6e-10 (every case of B, C, D and F), and in five of the small scenes (a256-hard-W4,
a257-plain-W2 and -W3, n65-hard-W2 and -W3) one stalled iteration, the eighth or ninth, fell the other way; ``M_grad``,
``M_loss`` and ``status`` are equal in every iteration of every case.

Largest errors measured on an MI355X, against the tolerances above: a share's slm_loss 5.5e-14 relative (1e-8); the summed
slm_assemble 6.8e-16 of the largest JtJ entry (1e-7) and 8.0e-15 on jtl (1e-8); the step behind the exchanged records 1.6e-15
of its largest component (1e-11); the loop's losses against the model 6.3e-11 relative on every scene but the tiny ones (1e-6).

What a sharded handle's parity entry points return is pinned here (A1, A2) and stated in include/super_lm.h: ``slm_loss`` the
data loss and count of the surfels [N r // W, N (r + 1) // W) of the caller's order, in either data form, and every
regulariser in full; ``slm_assemble`` the same window's data blocks in the pair form (before this file existed it returned
the WHOLE frame's there: k_data_grad did not look at the window), the rank's workgroups of tuple positions in the tuple form,
and every regulariser in full."""
import ctypes as C
import functools

import numpy as np
import pytest

import lm_shard_cases as lc
from lm_shard_cases import Ranks, ShardCase
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

_id = lambda c: c.id    # noqa: E731
TOL_STEP = 1e-11        # of the step's largest component: runs that differ only in summation order
TOL_ORDER = 1e-9        # beta (absolute) and losses (relative) of such runs
TOL_BETA = 1e-4         # final beta against the model
SLOT_UNBOUND = b"slot used before slm_bind_frame"


def _beta_of(name, tag):
    return lc.identity(lc.scene(name).J) if tag == "identity" else lc.perturbed(name)


# ------------------------------------------------------------------------------------------------ A. one evaluation per rank
A1_CASES = lc.POINTS + lc.EMPTY_SHARE + lc.ZERO_WEIGHT_SHARE + [c for c, what in lc.TINY if what == "runs"]


@pytest.mark.parametrize("case", A1_CASES, ids=_id)
def test_a1_slm_loss_returns_the_ranks_window_and_every_regulariser(case):
    """The share is the caller-order window in BOTH data forms (the tuple form's slm_loss runs k_data_loss too; its loop's loss
    pass, k_data_eval, takes 256-position workgroups of the tuple-sorted list instead -- B covers that through the sums)."""
    name, W = case.scene, case.world
    R = lc.case_ranks(case)
    worst = 0.0
    for tag in ("identity", "perturbed"):
        beta = _beta_of(name, tag)
        shares, (whole, count) = lc.share_losses(name, case.cfg, beta, W)        # (the model's conditions are asserted inside)
        reg = orc.total_loss(lc.frame(name), beta, lc.lwm._no_data(orc.default_opt()))[0]
        R.set_beta(beta)
        outs = [R.loss(e) for e in R.es]
        for r, (out, (want, cnt)) in enumerate(zip(outs, shares)):
            print(case.id, tag, "rank", r, "loss", out[0], "want", want, "count", out[3], cnt, "regularisers", out[1] + out[2], reg)
            assert int(out[3]) == cnt, (r, out, cnt)
            if cnt == 0 or want == 0.0:
                assert out[0] == 0.0, (r, out)
            else:
                np.testing.assert_allclose(out[0], want, rtol=1e-8, atol=1e-300)
                worst = max(worst, abs(out[0] - want) / want)
            if tag == "perturbed":                           # (at identity the regularisers are rounding residue of zero)
                np.testing.assert_allclose(out[1] + out[2], reg, rtol=1e-8, atol=1e-300)
            np.testing.assert_array_equal(out[1:3], outs[0][1:3])
        assert sum(int(o[3]) for o in outs) == count
        np.testing.assert_allclose(sum(o[0] for o in outs), whole, rtol=1e-8, atol=1e-300)
    R.close()
    print(case.id, "largest relative error of a share's loss", worst)


@pytest.mark.parametrize("case", lc.POINTS + lc.EMPTY_SHARE[:2] + lc.ZERO_WEIGHT_SHARE, ids=_id)
def test_a2_slm_assemble_shares_are_a_partition(case):
    """sum_r A_r - (W - 1) A_reg against the model's full system (Rot products in float32 on both sides): a surfel counted by
    two ranks or by none misses the JtJ tolerance by orders of magnitude"""
    name, W = case.scene, case.world
    R = lc.case_ranks(case)
    for tag in ("identity", "perturbed"):
        beta = _beta_of(name, tag)
        lc.conditions(name, case.cfg, beta)
        A_ref, b_ref, _ = lc.full_system(name, case.cfg, beta)
        A_reg, b_reg = lc.reg_system(name, beta)
        R.set_beta(beta)
        parts = [R.assemble(e) for e in R.es]
        A = sum(p[0] for p in parts) - (W - 1) * A_reg
        b = sum(p[1] for p in parts) - (W - 1) * b_reg
        scale = max(1.0, np.abs(A_ref).max())
        data = np.abs(A_ref - A_reg).max()
        print(case.id, tag, "JtJ err", np.abs(A - A_ref).max(), "tol", 1e-7 * scale, "jtl err", np.abs(b - b_ref).max(),
              "largest data entry", data)
        assert data > 1e3 * 1e-7 * scale                     # (a share counted twice or dropped is visible)
        np.testing.assert_allclose(b, b_ref, rtol=0, atol=1e-8)
        np.testing.assert_allclose(A, A_ref, rtol=0, atol=1e-7 * scale)
        for r, (Ar, br) in enumerate(parts):                 # no rank returns the whole frame's data term, none returns nothing
            own = np.abs(Ar - A_reg).max()
            assert 1e-7 * scale < own or lc.share_losses(name, case.cfg, beta, W)[0][r][0] == 0.0, (r, own)
    R.close()


@functools.lru_cache(maxsize=None)
def _unsharded_step(name, cfg, tag):
    """slm_solve(u = 10) of a fresh unsharded handle at the beta (shared, do not modify)"""
    R = Ranks([lc.scene(name)], cfg, 1, sems=[lc.sem(name)], ranks=[None])
    R.set_beta(_beta_of(name, tag))
    e = R.es[0]
    P = 7 * lc.scene(name).J
    d = R.torch.zeros(P, dtype=R.torch.float64, device=R.dev)
    st = R.torch.zeros(1, dtype=R.torch.int32, device=R.dev)
    R._lib.check(e.lib.slm_solve(e.h, 0, 10.0, d.data_ptr(), st.data_ptr(), e.stream), "slm_solve")
    assert int(st.item()) == 0
    out = d.cpu().numpy()
    R.close()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("case", lc.POINTS, ids=_id)
def test_a3_exchanged_records_are_the_same_bits_and_the_step_is_the_unsharded_one(case):
    name, W = case.scene, case.world
    want = {tag: _unsharded_step(name, case.cfg, tag) for tag in ("identity", "perturbed")}
    R = lc.case_ranks(case)
    for tag in ("identity", "perturbed"):
        R.bind()                                             # (u back to u0 = 10, the iteration counter to 0)
        R.set_beta(_beta_of(name, tag))
        for e in R.es:
            for what in (lc.SLM_X_PAIR_BLOCKS, lc.SLM_X_DELTA, lc.SLM_X_DATA_LOSS):
                ptr, n = C.c_void_p(), C.c_int64(-1)
                R._lib.check(e.lib.slm_lm_exchange_ptr(e.h, 0, what, C.byref(ptr), C.byref(n)), "slm_lm_exchange_ptr")
                assert n.value == R.exchange_size(e, 0, what) == R.get(e, 0, what).numel() > 0 and ptr.value
            assert R.exchange_size(e, 0, lc.SLM_X_DELTA) == 7 * lc.scene(name).J
        own = R.grad_and_exchange()
        sizes = {b.numel() for b in own}
        assert len(sizes) == 1
        own = [b.cpu().numpy() for b in own]
        after = [R.get(e, 0, lc.SLM_X_PAIR_BLOCKS).cpu().numpy() for e in R.es]
        for a in after[1:]:
            np.testing.assert_array_equal(a, after[0])
        np.testing.assert_allclose(after[0], sum(own), rtol=1e-15, atol=1e-300)
        assert all(np.abs(o).max() > 0 for o in own)         # every rank of these families has matched surfels
        R.call("slm_lm_solve")
        ref = want[tag]
        big = np.abs(ref).max()
        for r, e in enumerate(R.es):
            d = R.get(e, 0, lc.SLM_X_DELTA).cpu().numpy()
            print(case.id, tag, "rank", r, "step err", np.abs(d - ref).max(), "largest component", big, "tol", TOL_STEP * big)
            np.testing.assert_allclose(d, ref, rtol=0, atol=TOL_STEP * big)
    R.close()


# --------------------------------------------------------------------------------------------------------------- B. full loops
@functools.lru_cache(maxsize=None)
def _unsharded(names, cfg, state_f64=True, solver_path=0, iters=10):
    """([(beta, records)] per slot, solver form) of slm_run on a fresh unsharded handle (shared, do not modify)"""
    return lc.unsharded([lc.scene(n) for n in names], cfg, state_f64, solver_path, iters, sems=[lc.sem(n) for n in names],
                        opt=ShardCase(names[0], cfg, 1, iters=iters).opt)


@functools.lru_cache(maxsize=None)
def _loop(case):
    """[(beta, records)] per rank of the case's sharded loop (shared, do not modify)"""
    R = lc.case_ranks(case)
    out = [res[0] for res in R.run()]
    R.close()
    return out


def _fields(recs, *names):
    return [tuple(r[k] for k in names) for r in recs]


def _same_decisions(tag, recs, want):
    """``M_grad``, ``M_loss`` and ``status`` of every iteration equal; ``accepted`` equal wherever the decision of ``want`` is no
    rounding-level tie (``decisive`` of test_gpu_lm_weights.py: the loss further than 1e-9 relative from the best so far).
    In a stalled iteration the loss sits within 1e-13 relative of the best one (figures in the module docstring), the two runs
    differ by about as much, and ``loss < minimal_loss`` falls either way."""
    assert _fields(recs, "M_grad", "M_loss", "status") == _fields(want, "M_grad", "M_loss", "status"), tag
    dec = lc.tw.decisive([x["loss"] for x in want])
    acc, wacc = np.array([x["accepted"] for x in recs]), np.array([x["accepted"] for x in want])
    np.testing.assert_array_equal(acc[dec], wacc[dec], err_msg=tag)
    assert dec[:5].all(), (tag, dec)                         # (the comparison is no empty one)


def _check_ranks_against_unsharded(tag, ranks, want):
    """``ranks``: [(beta, records)] per rank, ``want``: (beta, records) of the unsharded run"""
    beta0, recs0 = ranks[0]
    for r, (beta, recs) in enumerate(ranks[1:], 1):
        np.testing.assert_array_equal(beta, beta0, err_msg=f"{tag}: rank {r} against rank 0")
        assert recs == recs0, f"{tag}: rank {r}'s records against rank 0's"
    wb, wr = want
    print(tag, "sharded - unsharded: beta", np.abs(beta0 - wb).max(), "loss rel",
          max(abs(a["loss"] - b["loss"]) / abs(b["loss"]) for a, b in zip(recs0, wr)), "accepted", [int(x["accepted"]) for x in recs0],
          "M_grad", [x["M_grad"] for x in recs0])
    _same_decisions(tag, recs0, wr)
    assert all(x["status"] == 0 for x in recs0)
    np.testing.assert_allclose(beta0, wb, rtol=0, atol=TOL_ORDER, err_msg=tag)
    np.testing.assert_allclose([x["loss"] for x in recs0], [x["loss"] for x in wr], rtol=TOL_ORDER, err_msg=tag)


def _check_against_model(tag, beta, recs, name, cfg, iters, flags=True):
    want_beta, trace = lc.model_trace(name, cfg, iters)
    want = np.array([t["loss"] for t in trace])
    loss = np.array([r["loss"] for r in recs])
    print(tag, "model: loss rel", np.abs(loss / want - 1).max(), "beta", np.abs(beta - want_beta).max())
    np.testing.assert_allclose(loss, want, rtol=1e-6, atol=1e-12, err_msg=tag)
    dec = lc.tw.decisive(want)
    acc = np.array([r["accepted"] for r in recs])
    if flags:
        np.testing.assert_array_equal(acc[dec], np.array([t["accepted"] for t in trace])[dec], err_msg=tag)
    assert [r["M_loss"] for r in recs] == [t["M_loss"] for t in trace], tag
    assert [r["M_grad"] for r in recs] == [t["M_grad"] for t in trace], tag      # the frame's count, never W times it
    np.testing.assert_allclose(beta, want_beta, rtol=0, atol=TOL_BETA, err_msg=tag)


@pytest.mark.parametrize("case", lc.LOOPS, ids=_id)
def test_b_loop_ranks_bitwise_equal_the_unsharded_run_and_the_models_trace(case):
    want, _ = _unsharded((case.scene,), case.cfg, case.state_f64, case.solver_path, case.iters)
    ranks = _loop(case)
    _check_ranks_against_unsharded(case.id, ranks, want[0])
    _check_against_model(case.id, *ranks[0], case.scene, case.cfg, case.iters)
    acc = [x["accepted"] for x in ranks[0][1]]
    if case in lc.GOLDENS or case.cfg == "trunc":
        assert False in acc[:-1] and True in acc[acc.index(False):]      # an iteration runs behind a reject (M_grad compared above)


# ------------------------------------------------------------------------------------------------------------------ C. batches
def _check_batch(tag, names, cfg, W, solver_path, batch):
    single_un, _ = zip(*[_unsharded((n,), cfg) for n in names])
    for i, name in enumerate(names):
        ranks = [res[i] for res in batch]
        _check_ranks_against_unsharded(f"{tag} slot {i} ({name})", ranks, single_un[i][0])
        beta1, recs1 = _loop(ShardCase(name, cfg, W))[0]                  # the slot's single-slot sharded run
        np.testing.assert_allclose(ranks[0][0], beta1, rtol=0, atol=TOL_ORDER)
        np.testing.assert_allclose([x["loss"] for x in ranks[0][1]], [x["loss"] for x in recs1], rtol=TOL_ORDER)
        _same_decisions(f"{tag} slot {i} ({name}) against its single-slot sharded run", ranks[0][1], recs1)
        _check_against_model(f"{tag} slot {i} ({name})", *ranks[0], name, cfg, 10)


@functools.lru_cache(maxsize=None)
def _weighted_batch():
    names, cfg, W = lc.BATCH_WEIGHTED
    R = Ranks([lc.scene(n) for n in names], cfg, W, sems=[lc.sem(n) for n in names])
    out = R.run()
    R.close()
    return out


def test_c_weighted_batch_of_three_slots_of_unlike_n():
    names, cfg, W = lc.BATCH_WEIGHTED
    assert sorted(lc.scene(n).N for n in names) == [65, 1200, 1200]       # (and the two of 1200 match 1123 and 754 surfels)
    _check_batch("weighted batch", names, cfg, W, 0, _weighted_batch())


# slm_debug_last_solver_form of a sharded step of the three-slot batch (enqueue_front_solve): solver_path 0 takes the task
# graph (1) while frames x nodes stays small, 3 the per-level launches (0); 4 asks for the hybrid form (2), which needs every
# slot to have the same number of levels and the same cut (solve_is_hybrid) -- slots of 40, 12 and 40 nodes do not: this batch
# is too small for it and the per-level form (0) runs.  The hybrid form under exchanged records needs a batch of like, larger
# graphs (eight frames of 300 nodes in test_gpu_num_neighbors.py); no test here forces it.
FORM_OF_PATH = {0: (1,), 3: (0,), 4: (0,)}


@pytest.mark.parametrize("solver_path", [0, 3, 4])
def test_c_unweighted_batch_in_every_solver_form(solver_path):
    names = lc.BATCH_PLAIN
    assert len({lc.scene(n).N for n in names}) == 3
    R = Ranks([lc.scene(n) for n in names], None, 3, solver_path=solver_path)
    out = R.run()
    forms = [e.lib.slm_debug_last_solver_form(e.h) for e in R.es]
    R.close()
    print("solver_path", solver_path, "form", forms, "(0 per-level launches, 1 task graph, 2 hybrid)")
    assert len(set(forms)) == 1 and forms[0] in FORM_OF_PATH[solver_path], forms
    _check_batch(f"batch sp{solver_path}", names, None, 3, solver_path, out)


def test_c_batch_with_a_slot_without_semantic_inputs_is_refused_and_the_next_runs():
    names, cfg, W = lc.BATCH_WEIGHTED
    R = Ranks([lc.scene(n) for n in names], cfg, W, sems=[lc.sem(n) for n in names], bind=False)
    for e in R.es:
        for slot in range(3):
            R.bind_slot(e, slot, semantic=slot != 1)
    text = b": slot 1 has no semantic inputs; call slm_bind_data_semantic after slm_bind_frame"
    for e in R.es:
        for fn in ("slm_lm_grad_local", "slm_lm_loss_local"):
            rc = getattr(e.lib, fn)(e.h, 3, e.stream)
            got = e.lib.slm_last_error()
            assert (rc, got) == (lc.UNBOUND, fn.encode() + text), (fn, rc, got)
    R.bind()
    out = R.run()
    R.close()
    for got, want in zip(out, _weighted_batch()):
        for (b, r), (wb, wr) in zip(got, want):
            np.testing.assert_allclose(b, wb, rtol=0, atol=TOL_ORDER)
            _same_decisions("the batch after the refused one", r, wr)


# -------------------------------------------------------------------------------------------------- D. tiny and degenerate
@pytest.mark.parametrize("case,what", lc.TINY, ids=[c.id for c, _ in lc.TINY])
def test_d_tiny_frames_run_and_a_frame_without_surfels_is_refused_at_the_bind(case, what):
    from super_amd.engine import DeviceFrame
    if what == "runs":
        empty = [r for r, (lo, hi) in enumerate(lc.bounds(lc.scene(case.scene).N, case.world)) if lo == hi]
        assert empty
        want, _ = _unsharded((case.scene,), case.cfg)
        ranks = _loop(case)
        _check_ranks_against_unsharded(case.id, ranks, want[0])
        # (against the model without the accept flags: with three surfels or one the loss falls below 1e-9, under the absolute
        #  floor 1e-12 of the loss comparison itself, where the device and the model differ by up to 6.4e-4 relative and the
        #  relative rule of ``decisive`` says nothing)
        _check_against_model(case.id, *ranks[0], case.scene, case.cfg, case.iters, flags=False)
        assert ranks[0][1][0]["M_grad"] == lc.scene(case.scene).N
        return
    where, code, text = what
    assert where == "bind" and lc.scene(case.scene).N == 0
    R = lc.case_ranks(case, bind=False)
    for e in R.es:
        cs = DeviceFrame.from_scene(lc.scene(case.scene), R.dev, state_f64=True).c_struct()
        rc = e.lib.slm_bind_frame(e.h, 0, C.byref(cs), e.stream)
        got = e.lib.slm_last_error()
        print(case.id, "slm_bind_frame", rc, got)
        assert (rc, got) == (code, text)
        rc = e.lib.slm_lm_grad_local(e.h, 1, e.stream)
        assert (rc, e.lib.slm_last_error()) == (lc.UNBOUND, SLOT_UNBOUND)
    # the handles take a normal frame afterwards
    R.scenes, R.sems = [lc.scene("n65")], [lc.sem("n65")]
    R.bind()
    out = [res[0] for res in R.run()]
    R.close()
    _check_ranks_against_unsharded(case.id + " then n65", out, _unsharded(("n65",), case.cfg)[0][0])


# ------------------------------------------------------------------------------------------ E. re-sharding and order of calls
@pytest.mark.parametrize("name,cfg", [("k6", None), ("k4", "hard"), ("k4", None)], ids=["pairs", "weighted", "tuples"])
def test_e_a_handle_sharded_again_is_unbound_and_then_the_new_ranks_share(name, cfg):
    R = Ranks([lc.scene(name)], cfg, 2, sems=[lc.sem(name)], ranks=[0])
    e = R.es[0]
    R.step()                                                 # used: records, u, reuse flags (alone: its own share only)
    assert e.lib.slm_set_shard(e.h, 1, 3) == 0, e.lib.slm_last_error()
    buf = R.torch.zeros(16, dtype=R.torch.float64, device=R.dev)
    for fn, args in (("slm_lm_grad_local", (e.h, 1, e.stream)), ("slm_lm_solve", (e.h, 1, e.stream)),
                     ("slm_lm_loss_local", (e.h, 1, e.stream)), ("slm_lm_accept", (e.h, 1, e.stream)),
                     ("slm_loss", (e.h, 0, buf.data_ptr(), e.stream)),
                     ("slm_lm_exchange_get", (e.h, 0, lc.SLM_X_DELTA, buf.data_ptr(), e.stream))):
        rc = getattr(e.lib, fn)(*args)
        assert (rc, e.lib.slm_last_error()) == (lc.UNBOUND, SLOT_UNBOUND), (fn, rc, e.lib.slm_last_error())
    R.bind()
    for tag in ("identity", "perturbed"):
        beta = _beta_of(name, tag)
        want, cnt = lc.share_losses(name, cfg, beta, 3)[0][1]
        R.set_beta(beta)
        out = R.loss(e)
        print(name, cfg, tag, "rank 1 of 3 after re-sharding: loss", out[0], "want", want, "count", out[3], cnt)
        assert int(out[3]) == cnt > 0
        np.testing.assert_allclose(out[0], want, rtol=1e-8, atol=1e-300)
    R.close()


def test_e_refusals_around_slm_set_shard():
    from super_amd.engine import DeviceFrame, Engine
    R = Ranks([lc.scene("k4")], None, 1, ranks=[None])       # a K = 4 slot bound on a handle that was never sharded
    e = R.es[0]
    buf = R.torch.zeros(1 << 20, dtype=R.torch.float64, device=R.dev)
    n = C.c_int64(-1)
    for fn, args in (("slm_lm_exchange_get", (e.h, 0, lc.SLM_X_PAIR_BLOCKS, buf.data_ptr(), e.stream)),
                     ("slm_lm_exchange_size", (e.h, 0, lc.SLM_X_PAIR_BLOCKS, C.byref(n)))):
        rc = getattr(e.lib, fn)(*args)
        assert (rc, e.lib.slm_last_error()) == (lc.UNBOUND, b"slm_lm_exchange: the slot was bound without slm_set_shard"), fn
    assert e.lib.slm_set_shard(e.h, 0, 2) == 0               # ... and sharded now: unbound
    rc = e.lib.slm_lm_exchange_get(e.h, 0, lc.SLM_X_PAIR_BLOCKS, buf.data_ptr(), e.stream)
    assert (rc, e.lib.slm_last_error()) == (lc.UNBOUND, SLOT_UNBOUND)
    R.bind()
    rc = e.lib.slm_run(e.h, 1, e.stream)
    assert (rc, e.lib.slm_last_error()) == (lc.UNSUPPORTED, b"slm_run: the frame is sharded; drive slm_lm_grad_local / slm_lm_solve / "
                                            b"slm_lm_loss_local / slm_lm_accept with the exchanges between them")
    R.step()                                                 # the refused slm_run left the handle usable
    R.close()


# ------------------------------------------------------------------------------------------------------- F. Python surface
class _Collectives:
    """In-place collectives over the ``exchange_view`` tensors of W mirrors held in one process: rank r's k-th call waits (is
    recorded) until every rank has made its k-th call, then all W tensors are combined in place."""

    def __init__(self, W):
        import torch
        self.torch, self.W = torch, W
        self.calls = [0] * W
        self.pending = {}

    def _op(self, r, combine):
        def op(t):
            k = self.calls[r]
            self.calls[r] += 1
            got = self.pending.setdefault(k, {})
            got[r] = t
            if len(got) == self.W:
                out = combine([got[i] for i in range(self.W)])
                for x in self.pending.pop(k).values():
                    x.copy_(out)
        return op

    def all_reduce(self, r):
        return self._op(r, lambda ts: self.torch.stack(ts).sum(0))

    def broadcast(self, r):
        return self._op(r, lambda ts: ts[0].clone())


def _mirror_ranks(opt, W, frames, **kw):
    """W ``LM_Solver`` mirrors of ``opt`` stepped alternately through ``_sharded_stages``; [(beta, records)] per rank"""
    import torch
    from super_amd import _lib
    from super_amd.LM import LM_Solver, _dev_ptr, _stream_ptr
    col = _Collectives(W)
    lms = [LM_Solver(opt, rank=r, world=W, all_reduce=col.all_reduce(r), broadcast=col.broadcast(r), **kw) for r in range(W)]
    gens, hs = [], []
    for lm in lms:
        h = lm._handle()
        sf, inputs, new_data = frames()
        bf = lm._bind(h, 0, sf, inputs, new_data)
        lm._bind_semantic(h, 0, bf, sf, new_data)
        hs.append((h, bf))
        gens.append(lm._sharded_stages(h, 1, bf.device))
    for _ in range(3 * int(opt.num_optimize_iterations)):
        for g in gens:
            next(g)
    for g in gens:
        with pytest.raises(StopIteration):
            next(g)
    assert not col.pending
    out = []
    for lm, (h, bf) in zip(lms, hs):
        st = _stream_ptr(bf.device)
        beta = torch.empty((bf.J, 7), dtype=torch.float64, device=bf.device)
        _lib.check(lm.lib.slm_get_beta(h, 0, _dev_ptr(beta), st), "slm_get_beta")
        out.append((beta.cpu().numpy(), lm.records(h, 0, st)))
    return out


PY_KW = {"hard": dict(sf_hard_seg_point_plane=True), "soft": dict(sf_soft_seg_point_plane=True), "trunc": dict(depth_model="raft_stereo")}


@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("cfg", ["hard", "soft", "trunc"])
def test_f_python_mirror_with_in_place_collectives(cfg, W):
    from super_amd.LM import LM_Solver
    name = "k4"
    opt = lc.tw._opt(4, **PY_KW[cfg])
    ranks = _mirror_ranks(opt, W, lambda: lc.tw._sem_frame(name), weighted_data=True)
    lm = LM_Solver(opt, weighted_data=True)
    assert (lm.seg_mode, lm.pp_max) == lc.CONFIGS[cfg]
    want = lm.LM(*lc.tw._sem_frame(name)).cpu().numpy(), lm.last_records[0]
    _check_ranks_against_unsharded(f"mirror {cfg} W{W}", ranks, want)
    _check_against_model(f"mirror {cfg} W{W}", *ranks[0], name, cfg, 10)


@pytest.mark.parametrize("cfg", ["hard", "soft"])
def test_f_semantic_weight_without_sf_point_plane_is_exchanged(cfg):
    """``LM_Solver._config`` puts the data term on for a semantic weight also without ``opt.sf_point_plane``; the sharded loop
    decided its exchanges by ``opt.sf_point_plane`` alone, so every rank solved on its own share and nothing was summed (the
    ranks disagreed with each other and with the unsharded solver: see the commit message for the figures)."""
    from super_amd.LM import LM_Solver
    name, W = "k4", 2
    opt = lc.tw._opt(4, sf_point_plane=False, **PY_KW[cfg])
    ranks = _mirror_ranks(opt, W, lambda: lc.tw._sem_frame(name), weighted_data=True)
    lm = LM_Solver(opt, weighted_data=True)
    want = lm.LM(*lc.tw._sem_frame(name)).cpu().numpy(), lm.last_records[0]
    assert want[1][0]["M_grad"] > 1000                       # the term is on
    _check_ranks_against_unsharded(f"mirror {cfg} without sf_point_plane", ranks, want)
    _check_against_model(f"mirror {cfg} without sf_point_plane", *ranks[0], name, cfg, 10)
