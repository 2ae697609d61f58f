"""The pair-record Jacobian pass (python-super_amd/csrc/slm_prep.hip: ``prep_pairs``; slm_pairs.h: ``pair_gram`` behind
``k_data_grad_pairs``, ``k_corr_grad_pairs`` and the morph kernel; slm_front.hip: ``k_pair_scatter``) on the frames of
tests/pair_plan_cases.py against the NumPy construction of tests/pair_plan_model.py, through the C ABI:

  plan      ``slm_debug_read_plan`` 13 blk_key, 14 sf_pidx, 15 sf_perm (16 tri_pidx with a face mesh) and ``slm_get_plan_info[7]``
            equal the model EXACTLY
  records   on a handle with ``slm_set_shard(0, 1)``, ARAP and Rot off, at a perturbed beta and at the identity:
            ``slm_lm_grad_local`` then ``slm_lm_exchange_get(SLM_X_PAIR_BLOCKS)`` against the records cut from the oracle's
            dense data-term system; the matched count EXACTLY
  solve     unsharded, ARAP and Rot on: one ``slm_solve(u = 0.37)`` on solver paths 2 and 3 against the dense Cholesky solve
  shares    world 2 and 3 (emulated ranks, lm_shard_cases.Ranks): every rank against the model restricted to its positions of
            sf_perm, the ranks' sum against the world-1 records
  users     the point-point correspondences, the morph term, the hard semantic weights and the face term on the same frames
  batch     three unlike frames of one K in one set of launches against their single-slot records

num_neighbors 4 is put onto the pair-record form with ``slm_enable_data_weights(0, 1e30)``: the truncation weight [s < 1e30]
is 1 for every matched surfel, so the system is the plain one (and the kernel the weighted variant of k_data_grad_pairs).

Tolerances.  Plan arrays, counts, matched counts: exact.  Records: see RECORD_TOL below.  Solve: the two bounds of
tests/test_gpu_solver_graphs.py (forward 1e-9 max(1, |ref|), backward 64 P eps).  The perturbed beta of the issue is generic
(its quaternions are not on the 2^-8 grid of solver_graph_cases.perturbed_beta), and the Rot term is evaluated in FLOAT32 by the
reference, the oracle and the library alike: the oracle widens r and J to float64 BEFORE it forms J^T J and J^T r, the library
and the reference form the products in float32 (solver_graph_cases.perturbed_beta measured 1 400 - 2 100 P eps from that
alone, on every solver path).  The reference of the solve test is therefore the oracle's system with the Rot products rounded
to float32 (lm_shard_cases._rot32, the rule of test_gpu_lm_weights.py / test_gpu_lm_face.py); the figures against the plain
oracle are printed beside it.

Needs an MI355X (-m gpu).  Run with -s for one MEASURE line per comparison."""
import ctypes as C
import functools

import numpy as np
import pytest

import lm_corr_model as lcm
import lm_face_model as lfm
import lm_morph_model as lmm
import lm_shard_cases as lsc
import lm_weight_model as lwm
import pair_plan_cases as ppc
import pair_plan_model as ppm
import solver_graph_cases as sgc
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

# Largest figures over all 402 comparisons of this file, measured on an MI355X (one run, -s; 63 tests in 5.7 s): record block
# entries against the models as a fraction of max(1, |A|max) (largest absolute difference 4.5e-13, at |A|max = 732 in
# holes_in_runs_k4 with the point-point correspondences), the J^T r entries, a batch slot against its single slot, the ranks'
# sum against the world-1 records, and the solve against the dense Cholesky solve of the system with float32 Rot products
# (against the plain oracle, whose Rot products are float64: forward up to 1.1e-9, backward 430 .. 71 000 P eps on EVERY case
# and both solver paths -- the rounding of the oracle's Rot term, not the solver; see the module docstring).
MEASURED = dict(block_over_scale=2.9e-14, jtr=5.3e-15, batch_against_single_slot=5.6e-17, ranks_against_world1=4.4e-16,
                forward=4.9e-15, backward_in_P_eps=0.042)
# Records.  The project's assembly tolerance for oracle against device is 1e-7 max(1, |A|max) for block entries and 1e-8 for
# J^T r (test_gpu_lm_weights.py, test_gpu_rigid.py).  The figures above are six orders of magnitude below it -- both sides sum
# the same float64 products, only the order differs -- so the bounds here are TIGHTENED to ten times the largest measured
# value: 3e-13 max(1, |A|max) and 6e-14.
RECORD_TOL = dict(block=3e-13, jtr=6e-14)     # block entries: x max(1, |A|max)
FORCE_K4 = (0, 1e30)                          # slm_enable_data_weights: every matched surfel weighs 1
U = 0.37
UNSUPPORTED, INVALID = 5, 1


def _torch():
    import torch
    return torch


def _engine(K, sharded=False, slots=1, **kw):
    from super_amd import _lib
    from super_amd.engine import Engine
    e = Engine(_torch().device("cuda", 0), max_frames=slots, num_iterations=1, **kw)
    if K == 4:
        _lib.check(e.lib.slm_enable_data_weights(e.h, FORCE_K4[0], FORCE_K4[1]), "slm_enable_data_weights")
    if sharded:
        _lib.check(e.lib.slm_set_shard(e.h, 0, 1), "slm_set_shard")
    return e


class _closing:
    def __init__(self, e):
        self.e = e

    def __enter__(self):
        return self.e

    def __exit__(self, *exc):
        self.e.close()


def _bind(e, c, slot=0):
    from super_amd.engine import DeviceFrame
    e.bind(slot, DeviceFrame.from_scene(c.scene, e.device, state_f64=c.state_f64))


def _dev(a, dt):
    return _torch().from_numpy(np.ascontiguousarray(a)).to(device="cuda", dtype=dt)


def _set_beta(e, beta, slot=0):
    from super_amd import _lib
    bt = _dev(beta, _torch().float64)
    _lib.check(e.lib.slm_set_beta(e.h, slot, bt.data_ptr(), e.stream), "slm_set_beta")
    _torch().cuda.synchronize()


def _read_plan(e, what, slot=0):
    from super_amd import _lib
    n = C.c_int64(0)
    _lib.check(e.lib.slm_debug_read_plan(e.h, slot, what, None, 0, C.byref(n), e.stream), "size")
    buf = np.zeros(max(n.value, 4), np.uint8)
    _lib.check(e.lib.slm_debug_read_plan(e.h, slot, what, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n), e.stream), "read")
    return buf[:n.value].copy()


def _assert_plan(e, plan, tag, slot=0):
    """blk_key, sf_pidx, sf_perm (and tri_pidx) of the slot equal the model's, array for array; so does the count of pairs"""
    want = dict(blk_key=plan.blk_key, sf_pidx=plan.sf_pidx, sf_perm=plan.sf_perm)
    want["tri_pidx"] = plan.tri_pidx if plan.tri_pidx is not None else np.zeros((0, 6), np.int32)
    for name, ref in want.items():
        got = _read_plan(e, ppm.WHAT[name], slot)
        assert got.size == ref.nbytes, (tag, name, "bytes", got.size, ref.nbytes)
        np.testing.assert_array_equal(got.view(ref.dtype), ref.reshape(-1), err_msg=f"{tag}: {name}")
    assert e.plan_info(slot)["pairs"] == plan.pairs, tag


def _grad(e, n=1):
    from super_amd import _lib
    _lib.check(e.lib.slm_lm_grad_local(e.h, n, e.stream), "slm_lm_grad_local")


def _records(e, plan, slot=0):
    """(records, matched count) of the slot's SLM_X_PAIR_BLOCKS buffer"""
    from super_amd import _lib
    n = C.c_int64(-1)
    _lib.check(e.lib.slm_lm_exchange_size(e.h, slot, lsc.SLM_X_PAIR_BLOCKS, C.byref(n)), "slm_lm_exchange_size")
    buf = _torch().empty(n.value, dtype=_torch().float64, device="cuda")
    _lib.check(e.lib.slm_lm_exchange_get(e.h, slot, lsc.SLM_X_PAIR_BLOCKS, buf.data_ptr(), e.stream), "slm_lm_exchange_get")
    _torch().cuda.synchronize()
    return ppm.split(buf.cpu().numpy(), plan)


def _compare(tag, plan, got, system):
    """records and matched count against the dense system (A, jtl, M): MEASURE line, then the bounds"""
    rec, M = got
    A, jtl, Mref = system
    want = ppm.records_of(plan, A, jtl)
    assert ppm.covered(plan, A), tag
    eb, ej = ppm.record_errors(plan, rec, want)
    scale = max(1.0, float(np.abs(A).max()))
    print(f"MEASURE {tag} pairs={plan.pairs} M={M:.0f} (model {Mref}) block={eb:.3e} |A|max={scale:.3e} jtr={ej:.3e}")
    assert np.isfinite(rec).all(), tag
    assert M == Mref, (tag, M, Mref)
    assert eb <= RECORD_TOL["block"] * scale, (tag, "block", eb, scale)
    assert ej <= RECORD_TOL["jtr"], (tag, "jtr", ej)


def _between(tag, plan, a, b, scale):
    eb, ej = ppm.record_errors(plan, a, b)
    print(f"MEASURE {tag} between: block={eb:.3e} jtr={ej:.3e}")
    assert eb <= RECORD_TOL["block"] * scale and ej <= RECORD_TOL["jtr"], (tag, eb, ej)


# ======================================================================================================== plan and records
@pytest.mark.parametrize("K", ppc.ALL_K)
def test_plan_equals_the_numpy_construction(K):
    with _closing(_engine(K, sharded=True, use_arap=False, use_rot=False)) as e:
        for name in ppc.names_of(K):
            c = ppc.case(name)
            _bind(e, c)
            _assert_plan(e, c.plan, name)
            _bind(e, c)                                   # ... and again on the slot's grown buffers
            _assert_plan(e, c.plan, name + " (second bind)")


@pytest.mark.parametrize("K", ppc.ALL_K)
def test_records_equal_the_blocks_of_the_oracles_system(K):
    with _closing(_engine(K, sharded=True, use_arap=False, use_rot=False)) as e:
        for name in ppc.names_of(K):
            c = ppc.case(name)
            _bind(e, c)
            for which, beta in ppc.betas(c.scene.J).items():
                _set_beta(e, beta)
                _grad(e)
                _compare(f"{name} {which}", c.plan, _records(e, c.plan), c.system(which))


def test_read_plan_refusals():
    """13..16 on a slot of the tuple-sorted form and 0..12 on a slot of the pair-record form, each with its own text"""
    c4, c6 = ppc.case("run_lengths_k4"), ppc.case("run_lengths_k6")
    n = C.c_int64(0)
    from super_amd.engine import Engine
    with _closing(Engine(_torch().device("cuda", 0))) as e:          # plain K = 4: the tuple-sorted plan
        _bind(e, c4)
        for what in (13, 14, 15, 16):
            assert e.lib.slm_debug_read_plan(e.h, 0, what, None, 0, C.byref(n), e.stream) == UNSUPPORTED
            assert e.lib.slm_last_error() == b"slm_debug_read_plan: the slot has no pair plan"
        assert e.lib.slm_debug_read_plan(e.h, 0, 4, None, 0, C.byref(n), e.stream) == 0 and n.value == 4 * c4.plan.pairs
    with _closing(_engine(6)) as e:
        _bind(e, c6)
        for what in (0, 4, 12, 17, -1):
            assert e.lib.slm_debug_read_plan(e.h, 0, what, None, 0, C.byref(n), e.stream) == UNSUPPORTED
            assert e.lib.slm_last_error() == b"slm_debug_read_plan: the slot has no tuple-sorted plan"
        assert e.lib.slm_debug_read_plan(e.h, 0, 16, None, 0, C.byref(n), e.stream) == 0 and n.value == 0      # no mesh
    with _closing(Engine(_torch().device("cuda", 0))) as e:
        _bind(e, c4)
        assert e.lib.slm_debug_read_plan(e.h, 0, 17, None, 0, C.byref(n), e.stream) == INVALID
        assert e.lib.slm_last_error() == b"slm_debug_read_plan: unknown array"


# ================================================================================================================== solve
@functools.lru_cache(maxsize=None)
def _solve_reference(name):
    """(A + U I, b, delta, norm2) of the oracle's full system at the perturbed beta, Rot products in float32; and the same of
    the plain oracle"""
    c = ppc.case(name)
    beta, opt = ppc.perturbed(c.scene.J), orc.default_opt()
    out = []
    A0, b0, _ = orc.normal_equations(c.fr, beta, orc.default_opt(mesh_rot=False))
    A32, b32 = lsc._rot32(beta, opt.mesh_rot_weight, np.array(A0), np.array(b0))
    for A, b in ((A32, b32), orc.normal_equations(c.fr, beta, opt)[:2]):
        Au = A + U * np.eye(len(b))
        out.append((Au, b, orc.solve_damped(A, b, U), float(np.linalg.norm(Au, 2))))
    return out


@pytest.mark.parametrize("solver_path", (2, 3))
@pytest.mark.parametrize("K", ppc.ALL_K)
def test_one_solve_matches_the_dense_cholesky_solve(K, solver_path):
    from super_amd import _lib
    torch = _torch()
    with _closing(_engine(K, solver_path=solver_path)) as e:
        for name in ppc.names_of(K):
            c = ppc.case(name)
            P = 7 * c.scene.J
            _bind(e, c)
            _set_beta(e, ppc.perturbed(c.scene.J))
            delta = torch.zeros(P, dtype=torch.float64, device="cuda")
            status = torch.full((1,), -7, dtype=torch.int32, device="cuda")
            _lib.check(e.lib.slm_solve(e.h, 0, U, delta.data_ptr(), status.data_ptr(), e.stream), "slm_solve")
            d = delta.cpu().numpy()
            assert int(status.item()) == 0 and np.isfinite(d).all(), (name, int(status.item()))
            (A, b, want, norm2), (Ap, bp, wantp, norm2p) = _solve_reference(name)
            fwd, bwd = float(np.abs(d - want).max()), sgc.backward_error(A, b, d, norm2)
            eps = P * np.finfo(np.float64).eps
            print(f"MEASURE solve {name} sp={solver_path} P={P} forward={fwd:.3e} backward={bwd / eps:.3f} P eps "
                  f"(plain oracle: forward={np.abs(d - wantp).max():.3e} backward={sgc.backward_error(Ap, bp, d, norm2p) / eps:.1f} P eps)")
            np.testing.assert_allclose(d, want, rtol=0, atol=1e-9 * max(1.0, np.abs(want).max()), err_msg=name)
            assert bwd <= sgc.backward_bound(P), (name, bwd / eps)


# ================================================================================================================= shares
@pytest.mark.parametrize("world", (2, 3))
@pytest.mark.parametrize("name", ppc.SHARED)
def test_shares_of_emulated_ranks(name, world):
    c = ppc.case(name)
    assert ppc.boundary_inside_a_run(c, world)
    cfg = FORCE_K4 if c.K == 4 else None
    beta = ppc.perturbed(c.scene.J)
    kw = dict(state_f64=c.state_f64, iters=1, use_arap=False, use_rot=False)
    one = lsc.Ranks([c.scene], cfg, 1, **kw)
    try:
        one.set_beta(beta)
        one.call("slm_lm_grad_local")
        whole, M = ppm.split(one.get(one.es[0], 0, lsc.SLM_X_PAIR_BLOCKS).cpu().numpy(), c.plan)
    finally:
        one.close()
    R = lsc.Ranks([c.scene], cfg, world, **kw)
    try:
        R.set_beta(beta)
        R.call("slm_lm_grad_local")
        parts = [ppm.split(R.get(e, 0, lsc.SLM_X_PAIR_BLOCKS).cpu().numpy(), c.plan) for e in R.es]
    finally:
        R.close()
    for r, (lo, hi) in enumerate(ppc.bounds(c.plan.N, world)):
        _compare(f"{name} W{world} rank {r} [{lo}, {hi})", c.plan, parts[r], c.system("perturbed", lo, hi))
    assert sum(p[1] for p in parts) == M == c.system("perturbed")[2]
    _between(f"{name} W{world} ranks' sum against world 1", c.plan, sum(p[0] for p in parts), whole,
             max(1.0, float(np.abs(c.system("perturbed")[0]).max())))


# =================================================================================================== other users of pair_gram
class _Term:
    """An unsharded handle with ONE opt-in term on the case's frame, ARAP and Rot off"""

    def __init__(self, term, c):
        from super_amd import _lib
        self.c, self.term, self._lib, self.keep = c, term, _lib, []
        torch = _torch()
        e = self.e = _engine(0, use_arap=False, use_rot=False)        # (K = 0: no forcing, the term puts the slot on the pair form)
        J, fr = c.scene.J, c.fr
        self.plan = c.plan
        if term == "corr":
            self.lam, self.targets = 0.8, ppc.corr_targets(c)
            _lib.check(e.lib.slm_enable_corr(e.h, 1, self.lam), "slm_enable_corr")
            _bind(e, c)
            o, n, v = self.targets
            o, n, v = _dev(o, torch.float64), _dev(n, torch.float64), _dev(v, torch.uint8)
            _lib.check(e.lib.slm_bind_corr_points(e.h, 0, o.data_ptr(), n.data_ptr(), v.data_ptr(), e.stream), "slm_bind_corr_points")
        elif term == "hard":
            self.sem, self.pat = ppc.hard_sem(c)
            _lib.check(e.lib.slm_enable_data_weights(e.h, 1, 0.0), "slm_enable_data_weights")
            _bind(e, c)
            s = self.sem
            self.keep = [_dev(s.sf_seg, torch.int32), _dev(s.sf_seg_conf, torch.float32), _dev(s.tgt_seg_conf, torch.float32)]
            _lib.check(e.lib.slm_bind_data_semantic(e.h, 0, 2, *[t.data_ptr() for t in self.keep], e.stream), "slm_bind_data_semantic")
        elif term == "morph":
            self.sem = lmm.sem_of(c.scene)
            self.lam = lmm.visible_weight(fr, self.sem, ppc.perturbed(J), ppc.data_opt())
            _lib.check(e.lib.slm_enable_morph(e.h, self.lam), "slm_enable_morph")
            _bind(e, c)
            s = self.sem
            self.keep = [_dev(s.img_seg, torch.int32), _dev(s.img_seg_conf, torch.float32), _dev(s.sf_seg, torch.int32)]
            counts = (C.c_int32 * 4)()
            _lib.check(e.lib.slm_bind_morph(e.h, 0, s.C, *[t.data_ptr() for t in self.keep], counts, e.stream), "slm_bind_morph")
            assert list(counts)[:s.C] == [len(x) for x in s.edges]
        else:
            assert term == "face"
            self.lam = 3.0          # (the term's largest entry is then of the size of the data term's)
            self.mesh, self.plan = ppc.face_mesh(c)
            _lib.check(e.lib.slm_enable_face(e.h, self.lam), "slm_enable_face")
            tri, areas = _dev(self.mesh[0], torch.int32), _dev(self.mesh[1], torch.float64)
            _lib.check(e.lib.slm_set_face_mesh(e.h, 0, int(tri.shape[1]), tri.data_ptr(), areas.data_ptr(), e.stream), "slm_set_face_mesh")
            torch.cuda.synchronize()
            _bind(e, c)

    def system(self, beta):
        fr, opt = self.c.fr, ppc.data_opt()
        if self.term == "corr":
            return lcm.normal_equations_with_corr(fr, beta, opt, self.targets, 1, self.lam)
        if self.term == "hard":
            ww = lwm.weights(fr, self.sem, beta, 1)
            lwm.check_conditions(ww, 1, 0.0)
            return lwm.normal_equations(fr, self.sem, beta, opt, 1, 0.0)
        if self.term == "morph":
            s = lmm.check_conditions(fr, self.sem, beta)
            assert s.n > 0, "the morph term keeps no surfel"
            return lmm.normal_equations_with_morph(fr, beta, opt, self.sem, self.lam)
        return lfm.normal_equations_with_face(fr, beta, opt, self.mesh, self.lam)


@pytest.mark.parametrize("term", ("corr", "morph", "hard", "face"))
@pytest.mark.parametrize("name", ppc.OTHER_USERS)
def test_other_users_of_the_run_gram(name, term):
    c = ppc.case(name)
    t = _Term(term, c)
    with _closing(t.e) as e:
        _assert_plan(e, t.plan, f"{name} {term}")
        for which, beta in ppc.betas(c.scene.J).items():
            system = t.system(beta)
            plain = c.system(which)
            assert system[2] == plain[2] and np.abs(np.asarray(system[0]) - plain[0]).max() > 0      # the term is visible
            _set_beta(e, beta)
            _grad(e)
            _compare(f"{name} {term} {which}", t.plan, _records(e, t.plan), system)


# ================================================================================================================== batch
@pytest.mark.parametrize("K", sorted(ppc.BATCHES))
def test_a_batch_of_unlike_frames_equals_its_single_slots(K):
    cs = [ppc.case(n) for n in ppc.BATCHES[K]]
    beta = ppc.perturbed(cs[0].scene.J)
    single = []
    with _closing(_engine(K, sharded=True, use_arap=False, use_rot=False)) as e:
        for c in cs:
            _bind(e, c)
            _set_beta(e, beta)
            _grad(e)
            single.append(_records(e, c.plan))
    with _closing(_engine(K, sharded=True, slots=3, use_arap=False, use_rot=False)) as e:
        for i, c in enumerate(cs):
            _bind(e, c, i)
            _set_beta(e, beta, i)
        _grad(e, 3)
        for i, c in enumerate(cs):
            got = _records(e, c.plan, i)
            _assert_plan(e, c.plan, f"batch K={K} slot {i}", i)
            _compare(f"batch K={K} slot {i} {c.name}", c.plan, got, c.system("perturbed"))
            assert got[1] == single[i][1]
            _between(f"batch K={K} slot {i} {c.name} against its single slot", c.plan, got[0], single[i][0],
                     max(1.0, float(np.abs(c.system("perturbed")[0]).max())))


# ----------------------------------------------------------------------------------------------------------------- RECORD
# One run of this file on an MI355X found no defect in prep_pairs, pair_gram, k_pair_scatter's inputs or the share bounds: every
# plan array equalled the NumPy construction, every matched count was exact, every record within MEASURED.
#
# Two scratch builds with a deliberately wrong run mask in pair_gram (slm_pairs.h; never committed), the records comparison of
# test_records_equal_the_blocks_of_the_oracles_system run case by case over all 79 cases:
#   `q < qe` -> `q <= qe` (a straddling k-step lets the NEXT run's first row into this run's masked operand):
#       one_set 47 of 47 pass (a wave is one run: the row behind it is a zero row or the next wave's);  all_distinct 0 of 8,
#       run_lengths 0 of 9, holes_in_runs 0 of 8, shared_prefix 0 of 3, shuffled 0 of 2, far_pairs 0 of 2 pass, e.g.
#       ('run_lengths_k6 perturbed', 'block', 0.2878, 1.512): a block entry off by 0.29 at |A|max = 1.5.
#   `q >= qs` -> `q > qs` (the first row of every run is masked out of one operand, so its outer product is lost):
#       every family fails, one_set included (0 of 47; ('one_set_n1_k1 perturbed', 'block', 0.6663, 1.0)) -- the first row of a
#       wave's only run is lost like any other run's, so this defect cannot pass one_set.
