"""The float64 model of the LM path's semantic boundary-morph term (tests/lm_morph_model.py) checked on the CPU: its loss
against ``graphfit_oracle.bn_morph`` (the reference-pinned oracle) at the same deformed positions, its Jacobian against
central differences with the selection frozen, and the properties the GPU tests (tests/test_gpu_lm_morph.py) rely on -- the
conditions under which a device and the model take the same side of every decision hold at every beta those tests visit, no
accept decision of their traces is a rounding-level tie, the kept count changes along a trace and a trace holds a reject,
and the weight rule that keeps the term a visible, not a swamping, part of the system.  The scenes, inputs and weights of the
GPU tests are defined here."""
import numpy as np
import pytest
import torch

import lm_morph_model as lmm
from oracle import graphfit_oracle as gfo
from oracle import lm_oracle as orc
from super_amd import synth

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


# ---- the scenes of the GPU tests ---------------------------------------------------------------------------------------
SHIFT = 6.0                       # make_scene's default: the target segmentation is the source's moved 6 px
SIZES = {4: (1200, 40), 6: (1200, 40), 3: (400, 24), 1: (400, 24)}
# boundary-list length, candidates and kept surfels per class at identity (classes 1 and 2; class 0 has no candidate)
AT_IDENTITY = {4: {1: (151, 107, 35), 2: (77, 113, 39)}, 6: {1: (151, 98, 36), 2: (77, 118, 40)}}


def scene_k(K, shift=SHIFT):
    """N surfels, J nodes (SIZES), ``num_neighbors`` K, three classes, the target segmentation moved ``shift`` px: the
    geometry of tests/test_lm_face_model.scene_k (it does not depend on the semantic arguments)"""
    N, J = SIZES[K]
    return _cached(("k", K, shift), lambda: synth.make_scene(N=N, J=J, H=60, W=80, seed=60 + K, n_neighbors=K, src_border=4,
                                                             tgt_border=3, tgt_holes=0.01, semantic=True, num_classes=3,
                                                             seg_shift=shift))


def frame_of(sc):
    return orc.Frame.from_scene(sc)


def identity(J):
    return np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (J, 1))


def ref_beta(J):
    return lmm.random_beta(J, 17, rot=0.01, trans=0.002)


def sem_k(K, kind=SHIFT):
    """the term's inputs of the GPU tests on scene_k(K): a number = make_scene's inputs at that ``seg_shift``; ``"none"`` =
    inputs without a candidate (below); ``"ring"`` = the hand-made ``img_seg`` of the search-shape test (below)"""
    def make():
        sc = scene_k(K)
        if kind == "none":
            # seg_shift 0 leaves 17 candidates (none kept): surfels within a pixel of a class boundary, whose class is the
            # ROUNDED pixel's while the term samples bilinearly.  No candidates at all: the surfels' classes are taken from
            # the image the term samples, at identity.
            s0 = lmm.sem_of(scene_k(K, 0.0))
            fr = frame_of(sc)
            x, y, _ = lmm.project(fr, np.asarray(fr.sf_points, dtype=np.float64))
            conf, _ = lmm.sampled_conf(fr, s0, x, y)
            return lmm.sem_of(sc, img_seg=s0.img_seg, img_seg_conf=s0.img_seg_conf, sf_seg=np.argmax(conf, axis=1))
        if kind == "ring":
            # img_seg: class 1 everywhere but ONE pixel of class 2 -- class 2 has exactly one boundary pixel (no boundary by
            # the term's rule), class 0 is absent from the image, class 1's list is the ring of eight pixels around that one
            # (shorter than a wave).  img_seg_conf stays the scene's, so the mismatching surfels are the same (classes 1
            # and 2): those of class 1 are pulled to the ring, those of class 2 are no candidates.
            seg = np.ones((sc.H, sc.W), dtype=np.int64)
            seg[30, 36] = 2
            return lmm.sem_of(sc, img_seg=seg)
        return lmm.sem_of(scene_k(K, float(kind)))
    return _cached(("sem", K, kind), make)


def outside_beta(K):
    """identity plus one translation of every node along x that moves the projections ~10 px to the right: the right-most
    surfels (src_border 4) project past the image's edge"""
    sc = scene_k(K)
    fx = float(np.float32(sc.K[0, 0]))
    z = float(np.asarray(sc.sf_points, dtype=np.float64)[:, 2].mean())
    beta = identity(sc.J)
    beta[:, 4] = 10.0 * z / fx
    return beta


def weight_of(K, kind=SHIFT):
    """the weight rule of the GPU tests: lambda from the model such that the largest entry of the term's J^T J equals the
    largest entry of the data term's at the reference beta"""
    sc = scene_k(K)
    return _cached(("lam", K, kind), lambda: lmm.visible_weight(frame_of(sc), sem_k(K, kind), ref_beta(sc.J), orc.default_opt()))


# (K, weight factor, u0, v) of every GPU trace: the weight is factor x weight_of(K).  The term's loss is not continuous (the
# selection changes with beta, and a surfel that has come within sqrt(15) px of its boundary leaves it), so every one of
# these traces holds rejects; the last is the default damping.
DAMPING = (100.0, 2.0)
TRACE_CASES = [(4, 1.0) + DAMPING, (6, 1.0) + DAMPING, (4, 3.0) + DAMPING, (6, 3.0) + DAMPING, (4, 1.0, 10.0, 7.5)]


def trace_of(K, factor, u, v, kind=SHIFT):
    def make():
        sc = scene_k(K)
        trace = []
        beta = lmm.lm_with_morph(frame_of(sc), orc.default_opt(), None if kind is None else sem_k(K, kind), factor * weight_of(K),
                                 u=u, v=v, trace=trace)
        return beta, trace
    return _cached(("trace", K, factor, u, v, kind), make)


# The eight-slot test runs ONE solver, so one weight (weight_of(BATCH_K)), over unlike inputs: make_scene's at these shifts
# (None: a slot without inputs), damping DAMPING.  Its single-slot runs are GPU traces too.
BATCH_K = 4
BATCH_KINDS = [6.0, 9.0, 12.0, None, 9.0, 6.0, 12.0, 6.0]


def batch_trace_of(kind):
    return trace_of(BATCH_K, 1.0, *DAMPING, kind=kind)


def visited(trace):
    """every beta a GPU run of the trace evaluates the term at: the point of each Jacobian pass and each trial point"""
    return [b for t in trace for b in (t["beta_at"], t["beta_trial"])]


# ---- the model itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 6])
def test_counts_at_identity(K):
    sc = scene_k(K)
    sem = sem_k(K)
    s = lmm.check_conditions(frame_of(sc), sem, identity(sc.J))
    got = {c: (len(sem.edges[c]), int((s.cand & (sem.sf_seg == c)).sum()), int((s.kept & (sem.sf_seg == c)).sum())) for c in (1, 2)}
    assert got == AT_IDENTITY[K] and not (s.cand & (sem.sf_seg == 0)).any()
    small = scene_k(3)
    s3 = lmm.select(frame_of(small), sem_k(3), identity(small.J))
    assert [int((s3.kept & (sem_k(3).sf_seg == c)).sum()) for c in range(3)] == [0, 11, 9]
    assert lmm.select(frame_of(sc), sem_k(K, 9.0), identity(sc.J)).n >= 2 * s.n      # seg_shift 9 doubles the kept count


@pytest.mark.parametrize("K", [4, 6])
def test_loss_equals_graphfit_oracle_with_the_squared_weight(K):
    """lambda^2 x ``gfo.bn_morph`` on the oracle's Problem at the same deformed positions"""
    sc = scene_k(K)
    fr, sem, lam = frame_of(sc), sem_k(K), 1.3
    pb = gfo.Problem(sc)
    for beta in (identity(sc.J), ref_beta(sc.J), lmm.random_beta(sc.J, 5, rot=0.03, trans=0.01)):
        T, _ = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, beta)
        ref = float(gfo.bn_morph(pb, torch.from_numpy(T)))
        mine, n, cand = lmm.morph_loss(fr, sem, beta, lam)
        assert n == sum(st[3] for st in pb.morph_stats) > 0 and cand == sum(st[2] for st in pb.morph_stats)
        np.testing.assert_allclose(mine, lam ** 2 * ref, rtol=1e-12)


def test_jacobian_matches_central_differences_with_the_selection_frozen():
    sc = scene_k(4)
    fr, sem, lam = frame_of(sc), sem_k(4), 0.37
    beta = lmm.random_beta(sc.J, 5)
    sel = lmm.select(fr, sem, beta)
    Jd, r = lmm.morph_jacobian(fr, sem, beta, lam, sel)
    assert Jd.shape == (2 * sel.n, 7 * sc.J) and sel.n > 20 and np.abs(r).max() > 0
    h = 1e-6
    for col in range(0, 7 * sc.J, 3):
        d = np.zeros(7 * sc.J)
        d[col] = h
        rp = lmm.morph_jacobian(fr, sem, beta + d.reshape(-1, 7), lam, sel)[1]
        rm = lmm.morph_jacobian(fr, sem, beta - d.reshape(-1, 7), lam, sel)[1]
        np.testing.assert_allclose(Jd[:, col], (rp - rm) / (2 * h), rtol=0, atol=1e-7 * max(1.0, np.abs(Jd).max()))
    assert (Jd != 0).sum(1).max() <= 7 * 4
    # the loss is the sum of the squared residuals plus the constant |e1 - e2|^2 / 4 of every kept surfel
    loss = lmm.morph_loss(fr, sem, beta, lam)[0]
    assert (r ** 2).sum() < loss
    for c in (1, 2):
        k = np.nonzero(sel.kept & (sem.sf_seg == c))[0]
        E = sem.edges[c]
        for i in k[:5]:
            d2 = ((E - [sel.x[i], sel.y[i]]) ** 2).sum(1)
            e1, e2 = E[np.argsort(d2, kind="stable")[:2]]
            np.testing.assert_allclose(sel.li[i], ((sel.x[i] - sel.target[i, 0]) ** 2 + (sel.y[i] - sel.target[i, 1]) ** 2)
                                       + ((e1 - e2) ** 2).sum() / 4.0, rtol=1e-12)


def test_no_kept_surfel_means_no_term():
    sc = scene_k(4)
    fr, sem = frame_of(sc), sem_k(4, "none")
    assert lmm.morph_loss(fr, sem, identity(sc.J), 2.0) == (0.0, 0, 0)
    A, b = lmm.morph_system(fr, sem, identity(sc.J), 2.0)
    assert not A.any() and not b.any()
    assert lmm.morph_loss(fr, None, identity(sc.J), 2.0) == (0.0, 0, 0)


# ---- what the GPU tests rely on ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [4, 6])
def test_weight_rule_keeps_the_term_within_ten_times_the_data_term(K):
    sc = scene_k(K)
    fr, sem, beta = frame_of(sc), sem_k(K), ref_beta(sc.J)
    data_max = np.abs(orc.normal_equations(fr, beta, orc.default_opt(mesh_arap=False, mesh_rot=False))[0]).max()
    at_one = np.abs(lmm.morph_system(fr, sem, beta, 1.0)[0]).max()
    print("largest entries: data", data_max, "term at weight 1", at_one, "lambda", weight_of(K))
    assert at_one > 10.0 * data_max                                   # in pixel units the term swamps the data term at weight 1
    for factor in sorted({c[1] for c in TRACE_CASES if c[0] == K}):
        got = np.abs(lmm.morph_system(fr, sem, beta, factor * weight_of(K))[0]).max()
        assert 0.1 * data_max <= got <= 10.0 * data_max
    for kind in (9.0, 12.0):                                          # the batch's other inputs at the batch's one weight
        got = np.abs(lmm.morph_system(fr, sem_k(K, kind), beta, weight_of(K))[0]).max()
        assert 0.1 * data_max <= got <= 10.0 * data_max


@pytest.mark.parametrize("K", [4, 6, 3, 1])
def test_conditions_hold_at_the_reference_beta(K):
    sc = scene_k(K)
    s = lmm.check_conditions(frame_of(sc), sem_k(K), ref_beta(sc.J))
    assert s.n >= 10
    if K == 4:
        for kind in (9.0, 12.0, "none", "ring"):
            lmm.check_conditions(frame_of(sc), sem_k(K, kind), ref_beta(sc.J))


@pytest.mark.parametrize("K,factor,u,v", TRACE_CASES)
def test_the_gpu_traces_are_decided_everywhere(K, factor, u, v):
    """the conditions at every beta of the trace, no accept decision a rounding-level tie, a kept count that changes and a
    reject"""
    sc = scene_k(K)
    fr, sem = frame_of(sc), sem_k(K)
    beta, trace = trace_of(K, factor, u, v)
    assert len(trace) == 10 and all("loss" in t for t in trace)
    for b in visited(trace):
        lmm.check_conditions(fr, sem, b)
    m = lmm.decision_margins(trace)
    acc = [t["accepted"] for t in trace]
    kept = [t["kept"] for t in trace]
    print("accepted", acc, "kept", kept, "kept at the trial points", [t["kept_trial"] for t in trace], "margins", m)
    assert (m > 1e-6).all()
    assert len(set(kept)) > 1 and not all(acc) and acc[0]
    without = orc.lm(fr, orc.default_opt(), u=u, v=v)
    assert np.abs(beta - without).max() > 1e-6                        # the term moves the solution


@pytest.mark.parametrize("kind", [6.0, 9.0, 12.0, None])
def test_the_batch_traces_are_decided_everywhere(kind):
    assert set(BATCH_KINDS) == {6.0, 9.0, 12.0, None}
    sc = scene_k(BATCH_K)
    beta, trace = batch_trace_of(kind)
    m = lmm.decision_margins(trace)
    print(kind, "accepted", [t["accepted"] for t in trace], "kept", [t["kept"] for t in trace], "margins", m)
    assert len(trace) == 10 and (m > 1e-6).all()
    if kind is not None:
        for b in visited(trace):
            lmm.check_conditions(frame_of(sc), sem_k(BATCH_K, kind), b)
        assert trace[0]["kept"] > 0


def test_without_candidates_the_trace_is_the_plain_one():
    sc = scene_k(4)
    fr, sem = frame_of(sc), sem_k(4, "none")
    u, v = DAMPING
    beta, trace = trace_of(4, 1.0, u, v, kind="none")
    for b in visited(trace):
        assert lmm.check_conditions(fr, sem, b).n == 0
    plain = orc.lm(fr, orc.default_opt(), u=u, v=v)
    np.testing.assert_array_equal(beta, plain)
    assert (lmm.decision_margins(trace) > 1e-6).all()


def test_search_shapes_are_decided():
    """the inputs of the GPU test of the search's edge shapes: the ring (a class with one boundary pixel, a class absent, a
    list shorter than a wave), projections outside the image, and the short-list scene of tests/gf_shape_cases.py"""
    import gf_shape_cases as shapes
    sc = scene_k(4)
    fr = frame_of(sc)
    ring = sem_k(4, "ring")
    assert [len(e) for e in ring.edges] == [0, 8, 1]
    s = lmm.check_conditions(fr, ring, ref_beta(sc.J))
    print("ring: candidates", int(s.cand.sum()), "kept", s.n)
    assert s.n > 0 and not (s.cand & (ring.sf_seg != 1)).any()
    assert (lmm.select(fr, sem_k(4), ref_beta(sc.J)).cand & (ring.sf_seg == 2)).any()
    s = lmm.check_conditions(fr, sem_k(4), outside_beta(4))
    assert 10 < (~s.inside).sum() < sc.N // 2 and s.n > 0 and not (s.cand & ~s.inside).any()
    short = shapes.short_list_scene()
    sem = lmm.sem_of(short)
    s = lmm.check_conditions(frame_of(short), sem, identity(short.J))
    assert len(sem.edges[2]) == 12 and s.n > 0
    full = [b for b in range(0, short.N - 255, 256) if s.cand[b:b + 256].all()]
    assert full                                                       # a workgroup whose 256 threads are all candidates


def test_combined_traces_are_decided_too():
    import lm_corr_model as lcm
    import lm_face_model as lfm
    import lm_weight_model as lwm
    sc = scene_k(4)
    fr, sem, lam, opt = frame_of(sc), sem_k(4), weight_of(4), orc.default_opt()
    u, v = DAMPING
    for name, base in combined_bases(sc).items():
        trace = []
        lmm.lm_with_morph(fr, opt, sem, lam, u=u, v=v, trace=trace, base=base)
        for b in visited(trace):
            lmm.check_conditions(fr, sem, b)
        print(name, [t["accepted"] for t in trace], lmm.decision_margins(trace))
        assert (lmm.decision_margins(trace) > 1e-6).all(), name


def combined_bases(sc):
    """the combinations of the GPU test: correspondences in mode 2, hard semantic weights, the face term"""
    import lm_corr_model as lcm
    import lm_face_model as lfm
    import lm_weight_model as lwm
    fr, opt = frame_of(sc), orc.default_opt()
    tg = corr_targets(sc)
    mesh = lfm.scene_mesh(sc)
    return {"corr": lmm.base_corr(fr, opt, tg, 2, 0.5), "hard": lmm.base_weighted(fr, opt, lwm.sem_of(sc), 1),
            "face": lmm.base_face(fr, opt, mesh, face_weight(sc))}


def corr_targets(sc):
    import lm_corr_model as lcm
    return _cached(("tg", id(sc)), lambda: lcm.targets_from_flow(frame_of(sc), synth.smooth_flow(sc.H, sc.W, 24, amp=(2.0, 1.5))))


def face_weight(sc):
    import lm_face_model as lfm
    return _cached(("lamf", id(sc)), lambda: lfm.visible_weight(frame_of(sc), lfm.scene_mesh(sc), ref_beta(sc.J), orc.default_opt()))
