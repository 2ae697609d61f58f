"""The opt-in terms of the rigid stage (slm_rigid_set_terms: flow-correspondence rows and per-residual data weights;
RigidAlign(corr_term=, weighted_data=), LM_Solver(rigid_terms=True)) on the GPU against the models of
tests/lm_weight_model.py and tests/lm_corr_model.py on the one-node frame of tests/rigid_model.py.

Shapes (tests/rigid_terms_cases.py).  k_rg_pass sums every 256 consecutive surfels into one partial and launches at most 512
workgroups per frame: N = 65 is one past a wave, N = 257 a second partial, N = 3000 twelve partials with a ragged last one,
N = 512 * 256 + 300 a second chunk of the grid-stride walk through the new accumulators.  60 x 80 / 96 x 128 semantic scenes
(the large one 480 x 640: a smaller image does not hold that many surfels), float64 and float32 state.

Tolerances.  Assembly: those of tests/test_gpu_rigid.py -- JtJ atol 1e-7 max(1, |A|max), jtl atol 1e-8, loss rtol 1e-8, counts
exact.  Loop records: accepted / M_grad / M_loss / u exact, loss rtol 1e-9.  Final raw beta_g: BETA_TOL below, ten times the
largest max|beta_dev - beta_model| measured on an MI355X over the loop fixtures of this file (LOOP_CASES at 4 and at 10
iterations, the train phase, the edge loops); every measured value is printed before it is asserted.  The reference is the
model, never the device.  tests/test_rigid_terms_model.py pins on the CPU that the fixtures meet the conditions under which a
device and the model must decide alike."""
import ctypes as C

import numpy as np
import pytest

import lm_corr_model as lcm
import rigid_model as rm
import rigid_terms_cases as rc
from helpers import ref_opt, torch_frame
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

# Measured on an MI355X, max|beta_dev - beta_model| per fixture, at 4 / 10 iterations: n3000 f64 point-point hard 2.2e-17 /
# 4.9e-17; n3000 f32 point-plane soft 4.1e-18 / 2.0e-17; n65 point-plane 9.8e-19 / 1.3e-17; issue scene exact targets 4.1e-18 /
# 2.0e-16; n257 truncated 1.4e-16 / 1.4e-16; n3000 truncated, weight 0.3 8.4e-16 / 8.4e-16 (its first step is the only one it
# keeps for seven iterations); train phase 1.7e-18; no valid correspondence 4.8e-18; all weights zero 1.6e-19; N = 1 3.9e-20.
# The largest is 8.379e-16.  Ten times that:
BETA_TOL = 8.4e-15

ASM_ATOL_A, ASM_ATOL_B, ASM_RTOL_LOSS = 1e-7, 1e-8, 1e-8


# ---------------------------------------------------------------------------------------------------- fixtures
def objects(name, f64=True, labels="own"):
    """sf / inputs / new_data on the device with the semantic fields; float32 state: the model's points rounded"""
    import torch
    sc = rc.scene(name)[0]
    sf, inputs, nd = torch_frame(sc)
    sf.points = torch.from_numpy(np.ascontiguousarray(rc.points(name, f64))).cuda().to(torch.float64 if f64 else torch.float32)
    s = rc.sem(name, labels)
    sf.seg = torch.from_numpy(s.sf_seg).cuda()
    sf.seg_conf = torch.from_numpy(s.sf_seg_conf).cuda()
    nd.seg_conf = torch.from_numpy(s.tgt_seg_conf).cuda()
    return sf, inputs, nd


def options(mode=0, weights="none", lam=1.0, n_iter=10, phase="test", base=None):
    o = ref_opt(base if base is not None else rm.rigid_opt(num_optimize_iterations=n_iter, phase=phase))
    o.sf_corr, o.sf_corr_weight = mode != 0, lam
    o.sf_corr_loss_type = "point-plane" if mode == 2 else "point-point"
    o.sf_hard_seg_point_plane, o.sf_soft_seg_point_plane = weights == "hard", weights == "soft"
    o.depth_model = "raft_stereo" if weights == "trunc" else "monodepth2"
    return o


def aligner(c, max_frames=1, n_iter=10, phase="test"):
    from super_amd.rigid import RigidAlign
    return RigidAlign(options(c.mode, c.weights, c.lam, n_iter, phase), max_frames=max_frames, corr_term=c.mode != 0,
                      weighted_data=c.weights != "none")


def triple(tg):
    import torch
    o, n, valid = tg
    return (torch.from_numpy(np.ascontiguousarray(o)).cuda(), torch.from_numpy(np.ascontiguousarray(n)).cuda(),
            torch.from_numpy(valid.astype(np.uint8)).cuda())


def corr_of(c):
    return None if c.mode == 0 else triple(c.corr[0])


def flow_of(name):
    import torch
    return torch.from_numpy(rc.flow(name)).cuda()


def check_records(recs, trace):
    assert len(recs) == len(trace)
    for r, t in zip(recs, trace):
        assert r["status"] == 0
        assert (r["accepted"], r["M_grad"], r["M_loss"]) == (t["accepted"], t["M_grad"], t["M_loss"]), (r, t)
        assert r["u"] == t["u"], (r["u"], t["u"])
        np.testing.assert_allclose(r["loss"], t["loss"], rtol=1e-9, atol=0)


def check_assembly(c, ra, frame, betas=(rm.IDENTITY, rm.displaced_beta())):
    for beta in betas:
        jtj, jtl, loss, M = ra.assemble(*frame, beta, corr_points=corr_of(c))
        A, b, Mo, lo, split = rc.system(c, beta)
        got = ra.last_assemble_terms
        print(f"{c.id}: M={M} |dA|={np.abs(jtj.cpu().numpy() - A).max():.3e} of {np.abs(A).max():.3e}, "
              f"|db|={np.abs(jtl.cpu().numpy() - b).max():.3e}, loss {loss!r} vs {lo!r}, terms {got} vs {split}")
        assert M == Mo
        np.testing.assert_allclose(jtj.cpu().numpy(), A, rtol=0, atol=ASM_ATOL_A * max(1.0, np.abs(A).max()))
        np.testing.assert_allclose(jtl.cpu().numpy(), b, rtol=0, atol=ASM_ATOL_B)
        np.testing.assert_allclose(loss, lo, rtol=ASM_RTOL_LOSS, atol=0)
        assert (got[1], got[3]) == (split[1], split[3])
        np.testing.assert_allclose([got[0], got[2]], [split[0], split[2]], rtol=ASM_RTOL_LOSS, atol=1e-300)


def run_loop(c, n_iter, phase="test", frame=None):
    import torch
    frame = frame or objects(c.name, c.f64, c.labels)
    ra = aligner(c, n_iter=n_iter, phase=phase)
    tg = ra.align(*frame, u=c.u, v=c.v, corr_points=corr_of(c))
    beta = ra.beta(0).cpu().numpy()
    want, trace, _ = rc.loop(c, n_iter, phase)
    err = float(np.abs(beta - want).max())
    print(f"rigid terms run {c.id} iters={n_iter} phase={phase}: max|beta_dev - beta_model| = {err:.3e}; losses "
          f"{[r['loss'] for r in ra.last_records[0]]}; terms {ra.last_terms[0]}")
    torch.cuda.synchronize()
    return ra, tg.cpu().numpy(), beta, want, trace, err


# ---------------------------------------------------------------------------------------------------- 1. assembly
@pytest.mark.parametrize("weights", ["none", "hard", "soft", "trunc"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name,f64", [("n3000", True), ("n3000", False), ("n65", True), ("n257", True)])
def test_assemble_matches_the_model_system(name, f64, mode, weights):
    c = rc.Case(name, f64, mode, weights, 0.7)
    check_assembly(c, aligner(c), objects(name, f64))


def test_assemble_walks_a_second_chunk_through_the_new_accumulators():
    c = rc.Case("big", True, 1, "hard", 0.7)
    check_assembly(c, aligner(c), objects("big"), betas=(rm.displaced_beta(),))


# ---------------------------------------------------------------------------------------------------- 2. the loop
@pytest.mark.parametrize("n_iter", [4, 10])
@pytest.mark.parametrize("c", rc.LOOP_CASES, ids=lambda c: c.id)
def test_run_matches_the_model_trace(c, n_iter):
    ra, tg, beta, want, trace, err = run_loop(c, n_iter)
    check_records(ra.last_records[0], trace)
    assert err <= BETA_TOL, err
    np.testing.assert_allclose(tg, rm.normalised(want), rtol=0, atol=BETA_TOL)
    A, b, M, lo, split = rc.system(c, beta)                       # the kept sums are those of the final beta
    got = ra.last_terms[0]
    assert (got[1], got[3]) == (split[1], split[3])
    np.testing.assert_allclose([got[0], got[2]], [split[0], split[2]], rtol=1e-8, atol=1e-300)


def test_train_phase_always_accepts():
    c = rc.TRAIN_CASE
    ra, tg, beta, want, trace, err = run_loop(c, 4, phase="train")
    check_records(ra.last_records[0], trace)
    assert all(r["accepted"] and r["u"] == c.u for r in ra.last_records[0])
    assert err <= BETA_TOL, err


def test_known_warp_ends_where_the_cpu_figures_say():
    """the pan along the surface: the plain stage slides, point-point rows on every third surfel fix it (default damping; the
    converged iterations' accept flags are rounding-level ties, the place the model ends at is not)"""
    frame = objects("issue")
    for label, c in (("plain", rc.Case("issue", True, 0)), ("pp_w3", rc.Case("issue", True, 1, "none", 3.0, "exact")),
                     ("pp_w10", rc.Case("issue", True, 1, "none", 10.0, "exact")),
                     ("plane_w1", rc.Case("issue", True, 2, "none", 1.0, "exact"))):
        ra = aligner(c)
        ra.align(*frame, corr_points=corr_of(c))
        got, want = rc.rms_mm("issue", ra.beta(0).cpu().numpy()), rc.KNOWN_WARP[label]
        print(f"known warp {label}: {got:.4f} mm (CPU figure {want})")
        assert abs(got - want) <= 0.006 * max(1.0, want), (label, got, want)


# ---------------------------------------------------------------------------------------------------- 3. selection edges
@pytest.mark.parametrize("i", [0, 255, 256, -1])
def test_exactly_one_valid_correspondence(i):
    c = rc.Case("n3000", True, 1, "none", 0.7, ("one", i))
    ra = aligner(c)
    check_assembly(c, ra, objects("n3000"))
    assert ra.last_assemble_terms[3] == 1


def test_no_valid_correspondence_equals_the_plain_model():
    ra, tg, beta, want, trace, err = run_loop(rc.NONE_CASE, 4)
    plain, ptrace, _ = rc.loop(rc.PLAIN_CASE, 4)
    check_records(ra.last_records[0], ptrace)
    assert np.abs(beta - plain).max() <= BETA_TOL
    assert ra.last_terms[0][2:] == (0.0, 0)


@pytest.mark.parametrize("mode,weights", [(1, "hard"), (2, "none")])
def test_surfels_with_one_term_only_on_the_holes_scene(mode, weights):
    c = rc.Case("holes", True, mode, weights, 0.7)
    valid = c.corr[0][2]
    matched = np.zeros(len(valid), bool)
    matched[orc.data_term(rc.frame("holes"), rm.IDENTITY[None, :], 1.0).match] = True
    assert (valid & ~matched).any() and (matched & ~valid).any()
    check_assembly(c, aligner(c), objects("holes"))


def test_every_matched_surfel_at_weight_zero_beside_valid_correspondences():
    ra, tg, beta, want, trace, err = run_loop(rc.OFF_CASE, 4)
    check_records(ra.last_records[0], trace)
    assert all(r["M_grad"] > 0 and r["M_loss"] > 0 for r in ra.last_records[0])
    data, M, corr, kept = ra.last_terms[0]
    assert data == 0.0 and M > 0 and corr > 0.0 and kept > 0
    assert err <= BETA_TOL, err


def test_one_surfel():
    ra, tg, beta, want, trace, err = run_loop(rc.ONE_SURFEL_CASE, 4)
    check_records(ra.last_records[0], trace)
    assert trace[0]["M_grad"] == 1 and ra.last_terms[0][3] == 1
    assert err <= BETA_TOL, err


# ---------------------------------------------------------------------------------------------------- 4. nothing moved
def _bits(ra, frame, **kw):
    ra.align(*frame, **kw)
    out = (ra.beta(0).cpu().numpy().tobytes(), ra.last_records[0])
    j = ra.assemble(*frame, rm.displaced_beta(), **kw)
    return out + (j[0].cpu().numpy().tobytes(), j[1].cpu().numpy().tobytes(), j[2], j[3])


def test_without_terms_the_stage_gives_the_bits_of_the_plain_stage():
    from super_amd.rigid import RigidAlign
    frame = objects("n3000")
    plain = _bits(RigidAlign(options(n_iter=4)), frame)                       # never called slm_rigid_set_terms
    ra = RigidAlign(options(n_iter=4))
    assert ra.lib.slm_rigid_set_terms(ra.h, 1, 0.7, 1, 0.0) == 0
    assert ra.lib.slm_rigid_set_terms(ra.h, 0, 0.0, 0, 0.0) == 0
    assert _bits(ra, frame) == plain                                          # after (0, 0, 0, 0)
    for mode in (1, 2):
        c = rc.Case("n3000", True, mode, "none", 0.7)
        assert _bits(aligner(c, n_iter=4), frame) == plain, mode              # a slot without inputs, the term enabled
        ra = aligner(c, max_frames=2, n_iter=4)                               # ... beside a slot WITH inputs (same launch)
        ra.align_batch([frame + (corr_of(c),), frame])
        assert (ra.beta(1).cpu().numpy().tobytes(), ra.last_records[1]) == plain[:2], mode


def test_two_runs_with_terms_give_the_same_bits():
    frame = objects("n3000")
    for c in (rc.Case("n3000", True, 1, "soft", 0.7), rc.Case("n3000", True, 2, "trunc", 0.7)):
        a = _bits(aligner(c, n_iter=4), frame, corr_points=corr_of(c))
        ra = aligner(c, n_iter=4)
        assert _bits(ra, frame, corr_points=corr_of(c)) == a
        assert _bits(ra, frame, corr_points=corr_of(c)) == a                  # and the same context again
        assert a[1][-1]["M_grad"] > 0


# ---------------------------------------------------------------------------------------------------- 5. batches
def test_a_batch_of_three_equals_the_three_single_runs():
    c = rc.Case("n3000", True, 1, "hard", 0.7)
    frames = [objects("n3000") + (flow_of("n3000"),), objects("n257") + (triple(rc.targets("n257")),), objects("n65") + (None,)]
    ra = aligner(c, max_frames=3, n_iter=4)
    ra.align_batch(frames)
    for i, fr in enumerate(frames):
        one = aligner(c, n_iter=4)
        kw = {} if fr[3] is None else (dict(flow=fr[3]) if not isinstance(fr[3], tuple) else dict(corr_points=fr[3]))
        one.align(*fr[:3], **kw)
        assert ra.beta(i).cpu().numpy().tobytes() == one.beta(0).cpu().numpy().tobytes(), i
        assert ra.last_records[i] == one.last_records[0] and ra.last_terms[i] == one.last_terms[0], i
    assert ra.last_terms[0][3] > 2000 and ra.last_terms[1][3] > 200 and ra.last_terms[2][3] == 0
    with pytest.raises(ValueError):
        ra.align_batch(frames + frames)


# ---------------------------------------------------------------------------------------------------- 6. targets
@pytest.mark.parametrize("name,f64", [("n3000", True), ("n3000", False), ("holes", True)])
def test_targets_from_a_flow_match_the_model(name, f64):
    c = rc.Case(name, f64, 1)
    go, gn, gv = (t.cpu().numpy() for t in aligner(c).corr_targets(*objects(name, f64), flow_of(name)))
    o, n, valid = rc.targets(name, f64)
    tie = lcm.tie_distance(rc.frame(name, f64), rc.flow(name)) <= 1e-4
    print(name, f64, "kept", int(gv.sum()), "model", int(valid.sum()), "excluded", int(tie.sum()))
    assert tie.sum() <= 5
    np.testing.assert_array_equal(gv[~tie].astype(bool), valid[~tie])
    both = ~tie & valid
    np.testing.assert_allclose(go[both], o[both], rtol=0, atol=2e-7 * np.abs(o).max())     # the float32 flow sample
    np.testing.assert_allclose(gn[both], n[both], rtol=0, atol=2e-7 * np.abs(n).max())
    assert (go[~gv.astype(bool)] == 0).all() and (gn[~gv.astype(bool)] == 0).all()


def _node_opt(mode=1, weights="hard", lam=0.05, n_iter=3):
    return options(mode, weights, lam, base=orc.default_opt(num_optimize_iterations=n_iter))


@pytest.mark.parametrize("f64", [True, False])
def test_targets_equal_the_bound_slots_bit_for_bit(f64):
    from super_amd.LM import LM_Solver
    opt = _node_opt(weights="none", n_iter=1)
    lm = LM_Solver(opt, corr_term=True)
    lm.LM(*objects("n3000", f64), flow=flow_of("n3000"))
    want = lm.corr_targets()
    from super_amd.rigid import RigidAlign
    got = RigidAlign(opt, corr_term=True).corr_targets(*objects("n3000", f64), flow_of("n3000"))
    for g, w in zip(got, want):
        assert g.cpu().numpy().astype(np.float64).tobytes() == w.cpu().numpy().astype(np.float64).tobytes()
    assert int(got[2].sum()) > 2000


# ---------------------------------------------------------------------------------------------------- 7. Python
def test_lm_solver_with_rigid_terms_equals_the_composition_by_hand():
    import torch
    from super_amd.LM import LM_Solver
    from super_amd.rigid import RigidAlign, rigid_update
    opt = _node_opt()
    frame, flow = objects("n3000"), flow_of("n3000")
    start = frame[0].points.clone()
    lm = LM_Solver(opt, global_rigid=True, rigid_terms=True, corr_term=True, weighted_data=True)
    beta = lm.LM(*frame, flow=flow).cpu().numpy()
    # by hand
    sf, inputs, nd = objects("n3000")
    ra = RigidAlign(opt, corr_term=True, weighted_data=True)
    tg3 = ra.corr_targets(sf, inputs, nd, flow)                   # on the unmoved model
    Tg = ra.align(sf, inputs, nd, corr_points=tg3)
    assert Tg.cpu().numpy().tobytes() == lm.last_rigid[0].cpu().numpy().tobytes()
    assert ra.last_records[0] == lm.last_rigid_records[0]
    rigid_update(sf, Tg)
    ref = LM_Solver(opt, corr_term=True, weighted_data=True)
    want = ref.LM(sf, inputs, nd, corr_points=tg3).cpu().numpy()
    print(f"LM_Solver(rigid_terms): max|beta - composition| = {np.abs(beta - want).max():.3e}; |T_g - I| = "
          f"{np.abs(Tg.cpu().numpy() - rm.IDENTITY).max():.3e}; kept {lm.last_corr_kept}")
    np.testing.assert_allclose(beta, want, rtol=0, atol=1e-9)
    assert torch.equal(frame[0].points, sf.points) and not torch.equal(frame[0].points, start)      # moved, alike
    # the node solve saw the targets of the UNMOVED model: not those a flow sampled on the moved model gives
    seen = lm.corr_targets()
    for g, w in zip(seen, tg3):
        assert g.cpu().numpy().astype(np.float64).tobytes() == w.cpu().numpy().astype(np.float64).tobytes()
    moved = ra.corr_targets(sf, inputs, nd, flow)
    assert not torch.equal(moved[0], tg3[0])
    # the stage carried the terms: another T_g than the plain stage's
    plain = LM_Solver(opt, global_rigid=True, corr_term=True, weighted_data=True)
    plain.LM(*objects("n3000"), flow=flow)
    assert np.abs(plain.last_rigid[0].cpu().numpy() - Tg.cpu().numpy()).max() > 1e-6


def test_lm_batch_with_rigid_terms_takes_a_fourth_element_per_frame():
    from super_amd.LM import LM_Solver
    opt = _node_opt()
    kw = dict(global_rigid=True, rigid_terms=True, corr_term=True, weighted_data=True)
    fourth = [flow_of("n3000"), triple(rc.targets("n257")), None]
    names = ["n3000", "n257", "n65"]
    lm = LM_Solver(opt, max_frames=3, **kw)
    betas = lm.LM_batch([objects(n) + (f,) for n, f in zip(names, fourth)])
    for i, (n, f) in enumerate(zip(names, fourth)):
        one = LM_Solver(opt, max_frames=3, **kw)
        b = one.LM_batch([objects(n) + (f,)])[0]
        assert lm.last_rigid[i].cpu().numpy().tobytes() == one.last_rigid[0].cpu().numpy().tobytes(), i
        np.testing.assert_allclose(betas[i].cpu().numpy(), b.cpu().numpy(), rtol=0, atol=1e-7)
    assert lm.last_corr_kept[2] is None and lm.last_corr_kept[0] > 2000


def test_refusals_that_need_a_context():
    import torch
    from super_amd import _lib
    from super_amd.rigid import RigidAlign, RigidFrame
    lib = _lib.load()
    frame = objects("n65")
    rf = RigidFrame(*frame)
    one = C.c_void_p(8)
    ra = RigidAlign(options(n_iter=4), max_frames=2)
    cfg = ra._config()

    def refused(rc_, text, code=1):
        assert rc_ == code and lib.slm_last_error().decode() == text, (rc_, lib.slm_last_error())

    # before slm_rigid_set_terms enabled the term
    refused(lib.slm_rigid_set_corr(ra.h, 0, one, one, one),
            "slm_rigid_set_corr: the correspondence term is off; call slm_rigid_set_terms with corr_mode 1 or 2 first")
    refused(lib.slm_rigid_set_semantic(ra.h, 0, 3, one, one, one),
            "slm_rigid_set_semantic: the semantic weight is off; call slm_rigid_set_terms with seg_mode 1 or 2 first")
    assert lib.slm_rigid_set_terms(ra.h, 2, 0.5, 1, 0.0) == 0
    for slot in (-1, 3):
        refused(lib.slm_rigid_set_corr(ra.h, slot, one, one, one), "slm_rigid_set_corr: bad slot")
        refused(lib.slm_rigid_set_semantic(ra.h, slot, 3, one, one, one), "slm_rigid_set_semantic: bad slot")
        refused(lib.slm_rigid_get_terms(ra.h, slot, one, None), "slm_rigid_get_terms: bad slot")
    refused(lib.slm_rigid_set_corr(ra.h, 0, one, None, one), "slm_rigid_set_corr: corr_mode 2 (point-plane) needs nrm")
    refused(lib.slm_rigid_set_corr(ra.h, 0, one, one, None), "slm_rigid_set_corr: null argument")
    for C_ in (0, 5):
        refused(lib.slm_rigid_set_semantic(ra.h, 0, C_, one, one, one),
                "slm_rigid_set_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)", code=5)
    refused(lib.slm_rigid_set_semantic(ra.h, 0, 3, one, None, one), "slm_rigid_set_semantic: null argument")
    # a semantic weight without the slot's inputs: refused, naming the slot -- no silent unweighted run
    arr = (_lib.SlmFrame * 2)(rf.c, rf.c)
    refused(lib.slm_rigid_run(ra.h, C.byref(cfg), 1, arr, None),
            "slm_rigid_run: slot 0 has no semantic inputs; call slm_rigid_set_semantic", code=4)
    seg, sc, tc = frame[0].seg.int(), frame[0].seg_conf.float().contiguous(), frame[2].seg_conf.float().contiguous()
    assert lib.slm_rigid_set_semantic(ra.h, 0, 3, seg.data_ptr(), sc.data_ptr(), tc.data_ptr()) == 0
    refused(lib.slm_rigid_run(ra.h, C.byref(cfg), 2, arr, None),
            "slm_rigid_run: slot 1 has no semantic inputs; call slm_rigid_set_semantic", code=4)
    b = torch.from_numpy(rm.IDENTITY.copy()).cuda()
    refused(lib.slm_rigid_assemble(ra.h, C.byref(cfg), C.byref(rf.c), b.data_ptr(), None, None, None, None),
            "slm_rigid_assemble: slot 2 has no semantic inputs; call slm_rigid_set_semantic", code=4)
    assert lib.slm_rigid_run(ra.h, C.byref(cfg), 1, arr, None) == 0                 # slot 0 has them
    assert lib.slm_rigid_set_semantic(ra.h, 0, 3, None, None, None) == 0            # null sf_seg clears
    refused(lib.slm_rigid_run(ra.h, C.byref(cfg), 1, arr, None),
            "slm_rigid_run: slot 0 has no semantic inputs; call slm_rigid_set_semantic", code=4)
    assert lib.slm_rigid_set_semantic(ra.h, 0, 3, seg.data_ptr(), sc.data_ptr(), tc.data_ptr()) == 0
    assert lib.slm_rigid_set_terms(ra.h, 2, 0.5, 1, 0.0) == 0                       # every call clears every slot
    refused(lib.slm_rigid_run(ra.h, C.byref(cfg), 1, arr, None),
            "slm_rigid_run: slot 0 has no semantic inputs; call slm_rigid_set_semantic", code=4)
    torch.cuda.synchronize()
    # the Python mirror
    hard = rc.Case("n65", True, 1, "hard")
    bare = objects("n65")
    del bare[0].seg
    with pytest.raises(ValueError, match=r"RigidAlign\(weighted_data=True\): sf.seg is missing"):
        aligner(hard).align(*bare)
    with pytest.raises(ValueError, match="flow / corr_points need RigidAlign"):
        RigidAlign(options(n_iter=4)).align(*frame, flow=flow_of("n65"))
    with pytest.raises(ValueError, match=r"flow must be \(1,2,96,128\)"):
        aligner(hard).align(*frame, flow=flow_of("n65")[:, :, :50])
    with pytest.raises(ValueError, match="corr_points must be"):
        aligner(hard).align(*frame, corr_points=triple(rc.targets("n257")))
    with pytest.raises(ValueError, match="give flow or corr_points, not both"):
        aligner(hard).align(*frame, flow=flow_of("n65"), corr_points=triple(rc.targets("n65")))
