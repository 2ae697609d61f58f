"""The global rigid pre-alignment stage of the LM path (slm_rigid_*, super_amd/rigid.py, LM_Solver(global_rigid=True)) on the
GPU against the LM oracle on the one-node frame of tests/rigid_model.py.

Shapes.  k_rg_pass (csrc/slm_rigid.hip) sums every 256 consecutive surfels into one partial (one surfel per thread, four
waves) and launches at most 512 workgroups per frame, so: N = 65 is one past a wave, N = 257 one past a workgroup (a second
partial), N = 3000 twelve partials with a ragged last one, and N = 512 * 256 + 300 = 131 372 makes the first 300 / 256 -> 2
workgroups walk a SECOND chunk of the grid-stride loop (chunk 512 and 513).  97 x 131 is the odd image; the edge scene of
tests/data_edge_cases.py brings holes in index_map, NaN target rows and surfels on the border rows and columns.

Tolerances.  Assembly: the project's own for this comparison (tests/test_gpu_lm_weights.py): JtJ atol 1e-7 max(1, |A|max),
jtl atol 1e-8, loss rtol 1e-8, counts exact.  Loop records: accepted / M_grad / M_loss / u exact, loss rtol 1e-9.  Final raw
beta_g: BETA_TOL below, ten times the largest max|beta_dev - beta_oracle| measured on an MI355X over the fixtures of this
file (RUN_CASES at 4 and at 10 iterations, the train phase and N = 1); every measured value is printed before it is
asserted."""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import data_edge_cases as dec
import rigid_model as rm
from helpers import ref_opt, torch_frame
from oracle import lm_oracle as orc
from super_amd import synth

pytestmark = pytest.mark.gpu

# Measured on an MI355X, max|beta_dev - beta_oracle| per fixture: four iterations 4.8e-17 (n3000 f64), 4.4e-17 (n3000 f32),
# 3.8e-17 (odd), 7.7e-17 (n257); ten iterations 1.5e-16, 1.7e-16, 4.2e-17, 3.4e-16; train phase 3.4e-16; N = 1 1.9e-17.  The
# largest is 3.365e-16 (the translation entries are of the order 1e-2, the quaternion's of 1: a few ulps).  Ten times that:
BETA_TOL = 3.4e-15


# ---------------------------------------------------------------------------------------------------- fixtures
@functools.lru_cache(maxsize=None)
def scene(name):
    """(synth.Scene, model points (N,3) float64): the model rigidly displaced against its target"""
    if name == "n3000":
        sc = synth.make_scene(N=3000, J=64, H=96, W=128, seed=3)
    elif name == "odd":
        sc = synth.make_scene(N=1500, J=48, H=97, W=131, seed=5)
    elif name == "big":
        sc = synth.make_scene(N=512 * 256 + 300, J=64, H=480, W=640, seed=2)
    elif name == "edge":
        sc = dec.edge_scene(4)
        return sc, sc.sf_points.astype(np.float64)          # the hand-placed surfels sit ON the boundaries: not displaced
    elif name in ("n65", "n257"):
        sc, p = scene("n3000")
        n = int(name[1:])
        pick = np.linspace(0, sc.N - 1, n).astype(np.int64)
        return dec.subset(sc, pick), p[pick]
    else:
        raise KeyError(name)
    return sc, rm.displace(sc.sf_points.astype(np.float64))


def objects(name, f64=True, points=None):
    """sf / inputs / new_data on the device and the oracle's one-node frame of the SAME numbers (float32 state: rounded)"""
    import torch
    sc, p = scene(name)
    p = p if points is None else points
    if not f64:
        p = p.astype(np.float32).astype(np.float64)
    sf, inputs, nd = torch_frame(sc)
    sf.points = torch.from_numpy(np.ascontiguousarray(p)).cuda().to(torch.float64 if f64 else torch.float32)
    return (sf, inputs, nd), rm.frame_of_scene(sc, p)


def aligner(max_frames=1, **kw):
    from super_amd.rigid import RigidAlign
    return RigidAlign(ref_opt(rm.rigid_opt(**kw)), max_frames=max_frames)


def check_records(recs, trace, n_iter):
    assert len(recs) == n_iter == len(trace)
    for r, t in zip(recs, trace):
        assert r["status"] == 0
        assert (r["accepted"], r["M_grad"], r["M_loss"]) == (t["accepted"], t["M_grad"], t["M_loss"]), (r, t)
        assert r["u"] == t["u"], (r["u"], t["u"])
        np.testing.assert_allclose(r["loss"], t["loss"], rtol=1e-9, atol=0)


# ---------------------------------------------------------------------------------------------------- 1. assembly
ASSEMBLE_CASES = [("n3000", True), ("n3000", False), ("n65", True), ("n257", True), ("odd", True), ("edge", True),
                  ("edge", False), ("big", True)]


@pytest.mark.parametrize("name,f64", ASSEMBLE_CASES)
def test_assemble_matches_the_oracle_system(name, f64):
    (sf, inputs, nd), fr1 = objects(name, f64)
    ra = aligner()
    opt = rm.rigid_opt()
    for beta in (rm.IDENTITY, rm.displaced_beta()):
        jtj, jtl, loss, M = ra.assemble(sf, inputs, nd, beta)
        A, b, Mo = orc.normal_equations(fr1, beta[None, :], opt)
        lo, Ml = orc.total_loss(fr1, beta[None, :], opt)
        print(f"{name} f64={f64}: M={M} |dA|={np.abs(jtj.cpu().numpy() - A).max():.3e} of {np.abs(A).max():.3e}, "
              f"|db|={np.abs(jtl.cpu().numpy() - b).max():.3e}, loss {loss!r} vs {lo!r}")
        assert M == Mo == Ml
        assert M > 0.5 * fr1.sf_points.shape[0] or name == "edge"
        np.testing.assert_allclose(jtj.cpu().numpy(), A, rtol=0, atol=1e-7 * max(1.0, np.abs(A).max()))
        np.testing.assert_allclose(jtl.cpu().numpy(), b, rtol=0, atol=1e-8)
        np.testing.assert_allclose(loss, lo, rtol=1e-8, atol=0)


def test_assemble_on_the_edge_scene_matches_exactly_the_surfels_the_rules_admit():
    """at identity T == p bitwise for one node at the origin, so every hand-placed tie is decided as the oracle decides it"""
    (sf, inputs, nd), fr1 = objects("edge", True)
    t = orc.data_term(fr1, rm.IDENTITY[None, :], 1.0)
    assert 0 < len(t.r) < fr1.sf_points.shape[0]                      # some dropped, some matched
    assert aligner().assemble(sf, inputs, nd, rm.IDENTITY)[3] == len(t.r)


# ---------------------------------------------------------------------------------------------------- 2./3. the loop
# (not the edge scene: its hand-placed surfels behind the camera and at Z + 1e-8 == 0 carry residuals of metres -- a loss of
# 31 against 1e-3 -- whose linearisation means nothing, and the match set changes by dozens per step by construction; the
# final point there measures the fixture.  The assembly tests above pin the kernel on that scene at two points.)
RUN_CASES = [("n3000", True), ("n3000", False), ("odd", True), ("n257", True)]


def run_case(name, f64, n_iter, phase="test"):
    import torch
    (sf, inputs, nd), fr1 = objects(name, f64)
    ra = aligner(num_optimize_iterations=n_iter, phase=phase)
    tg = ra.align(sf, inputs, nd)
    beta = ra.beta(0).cpu().numpy()
    want, trace = rm.run(fr1, rm.rigid_opt(num_optimize_iterations=n_iter, phase=phase))
    err = float(np.abs(beta - want).max())
    print(f"rigid run {name} f64={f64} iters={n_iter} phase={phase}: max|beta_dev - beta_oracle| = {err:.3e}; losses "
          f"{[r['loss'] for r in ra.last_records[0]]}")
    torch.cuda.synchronize()
    return ra, tg.cpu().numpy(), beta, want, trace, err


@pytest.mark.parametrize("name,f64", RUN_CASES)
def test_run_four_iterations_matches_the_oracle_trace(name, f64):
    ra, tg, beta, want, trace, err = run_case(name, f64, 4)
    check_records(ra.last_records[0], trace, 4)
    assert err <= BETA_TOL, err
    np.testing.assert_allclose(tg, rm.normalised(want), rtol=0, atol=BETA_TOL)
    assert abs(np.linalg.norm(tg[:4]) - 1.0) < 1e-15
    loss0 = orc.total_loss(objects(name, f64)[1], rm.IDENTITY[None, :], rm.rigid_opt())[0]
    assert min(r["loss"] for r in ra.last_records[0] if r["accepted"]) < 0.1 * loss0   # the displacement is removed


@pytest.mark.parametrize("name,f64", RUN_CASES)
def test_run_ten_iterations_final_point_and_loss(name, f64):
    ra, tg, beta, want, trace, err = run_case(name, f64, 10)
    assert err <= BETA_TOL, err
    best = min(t["loss"] for t in trace if t["accepted"])
    got = min(r["loss"] for r in ra.last_records[0] if r["accepted"])
    np.testing.assert_allclose(got, best, rtol=1e-9, atol=0)


def test_train_phase_always_accepts():
    ra, tg, beta, want, trace, err = run_case("n3000", True, 4, phase="train")
    check_records(ra.last_records[0], trace, 4)
    assert all(r["accepted"] and r["u"] == 10.0 for r in ra.last_records[0])
    assert err <= BETA_TOL, err


# ---------------------------------------------------------------------------------------------------- 4. degenerate frames
def _degenerate(kind):
    import torch
    sc, p = scene("n3000")
    sf, inputs, nd = torch_frame(sc)
    if kind == "N0":
        sf.points = sf.points[:0].contiguous()
    elif kind == "T0":
        nd.points, nd.norms = nd.points[:0].contiguous(), nd.norms[:0].contiguous()
        nd.index_map = -torch.ones_like(nd.index_map)
        nd.valid = torch.zeros_like(nd.valid)
    elif kind == "outside":                                   # half of the model far to the side, half behind and off-axis
        q = p.copy()
        q[::2, 0] += 50.0
        q[1::2] *= -1.0
        q[1::2, 1] += 50.0
        sf.points = torch.from_numpy(q).cuda()
    return sf, inputs, nd


@pytest.mark.parametrize("kind", ["N0", "T0", "outside"])
def test_a_frame_without_matches_ends_at_identity(kind):
    ra = aligner(num_optimize_iterations=4)
    tg = ra.align(*_degenerate(kind)).cpu().numpy()
    assert (tg == rm.IDENTITY).all(), tg
    assert (ra.beta(0).cpu().numpy() == rm.IDENTITY).all()
    recs = ra.last_records[0]
    assert len(recs) == 4 and all(r["status"] == 0 and r["M_grad"] == 0 and r["M_loss"] == 0 for r in recs)
    assert recs[0]["accepted"] and recs[0]["loss"] == 0.0


def test_one_surfel():
    import torch
    sc, p = scene("n3000")
    one = p[1234:1235]
    sf, inputs, nd = torch_frame(sc)
    sf.points = torch.from_numpy(one.copy()).cuda()
    ra = aligner(num_optimize_iterations=4)
    ra.align(sf, inputs, nd)
    want, trace = rm.run(rm.frame_of_scene(sc, one), rm.rigid_opt(num_optimize_iterations=4))
    beta = ra.beta(0).cpu().numpy()
    print(f"rigid run N=1: max|beta_dev - beta_oracle| = {np.abs(beta - want).max():.3e}")
    check_records(ra.last_records[0], trace, 4)
    assert trace[0]["M_grad"] == 1
    assert np.abs(beta - want).max() <= BETA_TOL


# ---------------------------------------------------------------------------------------------------- 5./6. bits, batches
def _single(frame, n_iter=4):
    ra = aligner(num_optimize_iterations=n_iter)
    ra.align(*frame)
    return ra.beta(0).cpu().numpy(), ra.last_records[0]


def test_two_runs_give_the_same_bits():
    frame = objects("n3000")[0]
    (b0, r0), (b1, r1) = _single(frame), _single(frame)
    assert b0.tobytes() == b1.tobytes() and r0 == r1
    ra = aligner(num_optimize_iterations=4)                     # and the same context run twice
    ra.align(*frame)
    first = ra.beta(0).cpu().numpy().tobytes()
    ra.align(*frame)
    assert ra.beta(0).cpu().numpy().tobytes() == first == b0.tobytes()
    j0 = ra.assemble(*frame, rm.displaced_beta())
    j1 = ra.assemble(*frame, rm.displaced_beta())
    assert j0[0].cpu().numpy().tobytes() == j1[0].cpu().numpy().tobytes() and j0[2:] == j1[2:]
    assert ra.beta(0).cpu().numpy().tobytes() == first          # the assembly has a slot of its own


def test_a_batch_of_three_equals_the_three_single_runs():
    frames = [objects("n3000")[0], _degenerate("N0"), objects("odd")[0]]
    ra = aligner(max_frames=4, num_optimize_iterations=4)
    tgs = ra.align_batch(frames)
    for i, fr in enumerate(frames):
        b, recs = _single(fr)
        assert ra.beta(i).cpu().numpy().tobytes() == b.tobytes(), i
        assert ra.last_records[i] == recs, i
    assert (tgs[1].cpu().numpy() == rm.IDENTITY).all()
    with pytest.raises(ValueError):
        ra.align_batch(frames + frames)


def test_a_failed_factorisation_stops_its_frame_only():
    """The middle frame's target has x = +inf in every point: its surfels still match (o is inf, not NaN), e = T - o is
    -inf, the tap sums of the Jacobian are inf - inf and every pivot is NaN.  (A NaN or inf in sf_points cannot do it: at the
    identity it makes all of T(p) NaN -- 0 * NaN in the cross products --, the projection is not finite and the surfel is
    dropped by the match test.)"""
    import torch
    good0, good1 = objects("n3000")[0], objects("odd")[0]
    sf, inputs, nd = objects("n3000")[0]
    nd = SimpleNamespace(**vars(nd))
    nd.points = nd.points.clone()
    nd.points[:, 0] = float("inf")
    ra = aligner(max_frames=3, num_optimize_iterations=4)
    tgs = ra.align_batch([good0, (sf, inputs, nd), good1])
    bad = ra.last_records[1]
    assert bad[0]["status"] == 1 and bad[0]["u"] == 10.0 and bad[0]["M_grad"] > 0
    assert all(r["status"] == 2 for r in bad[1:])
    assert (tgs[1].cpu().numpy() == rm.IDENTITY).all()
    for i, fr in ((0, good0), (2, good1)):
        b, recs = _single(fr)
        assert ra.beta(i).cpu().numpy().tobytes() == b.tobytes() and ra.last_records[i] == recs
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 7. the move
@pytest.mark.parametrize("f64", [True, False])
def test_transform_matches_the_oracle_move(f64):
    import torch
    from super_amd.rigid import rigid_transform
    sc, p = scene("n3000")
    dt, ndt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
    p = p.astype(ndt)
    n = sc.sf_norms.astype(ndt).copy()
    n[17] = 0.0
    Tg = rm.normalised(rm.displaced_beta(angle=0.3))
    P, Nn = torch.from_numpy(p.copy()).cuda(), torch.from_numpy(n.copy()).cuda()
    rigid_transform(P, Nn, torch.from_numpy(Tg))
    wp, wn = rm.moved(p.astype(np.float64), n.astype(np.float64), Tg)
    gp, gn = P.cpu().numpy().astype(np.float64), Nn.cpu().numpy().astype(np.float64)
    assert P.dtype == dt and Nn.dtype == dt
    if f64:
        np.testing.assert_allclose(gp, wp, rtol=0, atol=1e-14)
        np.testing.assert_allclose(gn, wn, rtol=0, atol=1e-14)
    else:                                                       # one float32 ulp of the result vector's magnitude
        for got, want in ((gp, wp), (gn, wn)):
            ulp = np.spacing(np.linalg.norm(want, axis=1).astype(np.float32)).astype(np.float64)[:, None]
            assert (np.abs(got - want) <= np.maximum(ulp, 1e-45)).all()
    assert (gn[17] == 0.0).all()
    only_points = torch.from_numpy(p.copy()).cuda()
    rigid_transform(only_points, None, torch.from_numpy(Tg))
    assert only_points.cpu().numpy().tobytes() == P.cpu().numpy().tobytes()


@pytest.mark.parametrize("f64", [True, False])
def test_rigid_update_moves_surfels_and_nodes_and_leaves_the_skinning_tables(f64):
    import torch
    from super_amd.rigid import rigid_update
    (sf, inputs, nd), _ = objects("n3000", f64)
    ed = sf.ED_nodes
    if not f64:
        sf.norms, ed.points, ed.norms = sf.norms.float(), ed.points.float(), ed.norms.float()
    old = (sf.points, sf.norms, ed.points, ed.norms)
    copies = [t.clone() for t in old]
    knn = (sf.knn_indices, sf.knn_w, ed.knn_indices, ed.knn_w)
    knn_copies = [t.clone() for t in knn]
    Tg = rm.normalised(rm.displaced_beta(angle=0.2))
    rigid_update(sf, torch.from_numpy(Tg).cuda())
    for t, c in zip(old, copies):                              # out of place: the caller's old tensors are untouched
        assert torch.equal(t, c)
    for t, c, now in zip(knn, knn_copies, (sf.knn_indices, sf.knn_w, ed.knn_indices, ed.knn_w)):
        assert now is t and torch.equal(t, c)
    tol = 1e-14 if f64 else 2e-7
    for pts, nrm, op, on in ((sf.points, sf.norms, copies[0], copies[1]), (ed.points, ed.norms, copies[2], copies[3])):
        assert pts.dtype == op.dtype and nrm.dtype == on.dtype
        wp, wn = rm.moved(op.cpu().numpy().astype(np.float64), on.cpu().numpy().astype(np.float64), Tg)
        np.testing.assert_allclose(pts.cpu().numpy(), wp, rtol=0, atol=tol * max(1.0, np.abs(wp).max()))
        np.testing.assert_allclose(nrm.cpu().numpy(), wn, rtol=0, atol=tol)


# ---------------------------------------------------------------------------------------------------- 8. LM_Solver
def test_lm_solver_with_global_rigid_equals_the_composition_by_hand():
    import torch
    from super_amd.LM import LM_Solver
    opt = orc.default_opt()
    (sf, inputs, nd), fr1 = objects("n3000")
    ed = sf.ED_nodes
    start = [t.clone() for t in (sf.points, sf.norms, ed.points, ed.norms)]
    lm = LM_Solver(ref_opt(opt), global_rigid=True)
    beta = lm.LM(sf, inputs, nd).cpu().numpy()
    # by hand: the oracle's stage, the oracle's move, the existing solver on the moved model
    want_g, _ = rm.run(fr1, rm.rigid_opt())
    Tg = rm.normalised(want_g)
    print(f"LM_Solver(global_rigid): |T_g - oracle| = {np.abs(lm.last_rigid[0].cpu().numpy() - Tg).max():.3e}")
    np.testing.assert_allclose(lm.last_rigid[0].cpu().numpy(), Tg, rtol=0, atol=BETA_TOL)
    sf2, inputs2, nd2 = objects("n3000")[0]
    ed2 = sf2.ED_nodes
    mp, mn = rm.moved(start[0].cpu().numpy(), start[1].cpu().numpy(), Tg)
    gp, gn = rm.moved(start[2].cpu().numpy(), start[3].cpu().numpy(), Tg)
    sf2.points, sf2.norms = torch.from_numpy(mp).cuda(), torch.from_numpy(mn).cuda()
    ed2.points, ed2.norms = torch.from_numpy(gp).cuda(), torch.from_numpy(gn).cuda()
    ref = LM_Solver(ref_opt(opt))
    want = ref.LM(sf2, inputs2, nd2).cpu().numpy()
    print(f"LM_Solver(global_rigid): max|beta - composition| = {np.abs(beta - want).max():.3e}; rigid losses "
          f"{[r['loss'] for r in lm.last_rigid_records[0]]}; LM losses {[r['loss'] for r in lm.last_records[0]]}")
    np.testing.assert_allclose(beta, want, rtol=0, atol=1e-9)
    # sf was moved by the call (documented), to the oracle's move
    np.testing.assert_allclose(sf.points.cpu().numpy(), mp, rtol=0, atol=1e-10)
    np.testing.assert_allclose(ed.points.cpu().numpy(), gp, rtol=0, atol=1e-10)
    # the stage pays: the node solve starts from a far smaller loss than on the displaced model
    plain = LM_Solver(ref_opt(opt))
    plain.LM(*objects("n3000")[0])
    assert lm.last_records[0][0]["loss"] < plain.last_records[0][0]["loss"]


def test_global_rigid_false_changes_nothing(monkeypatch):
    """Without the flag LM() makes the calls it made before: the stage is never entered, no context for it exists, sf is
    not touched.  Two runs of the node solve itself are NOT bit-identical (measured here on an MI355X: two LM_Solver(opt)
    on the same frame differ in the last bit of beta; its assembly adds with float atomics), so the results of two runs
    are compared to the LM tests' atol = 1e-9, not bitwise."""
    import torch
    from super_amd import rigid
    from super_amd.LM import LM_Solver

    def never(*a, **k):
        raise AssertionError("the rigid stage was entered without global_rigid")
    monkeypatch.setattr(LM_Solver, "_rigid_stage", never)
    monkeypatch.setattr(rigid.RigidAlign, "__init__", never)
    monkeypatch.setattr(rigid, "rigid_update", never)
    opt = ref_opt(orc.default_opt())
    frame_a, frame_b = objects("n3000")[0], objects("n3000")[0]
    sf = frame_b[0]
    held = (sf.points, sf.norms, sf.ED_nodes.points, sf.ED_nodes.norms)
    a = LM_Solver(opt).LM(*frame_a)
    lm = LM_Solver(opt, global_rigid=False)
    b = lm.LM(*frame_b)
    np.testing.assert_allclose(b.cpu().numpy(), a.cpu().numpy(), rtol=0, atol=1e-9)
    assert all(x is y for x, y in zip(held, (sf.points, sf.norms, sf.ED_nodes.points, sf.ED_nodes.norms)))
    assert lm.last_rigid is None and lm._rigid is None and lm.global_rigid is False
    lm.prepare_model(frame_b[0])                                # still allowed
    torch.cuda.synchronize()


def test_lm_solver_refusals_with_global_rigid():
    from super_amd.LM import LM_Solver
    opt = ref_opt(orc.default_opt())
    lm = LM_Solver(opt, global_rigid=True, max_frames=2)
    frame = objects("n3000")[0]
    with pytest.raises(NotImplementedError, match="prepare_model: not with global_rigid"):
        lm.prepare_model(frame[0])
    with pytest.raises(ValueError, match="must not share an sf object"):
        lm.LM_batch([frame, frame])


# ---------------------------------------------------------------------------------------------------- 9. a sequence
def _sequence(global_rigid):
    """Four frames of the deforming synthetic surface of tests/test_gpu_fusion.py with a rigid drift between frames: the
    whole surface comes 6 mm nearer per frame (the endoscope advancing), THREE iterations per stage.  Why three: a rigid
    motion costs the node solve nothing (ARAP and Rot are zero on it), so given enough iterations both runs end in the SAME
    minimum and "not larger" would compare rounding errors -- the oracle on one such frame pair (3000 surfels, 64 nodes)
    gives with / without = 1 + 1e-9 at ten iterations for 4, 6 and 10 mm alike, and 0.83 / 0.82 / 0.78 at three.  What the
    stage buys is iterations, so the budget must be one the drift does not fit into."""
    import torch
    from driver_harness import FrameLoop
    from super_amd.LM import LM_Solver
    H, W = 96, 128
    K = synth._scaled_intrinsics(H, W)
    inv_K = np.linalg.pinv(K)
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    color = np.random.default_rng(2).uniform(0, 255, (3, H, W)).astype(np.float32)
    opt = SimpleNamespace(height=H, width=W, data="superv1", load_valid_mask=False, depth_model="monodepth2",
                          dilate_invalid_kernel=0, normal_model="naive", phase="test", method="super", load_depth=True,
                          deform_udpate_method="super_edg", mesh_step_size=8, use_derived_gradient=True,
                          sf_point_plane=True, mesh_arap=True, mesh_rot=True, mesh_face=False, sf_point_plane_weight=1.0,
                          mesh_arap_weight=10.0, mesh_rot_weight=1.0, mesh_face_weight=1.0, num_optimize_iterations=3,
                          num_neighbors=4, num_ED_neighbors=4, th_dist=0.02, th_cosine_ang=0.4, th_time_steps=30,
                          disable_merging_new_surfels=False, disable_merging_exist_surfels=False,
                          disable_adding_new_surfels=False, disable_removing_unstable_surfels=False,
                          slm_prepare_ahead=False)
    loop = FrameLoop(opt)
    loop.lm = LM_Solver(opt, global_rigid=global_rigid)
    finals = []
    for k in range(4):
        depth = (synth._surface(uu, vv, H, W, 0.3 + 0.03 * k) - 0.006 * k).astype(np.float32)
        depth[:4] = 0.0
        depth[:, :4] = 0.0
        inputs = {("depth", 0): torch.from_numpy(depth.copy())[None, None], ("disp", 0): torch.zeros(1, 1, H, W),
                  "inv_K": torch.from_numpy(inv_K)[None], "K": torch.from_numpy(K)[None],
                  ("color", 0): torch.from_numpy(color)[None], "divterm": torch.tensor(1.0 / (2 * 0.6 * 0.6)),
                  "filename": ["%06d" % k], "time": k, "ID": torch.tensor([k])}
        loop(SimpleNamespace(), inputs)
        if k:
            acc = [r["loss"] for r in loop.lm.last_records[0] if r["status"] == 0 and r["accepted"]]
            finals.append(acc[-1])
            assert torch.isfinite(loop.sf.points).all()
    return finals


def test_sequence_with_rigid_drift_final_losses_are_not_larger():
    """a sanity check of the wiring between two runs of this code, no accuracy claim"""
    without, with_ = _sequence(False), _sequence(True)
    print("final accepted LM loss per frame: without", without, "with global_rigid", with_)
    assert len(without) == len(with_) == 3
    for a, b in zip(without, with_):
        assert b <= a, (without, with_)


# ---------------------------------------------------------------------------------------------------- refusals with a context
def test_refusals_that_need_a_context():
    from super_amd import _lib
    from super_amd.rigid import RigidFrame
    lib = _lib.load()
    ra = aligner(max_frames=2, num_optimize_iterations=4)
    rf = RigidFrame(*objects("n65")[0])
    cfg = ra._config()
    one = C.c_void_p(8)

    def refused(rc, text):
        assert rc == 1 and lib.slm_last_error().decode() == text, (rc, lib.slm_last_error())

    def frame(**kw):
        f = _lib.SlmFrame()
        C.memmove(C.byref(f), C.byref(rf.c), C.sizeof(f))
        for k, v in kw.items():
            setattr(f, k, v)
        return f

    arr = (_lib.SlmFrame * 3)(rf.c, rf.c, rf.c)
    for n in (0, 3, -1):
        refused(lib.slm_rigid_run(ra.h, C.byref(cfg), n, arr, None), "slm_rigid_run: n_frames must be in 1..max_frames")
    bad = ra._config()
    bad.num_iterations = -1
    refused(lib.slm_rigid_run(ra.h, C.byref(bad), 1, arr, None), "slm_rigid_run: num_iterations must be >= 0")
    refused(lib.slm_rigid_assemble(ra.h, C.byref(bad), C.byref(rf.c), one, None, None, None, None),
            "slm_rigid_assemble: num_iterations must be >= 0")
    for fn, call in (("slm_rigid_run", lambda f: lib.slm_rigid_run(ra.h, C.byref(cfg), 1, C.byref(f), None)),
                     ("slm_rigid_assemble", lambda f: lib.slm_rigid_assemble(ra.h, C.byref(cfg), C.byref(f), one, None, None,
                                                                             None, None))):
        refused(call(frame(H=1)), fn + ": H and W must be >= 2")
        refused(call(frame(W=1)), fn + ": H and W must be >= 2")
        refused(call(frame(N=-1)), fn + ": N and T must be >= 0")
        refused(call(frame(sf_points=None)), fn + ": N > 0 needs sf_points")
        for name in ("tgt_points", "tgt_norms", "index_map", "tgt_valid"):
            refused(call(frame(**{name: None})), fn + ": T > 0 needs tgt_points, tgt_norms, index_map and tgt_valid")
    recs = (_lib.SlmIterRecord * 4)()
    for slot in (-1, 2):
        refused(lib.slm_rigid_get(ra.h, slot, one, None), "slm_rigid_get: bad slot")
        refused(lib.slm_rigid_get_beta(ra.h, slot, one, None), "slm_rigid_get_beta: bad slot")
        refused(lib.slm_rigid_get_records(ra.h, slot, recs, 4, None, None), "slm_rigid_get_records: bad slot")
    refused(lib.slm_rigid_get_records(ra.h, 0, recs, -1, None, None), "slm_rigid_get_records: max_records must be >= 0")
    # a slot that never ran reads as a finished run at identity, with no records
    got = C.c_int32(-1)
    assert lib.slm_rigid_get_records(ra.h, 1, recs, 4, C.byref(got), None) == 0 and got.value == 0
    assert (ra.beta(1).cpu().numpy() == rm.IDENTITY).all()
    # nothing above disturbed the context
    ra.align(*objects("n65")[0])
    assert ra.last_records[0][0]["M_grad"] == 65
    with pytest.raises(ValueError):
        aligner(max_frames=0)
