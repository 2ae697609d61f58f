"""The inputs of test_gpu_render_loss_shapes.py, checked with the CPU models alone (no GPU): every SSIM image / target pair
reaches the branches it is there for, the model's SSIM gradient equals finite differences where a pixel lies three times
in a reflected window, the vectorised hit sets equal the loop's, and the hand-built scenes keep their share of
threshold pixels under the cap.  Tolerances: 1e-6 of the largest entry on the finite differences (as
test_render_grad_model.py); everything else is exact."""
import ctypes as C

import numpy as np
import pytest

import render_grad_model as rgm
import render_loss_cases as rc
import render_model as rm


# ---- SSIM inputs ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,holes", rc.SSIM_CASES)
def test_ssim_inputs_reach_every_branch(h, w, holes):
    img, tgt = rc.ssim_inputs(h, w, holes)
    assert img.dtype == tgt.dtype == np.float32 and img.shape == (h, w, 3) and tgt.shape == (3, h, w)
    rc.assert_ssim_branches(h, w, holes, img, rc.ssim_model(img, tgt))


@pytest.mark.parametrize("h,w,holes", [(6, 6, False), (10, 17, True)])
def test_ssim_model_gradient_matches_finite_differences(h, w, holes):
    """h or w in 6..10: a pixel lies up to three times in a reflected window along that axis.  Central differences of the
    model's loss in float64 on corners, an edge pixel and the centre pin that multiplicity independently of autograd's
    reflection-pad backward.  The selection is constant under the step (the margins of assert_ssim_branches)."""
    img, tgt = rc.ssim_inputs(h, w, holes)
    mod = rc.ssim_model(img, tgt)
    x, t = img.astype(np.float64), tgt.astype(np.float64)
    scale = np.abs(mod["grad"]).max()
    assert scale > 0
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w - 1), (0, w // 2), (h // 2, w // 2), (h - 1, w // 2 + 1)]
    pts = [p for p in pts if x[p].min() > 0]                 # a hole sits at the mask's threshold: not differentiable
    assert len(pts) >= 6
    step, checked = 1e-6, 0
    for i, j in pts:
        for c in range(3):
            a, b = x.copy(), x.copy()
            a[i, j, c] += step
            b[i, j, c] -= step
            fd = (rc.ssim_loss_only(a, t) - rc.ssim_loss_only(b, t)) / (2 * step)
            assert abs(fd - mod["grad"][i, j, c]) <= 1e-6 * scale, (i, j, c, fd, mod["grad"][i, j, c])
            checked += abs(fd) > 1e-3 * scale
    assert checked >= 6                                       # not a comparison of zeros


def test_ssim_refusals_need_no_device():
    """sizes below 6 and null pointers are refused before anything touches the device (host buffers are never read)"""
    from super_amd import _lib, build
    build.build()
    lib = _lib.load()
    buf = (C.c_float * (3 * 16 * 16))()
    out = (C.c_double * 2)()
    fn = lib.slm_render_ssim_loss
    fn.restype = C.c_int
    args = lambda h, w, a, b, o: (C.c_int32(h), C.c_int32(w), a, b, C.c_double(1.0), o, None, None)
    p, o = C.cast(buf, C.c_void_p), C.cast(out, C.c_void_p)
    for h, w in ((5, 16), (16, 5), (5, 5), (0, 16), (16, -1)):
        assert fn(*args(h, w, p, p, o)) == _lib.SLM_ERR_INVALID, (h, w)
        assert b"slm_render_ssim_loss" in lib.slm_last_error() and b">= 6" in lib.slm_last_error()
    for a, b, o2 in ((None, p, o), (p, None, o), (p, p, None)):
        assert fn(*args(16, 16, a, b, o2)) == _lib.SLM_ERR_INVALID
        assert b"slm_render_ssim_loss" in lib.slm_last_error() and b"null" in lib.slm_last_error()


# ---- hit sets ---------------------------------------------------------------------------------------------------------

def _scene_60x80():
    from super_amd import synth
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    return sc.sf_points, None, sc.K, sc.H, sc.W, 0.01


def _overflow_one_tile():
    rng = np.random.default_rng(4)                  # the scene of test_gpu_render_grad.test_backward_on_the_overflow_path
    n = 6000
    Z = rng.uniform(0.5, 3.0, n)
    u, v = rng.uniform(17.5, 30.5, n), rng.uniform(17.5, 30.5, n)
    return np.stack([(u - 32.0) * Z / 100.0, (v - 24.0) * Z / 100.0, Z], 1), None, rc.K0, 48, 64, 1.0 * Z.min() / 100.0


HIT_SCENES = {"60x80": _scene_60x80, "overflow": _overflow_one_tile, "overflow_neighbours": rc.overflow_with_neighbours,
              "ties": rc.ties, "big_splats": rc.big_splats}


@pytest.mark.parametrize("name", list(HIT_SCENES))
@pytest.mark.parametrize("n_track,view_scale", [(rm.N_TRACK, 1.0), (3, 1.0), (rm.N_TRACK, 0.5)])
def test_vectorised_hit_sets_equal_the_loop(name, n_track, view_scale):
    P, _, K, H, W, rad = HIT_SCENES[name]()
    want = rgm.hit_sets(P, K, H, W, rad, view_scale, n_track)
    assert len(want[0]) > 0
    for max_candidates in (8_000_000, 5_000):                 # one pass, and many
        got = rgm.hit_sets_fast(P, K, H, W, rad, view_scale, n_track, max_candidates)
        for a, b in zip(got, want):
            assert a.dtype == b.dtype
            np.testing.assert_array_equal(a, b)


def test_vectorised_hit_sets_of_no_points_and_all_culled():
    for P in (np.zeros((0, 3)), np.array([[0, 0, 0.005], [0, 0, 20.0], [0, 0, -1.0], [50.0, 0, 1.0]])):
        for a, b in zip(rgm.hit_sets_fast(P, rc.K0, 48, 64, 0.02), rgm.hit_sets(P, rc.K0, 48, 64, 0.02)):
            np.testing.assert_array_equal(a, b)
            assert len(a) == 0


# ---- hand-built scenes ------------------------------------------------------------------------------------------------

def test_big_splats_span_tiles_and_every_border():
    P, cols, K, H, W, rad = rc.big_splats()
    w, h, f, ccx, ccy = rm.camera(K, H, W)
    x0, x1 = rm._range(P[:, 0], P[:, 2], rad, f, ccx, w, 0.5)
    y0, y1 = rm._range(P[:, 1], P[:, 2], rad, f, ccy, h, 0.5)
    u, v = f * P[:, 0] / P[:, 2] + ccx, f * P[:, 1] / P[:, 2] + ccy
    for outside, clipped in ((u < 0, x0 == 0), (u > w - 1, x1 == w - 1), (v < 0, y0 == 0), (v > h - 1, y1 == h - 1)):
        assert (outside & clipped & (x0 <= x1) & (y0 <= y1)).sum() >= 2          # centred outside, box cut by that side
    tiles_x, tiles_y = x1 // 16 - x0 // 16 + 1, y1 // 16 - y0 // 16 + 1
    assert (np.minimum(tiles_x, tiles_y) >= 3).mean() > 0.5 and tiles_x.max() >= 7
    px = 2 * f * rad / P[:, 2]
    assert 40 <= px.min() and px.max() <= 120
    fact = rc.hand_scene_facts(P, cols, K, H, W, rad)
    assert fact["taken"].all()                                 # every surfel is in the comparison


def test_overflow_scene_fills_the_centre_tile_and_shares_with_all_neighbours():
    P, cols, K, H, W, rad = rc.overflow_with_neighbours()
    lists = rc.tile_lists(P, K, H, W, rad)
    assert len(lists[(1, 1)]) > 4096
    for t in ((0, 0), (0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1), (2, 2)):
        own = lists[t] - lists[(1, 1)]
        assert len(lists[t] & lists[(1, 1)]) > 0 and len(own) > 100, t
    px = 100.0 * rad / P[:, 2]
    assert 2.0 <= px.min() and px.max() <= 3.0
    fact = rc.hand_scene_facts(P, cols, K, H, W, rad, max_lost=rc.OVERFLOW_MAX_LOST)
    assert fact["count"].reshape(H, W)[16:32, 16:32].min() == rm.N_TRACK


@pytest.mark.parametrize("n_track", [rm.N_TRACK, 3])
def test_tie_scene_cuts_inside_the_tie_group(n_track):
    P, cols, K, H, W, rad = rc.ties()
    fact = rc.hand_scene_facts(P, cols, K, H, W, rad, n_track)
    assert fact["near_share"] == 0.0
    tie = np.setdiff1d(np.arange(len(P)), rc.TIE_FRONT + rc.TIE_BEHIND)
    assert len(tie) == 70 and (P[tie] == P[tie[0]]).all()
    taken = fact["taken"]
    assert taken[list(rc.TIE_FRONT)].all() and taken[tie].any() and not taken[tie].all()     # the cut is inside the group
    first = n_track if n_track < 64 else 64                    # pixels that see the tie group alone take its first rows
    assert taken[tie[:first]].all() and not taken[tie[first:]].any()
    assert taken[list(rc.TIE_BEHIND)].all()                    # shifted sideways: pixels with fewer than n_track hits
    assert fact["count"].max() == n_track
