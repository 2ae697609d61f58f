"""Pins tests/render_radii_model.py (the CPU restatement of the per-point-radius renderer) three ways: against
render_model.render when all radii are equal, against a hand-computed scene of two spheres with different radii over one
pixel, and its gradients against central finite differences in float64.  No GPU."""
import math

import numpy as np
import torch

import render_model as rm
import render_radii_model as rrm

K0 = np.array([[100.0, 0, 32.0], [0, 100.0, 24.0], [0, 0, 1]])


def test_equal_radii_are_render_model_exactly():
    from super_amd import synth
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    cols = np.random.default_rng(12).uniform(size=(sc.N, 3)).astype(np.float32)
    for r, scale, n_track in ((0.01, 1.0, rm.N_TRACK), (2e-3, 0.5, rm.N_TRACK), (0.01, 1.0, 3)):
        r32 = float(np.float32(r))
        assert r32 != r
        want = rm.render(sc.sf_points, cols, sc.K, sc.H, sc.W, r32, scale, bg=(0.1, 0.2, 0.3), n_track=n_track)
        got = rrm.render(sc.sf_points, cols, np.full(sc.N, r, np.float32), sc.K, sc.H, sc.W, scale, bg=(0.1, 0.2, 0.3),
                         n_track=n_track)
        for k in ("img", "front", "count", "near"):
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert (want["count"] > 0).any() and (r < 0.01 or (want["count"] > 1).any())


def test_two_spheres_with_different_radii_over_one_pixel():
    # pixel (24, 32) looks along the axis: d = (0, 0, 1), so rho = sqrt(X^2 + Y^2).  Sphere 0 at Z = 1 with r = 0.005 is
    # 0.003 off the axis; sphere 1, half a gamma behind in zt, with r = 0.02 is 0.005 off the axis.
    dz = float(np.float32(1.0 + 0.5 * rm.GAMMA * (rm.Z_FAR - rm.Z_NEAR))) - 1.0
    P = np.array([[0.003, 0.0, 1.0], [0.0, 0.005, 1.0 + dz]])
    cols = np.array([[1.0, 0.0, 0.25], [0.0, 0.5, 0.75]], np.float32)
    radii = np.array([0.005, 0.02], np.float32)
    bg = np.array([0.1, 0.2, 0.3])
    out = rrm.render(P, cols, radii, K0, 48, 64, bg=bg)
    P32 = P.astype(np.float32).astype(np.float64)
    r0, r1 = float(radii[0]), float(radii[1])                     # the float32 values, widened
    w0 = 1.0 - math.hypot(P32[0, 0], P32[0, 1]) / r0
    zt0, zt1 = (rm.Z_FAR - P32[0, 2]) / (rm.Z_FAR - rm.Z_NEAR), (rm.Z_FAR - P32[1, 2]) / (rm.Z_FAR - rm.Z_NEAR)
    w1 = (1.0 - math.hypot(P32[1, 0], P32[1, 1]) / r1) * math.exp((zt1 - zt0) / rm.GAMMA)
    wbg = math.exp((rm.BG_EPS - zt0) / rm.GAMMA)
    want = (w0 * cols[0].astype(np.float64) + w1 * cols[1].astype(np.float64) + wbg * bg) / (w0 + w1 + wbg)
    assert 0.39 < w0 < 0.41 and 0.4 < w1 < 0.5                    # (1 - 0.6), (1 - 0.25) e^-0.5
    np.testing.assert_allclose(out["img"][24, 32], want, rtol=1e-14)
    assert out["front"][24, 32] == 0 and out["count"][24, 32] == 2
    # one pixel to the right (rho grows by ~0.01): beyond sphere 0's radius, inside sphere 1's
    assert out["count"][24, 33] == 1 and out["front"][24, 33] == 1
    np.testing.assert_allclose(out["img"][24, 33], cols[1], rtol=1e-12)
    # with the radii swapped sphere 1 misses the centre pixel (0.005 is not < float32(0.005)... it is its own radius)
    sw = rrm.render(P, cols, radii[::-1].copy(), K0, 48, 64, bg=bg)
    assert sw["count"][24, 32] == 1 and sw["front"][24, 32] == 0
    # rows with a radius that is 0, negative, NaN or inf are culled
    bad = rrm.render(np.tile(P[:1], (4, 1)), np.ones((4, 3), np.float32), [0.0, -1.0, np.nan, np.inf], K0, 48, 64, bg=bg)
    assert (bad["count"] == 0).all() and (bad["front"] == -1).all()


def _fd_scene():
    # eight spheres around the image centre within 1e-4 m of depth (they blend), radii 2.5 .. 6 px
    rng = np.random.default_rng(2)
    n = 8
    Z = 1.0 + rng.uniform(0.0, 1e-4, n)
    u, v = 32.0 + rng.uniform(-5.0, 5.0, n), 24.0 + rng.uniform(-5.0, 5.0, n)
    P = np.stack([(u - 32.0) * Z / 100.0, (v - 24.0) * Z / 100.0, Z], 1)
    # float32-representable inputs, so that the roundings the model passes are identities and the differences see them
    P = P.astype(np.float32).astype(np.float64)
    cols = rng.uniform(size=(n, 3)).astype(np.float32).astype(np.float64)
    radii = (rng.uniform(2.5, 6.0, n) * Z / 100.0).astype(np.float32).astype(np.float64)
    return P, cols, radii


def test_gradients_match_central_differences():
    P, cols, radii = _fd_scene()
    H, W, step = 48, 64, 1e-7
    hits = rrm.hit_sets(P, radii, K0, H, W)
    pix, ids, _ = hits
    assert len(np.unique(ids)) == len(P) and np.bincount(pix).max() >= 3
    # no candidate lies within the difference step of a rho = r threshold (in rho or in r): the hit sets do not move
    w, h, f, ccx, ccy = rm.camera(K0, H, W)
    ii, jj = np.mgrid[0:h, 0:w]
    for k in range(len(P)):
        margin = np.abs(rm.rho(P[k][None], ii.ravel(), jj.ravel(), f, ccx, ccy) - radii[k]).min()
        assert margin > 10 * step, (k, margin)
    g = np.random.default_rng(0).normal(size=(H, W, 3))

    def L(p, c, r):      # float64 throughout: the blend without its float32 roundings, at the fixed hit sets
        img = rrm.blend(torch.from_numpy(p), torch.from_numpy(c), torch.from_numpy(r), hits, K0, H, W, bg=(0.1, 0.2, 0.3))
        return float((img * torch.from_numpy(g)).sum())

    # _round32 inside the blend would snap a perturbed input back: difference the unrounded expression instead
    orig = rrm._round32
    rrm._round32 = lambda t: t
    try:
        gp, gc, gr = rrm.grads(P, cols, radii, g, hits, K0, H, W, bg=(0.1, 0.2, 0.3))
        for arr, grad, name in ((P, gp, "P"), (cols, gc, "c"), (radii, gr, "r")):
            fd = np.zeros_like(arr)
            for idx in np.ndindex(*arr.shape):
                a, b = arr.copy(), arr.copy()
                a[idx] += step
                b[idx] -= step
                args = {"P": (a, cols, radii), "c": (P, a, radii), "r": (P, cols, a)}[name]
                brgs = {"P": (b, cols, radii), "c": (P, b, radii), "r": (P, cols, b)}[name]
                fd[idx] = (L(*args) - L(*brgs)) / (2 * step)
            scale = np.abs(grad).max()
            assert scale > 0, name
            # central differences of step 1e-7 on values of order 1: truncation ~ step^2 f''' and cancellation
            # ~ 1e-16 |L| / step ~ 1e-8 relative to gradients of order |L| / r
            np.testing.assert_allclose(fd, grad, rtol=0, atol=1e-5 * scale, err_msg=name)
    finally:
        rrm._round32 = orig
    # with the roundings in place (identities on these inputs) the gradients are the same
    gp2, gc2, gr2 = rrm.grads(P, cols, radii, g, hits, K0, H, W, bg=(0.1, 0.2, 0.3))
    for a, b in ((gp, gp2), (gc, gc2), (gr, gr2)):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)


def test_blend_equals_the_forward_and_the_one_radius_gradients():
    import render_color_grad_model as rcm
    import render_grad_model as rgm
    P, cols, radii = _fd_scene()
    hits = rrm.hit_sets(P, radii, K0, 48, 64)
    img = rrm.blend(torch.from_numpy(P), torch.from_numpy(cols), torch.from_numpy(radii), hits, K0, 48, 64, bg=(0.1, 0.2, 0.3))
    want = rrm.render(P, cols, radii, K0, 48, 64, bg=(0.1, 0.2, 0.3))
    np.testing.assert_allclose(img.numpy(), want["img"], rtol=0, atol=1e-13)
    # all radii equal: hit sets and dL/dP, dL/dc are those of the one-radius models
    r = float(np.float32(0.04))
    eq = np.full(len(P), r)
    h1, h2 = rrm.hit_sets(P, eq, K0, 48, 64), rgm.hit_sets(P, K0, 48, 64, r)
    for a, b in zip(h1, h2):
        np.testing.assert_array_equal(a, b)
    g = np.random.default_rng(1).normal(size=(48, 64, 3))
    gp, gc, gr = rrm.grads(P, cols, eq, g, h1, K0, 48, 64)
    wp, wc = rcm.grads(P, cols, g, K0, 48, 64, r)
    np.testing.assert_allclose(gp, wp, rtol=0, atol=1e-12 * np.abs(wp).max())
    np.testing.assert_allclose(gc, wc, rtol=0, atol=1e-12 * np.abs(wc).max())
    assert np.abs(gr).max() > 0
