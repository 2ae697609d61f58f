"""The CPU restatement of the colour gradient (tests/render_color_grad_model.py) pinned on its own: at fixed hit sets the
image is linear in the colours, so its autograd gradient equals central finite differences to round-off; its image
and point gradient equal render_grad_model's; the colour gradient equals the spec's sum g w_k / W written out."""
import numpy as np
import pytest
import torch

import render_color_grad_model as rcm
import render_grad_model as rgm
import render_model as rm

K1 = np.array([[40.0, 0, 12.0], [0, 40.0, 10.0], [0, 0, 1]])
H1, W1 = 20, 24
DZ = 1e-5 * (rm.Z_FAR - rm.Z_NEAR)           # 1e-5 apart in zt
ZB = rm.Z_FAR - 0.5 * rm.GAMMA * (rm.Z_FAR - rm.Z_NEAR)   # zt = gamma / 2: w_bg does not underflow
SCENES = {
    # one sphere in front of the background's depth: the colour shares its pixels with bg
    "bg": ([[0.013 * ZB, -0.007 * ZB, ZB]], 0.05 * ZB, rm.N_TRACK),
    # two overlapping spheres 1e-5 apart in zt: both weights in play
    "two_close": ([[0.01, 0.0, 1.0], [-0.012, 0.004, 1.0 + DZ]], 0.05, rm.N_TRACK),
    # four spheres on pixels with more than n_track = 2 hits: the cut
    "cut": ([[0.0, 0.0, 1.0], [0.004, 0.0, 1.0 + DZ], [-0.004, 0.003, 1.0 + 2 * DZ], [0.002, -0.003, 1.0 + 0.3 * DZ]],
            0.05, 2),
}
BG = (0.2, 0.3, 0.4)


def _scene(name):
    P, rad, nt = SCENES[name]
    rng = np.random.default_rng(3)
    cols = rng.uniform(0.1, 0.9, size=(len(P), 3)).astype(np.float32).astype(np.float64)
    g = rng.normal(size=(H1, W1, 3))
    return np.array(P, np.float64), cols, rad, nt, g


@pytest.mark.parametrize("name", list(SCENES))
def test_colour_gradient_matches_finite_differences(name):
    P, cols, rad, nt, g = _scene(name)
    hits = rgm.hit_sets(P, K1, H1, W1, rad, n_track=nt)
    gt = torch.from_numpy(g)
    Pt = torch.from_numpy(P)

    def L(c):
        return (rcm.blend(Pt, c, hits, K1, H1, W1, rad, bg=BG) * gt).sum()

    Ct = torch.from_numpy(cols).requires_grad_(True)
    L(Ct).backward()
    ag = Ct.grad.numpy()
    fd = np.zeros_like(cols)
    h = 2.0 ** -10                               # the f32 rounding of c +- h is exact: the blend is linear in c
    for k in range(cols.shape[0]):
        for c in range(3):
            a, b = cols.copy(), cols.copy()
            a[k, c] += h
            b[k, c] -= h
            fd[k, c] = (float(L(torch.from_numpy(a))) - float(L(torch.from_numpy(b)))) / (2 * h)
    scale = np.abs(ag).max()
    reach = np.abs(ag).max(1) > 0
    assert scale > 0
    # every sphere reaches a pixel, but with n_track = 2 the cut leaves one out everywhere
    assert reach.sum() == len(P) - (name == "cut")
    np.testing.assert_allclose(ag, fd, rtol=0, atol=1e-9 * scale)


@pytest.mark.parametrize("name", list(SCENES))
def test_image_and_point_gradient_equal_render_grad_model(name):
    P, cols, rad, nt, g = _scene(name)
    hits = rgm.hit_sets(P, K1, H1, W1, rad, n_track=nt)
    a = torch.from_numpy(P).requires_grad_(True)
    b = torch.from_numpy(P).requires_grad_(True)
    ia = rcm.blend(a, torch.from_numpy(cols), hits, K1, H1, W1, rad, bg=BG)
    ib = rgm.blend(b, cols.astype(np.float32), hits, K1, H1, W1, rad, bg=BG)
    np.testing.assert_allclose(ia.detach().numpy(), ib.detach().numpy(), rtol=0, atol=1e-15)
    (ia * torch.from_numpy(g)).sum().backward()
    (ib * torch.from_numpy(g)).sum().backward()
    np.testing.assert_allclose(a.grad.numpy(), b.grad.numpy(), rtol=0, atol=1e-12 * np.abs(b.grad.numpy()).max())


def test_colour_gradient_is_the_spec_sum():
    """dL/dc_k = sum over the pixels k takes part in of g w_k / W, written out pixel by pixel"""
    P, cols, rad, nt, g = _scene("cut")
    pix, ids, rank = rgm.hit_sets(P, K1, H1, W1, rad, n_track=nt)
    w, h, f, ccx, ccy = rm.camera(K1, H1, W1)
    P32 = P.astype(np.float32).astype(np.float64)
    want = np.zeros_like(cols)
    for q in np.unique(pix):
        at = pix == q
        i, j = divmod(int(q), w)
        ks, zt = ids[at], (rm.Z_FAR - P32[ids[at], 2]) / (rm.Z_FAR - rm.Z_NEAR)
        zmax = zt[rank[at] == 0][0]
        r = rm.rho(P32[ks], np.full(len(ks), i), np.full(len(ks), j), f, ccx, ccy)
        wk = (1.0 - r / rad) * np.exp((zt - zmax) / rm.GAMMA)
        Wp = wk.sum() + np.exp((rm.BG_EPS - zmax) / rm.GAMMA)
        for k, wkk in zip(ks, wk):
            want[k] += g[i, j] * wkk / Wp
    _, got = rcm.grads(P, cols, g, K1, H1, W1, rad, bg=BG, n_track=nt)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * np.abs(want).max())


def test_no_points_and_all_culled_give_zero():
    g = np.ones((H1, W1, 3))
    gp, gc = rcm.grads(np.zeros((0, 3)), np.zeros((0, 3)), g, K1, H1, W1, 0.05)
    assert gp.shape == gc.shape == (0, 3)
    P = np.array([[0, 0, 0.005], [0, 0, 20.0], [0, 0, -1.0], [50.0, 0, 1.0]])
    gp, gc = rcm.grads(P, np.ones((4, 3)), g, K1, H1, W1, 0.05)
    assert (gc == 0).all() and (gp == 0).all()
