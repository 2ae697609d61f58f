"""The CPU restatement of the render loss (tests/render_grad_model.py) pinned on its own: its image equals
render_model's, its autograd gradient equals central finite differences on hand-built scenes, and its SSIM loss
equals a direct numpy evaluation.  Tolerances: 1e-6 relative (of the largest entry) on the finite differences,
1e-12 on the rest."""
import numpy as np
import pytest
import torch

import render_grad_model as rgm
import render_model as rm

K1 = np.array([[40.0, 0, 12.0], [0, 40.0, 10.0], [0, 0, 1]])
H1, W1 = 20, 24
DZ = 1e-5 * (rm.Z_FAR - rm.Z_NEAR)           # 1e-5 apart in zt
ZB = rm.Z_FAR - 0.5 * rm.GAMMA * (rm.Z_FAR - rm.Z_NEAR)   # zt = gamma / 2
SCENES = {
    # one sphere off the axis, half a gamma in front of the background's depth (else w_bg underflows and the colour is
    # c_k wherever it is hit): the rho term
    "off_axis": ([[0.013 * ZB, -0.007 * ZB, ZB]], 0.05 * ZB, rm.N_TRACK),
    # two overlapping spheres 1e-5 apart in zt: the depth term
    "two_close": ([[0.01, 0.0, 1.0], [-0.012, 0.004, 1.0 + DZ]], 0.05, rm.N_TRACK),
    # four spheres on pixels with more than n_track = 2 hits: the cut
    "cut": ([[0.0, 0.0, 1.0], [0.004, 0.0, 1.0 + DZ], [-0.004, 0.003, 1.0 + 2 * DZ], [0.002, -0.003, 1.0 + 0.3 * DZ]],
            0.05, 2),
}


def _scene(name):
    P, rad, nt = SCENES[name]
    rng = np.random.default_rng(3)
    cols = rng.uniform(0.1, 0.9, size=(len(P), 3)).astype(np.float32)
    g = rng.normal(size=(H1, W1, 3))
    return np.array(P, np.float64), cols, rad, nt, g


@pytest.mark.parametrize("name", list(SCENES))
def test_autograd_matches_finite_differences(name):
    P, cols, rad, nt, g = _scene(name)
    hits = rgm.hit_sets(P, K1, H1, W1, rad, n_track=nt)
    bg = (0.2, 0.3, 0.4)
    gt = torch.from_numpy(g)

    def L(Pt):
        return (rgm.blend(Pt, cols, hits, K1, H1, W1, rad, bg=bg, round32=False) * gt).sum()

    Pt = torch.from_numpy(P).requires_grad_(True)
    L(Pt).backward()
    ag = Pt.grad.numpy()
    fd = np.zeros_like(P)
    h = 1e-9
    for k in range(P.shape[0]):
        for c in range(3):
            a, b = P.copy(), P.copy()
            a[k, c] += h
            b[k, c] -= h
            fd[k, c] = (float(L(torch.from_numpy(a))) - float(L(torch.from_numpy(b)))) / (2 * h)
    scale = np.abs(ag).max()
    assert scale > 0
    np.testing.assert_allclose(ag, fd, rtol=0, atol=1e-6 * scale)
    if name == "two_close":
        assert np.abs(ag[:, 2]).max() > 1e3           # the depth term is in play
    if name == "cut":
        count = np.bincount(hits[0], minlength=H1 * W1)
        assert count.max() == 2 and (rm.render(P, cols, K1, H1, W1, rad, n_track=3)["count"] == 3).any()


def test_gradient_is_zero_at_rho_zero_and_finite():
    P = np.array([[0.0, 0.0, 1.0]])                       # on the ray of pixel (10, 12): rho = 0 there
    cols = np.array([[0.5, 0.25, 0.75]], np.float32)
    Pt = torch.from_numpy(P).requires_grad_(True)
    img = rgm.render(Pt, cols, K1, H1, W1, 0.05)
    img[10, 12].sum().backward()
    assert torch.isfinite(Pt.grad).all()
    np.testing.assert_allclose(Pt.grad.numpy()[0, :2], 0.0, atol=1e-12)


def test_image_equals_render_model():
    from super_amd import synth
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    rng = np.random.default_rng(12)
    cols = rng.uniform(size=(sc.N, 3)).astype(np.float32)
    for nt in (rm.N_TRACK, 3):
        want = rm.render(sc.sf_points, cols, sc.K, sc.H, sc.W, 0.01, bg=(0.1, 0.2, 0.3), n_track=nt)
        hits = rgm.hit_sets(sc.sf_points, sc.K, sc.H, sc.W, 0.01, n_track=nt)
        got = rgm.blend(torch.from_numpy(sc.sf_points), cols, hits, sc.K, sc.H, sc.W, 0.01, bg=(0.1, 0.2, 0.3)).numpy()
        ok = ~want["near"]
        np.testing.assert_allclose(got[ok], want["img"][ok], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(np.bincount(hits[0], minlength=sc.H * sc.W).reshape(sc.H, sc.W)[ok],
                                      want["count"][ok])


def _ssim_numpy(img, tgt, weight):
    """direct loops: reflected 11x11 windows, clipped windows for the mask"""
    h, w, _ = img.shape
    ref = lambda k, n: -k if k < 0 else (2 * n - 2 - k if k >= n else k)
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = np.zeros((h, w))
    valid = np.zeros((h, w), bool)
    for i in range(h):
        for j in range(w):
            S = []
            for c in range(3):
                xs = np.array([[img[ref(i + a, h), ref(j + b, w), c] for b in range(-5, 6)] for a in range(-5, 6)])
                ys = np.array([[tgt[c, ref(i + a, h), ref(j + b, w)] for b in range(-5, 6)] for a in range(-5, 6)])
                mx, my = xs.mean(), ys.mean()
                sx, sy, sxy = (xs * xs).mean() - mx * mx, (ys * ys).mean() - my * my, (xs * ys).mean() - mx * my
                n = (2 * mx * my + C1) * (2 * sxy + C2)
                d = (mx * mx + my * my + C1) * (sx + sy + C2)
                S.append(min(max((1 - n / d) / 2, 0.0), 1.0))
            m[i, j] = np.mean(S) ** 2
            win = img[max(i - 5, 0):i + 6, max(j - 5, 0):j + 6]
            valid[i, j] = win.min() > 0
    sel = valid & (m < 0.1)
    return weight * m[sel].sum(), int(sel.sum()), m


def test_ssim_matches_direct_numpy():
    rng = np.random.default_rng(8)
    h, w = 13, 17
    base = rng.uniform(0.2, 0.8, size=(h, w, 3))
    img = base + 0.02 * rng.normal(size=(h, w, 3))
    img[0, 3] = 0.0                                 # a black pixel: the windows that see it are not valid
    img[12, 16, 1] = -0.1
    tgt = np.transpose(base, (2, 0, 1)) + 0.02 * rng.normal(size=(3, h, w))
    loss, kept, m, _ = rgm.ssim_loss(torch.from_numpy(img), torch.from_numpy(tgt), 0.5)
    want_loss, want_kept, want_m = _ssim_numpy(img, tgt, 0.5)
    np.testing.assert_allclose(m.numpy(), want_m, rtol=1e-12, atol=0)
    assert kept == want_kept and 0 < kept < h * w
    assert abs(float(loss) - want_loss) <= 1e-12 * abs(want_loss)
