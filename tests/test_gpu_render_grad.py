"""The renderer backward (slm_render_backward) and the SSIM render loss (slm_render_ssim_loss) against the CPU
restatement of tests/render_grad_model.py.  Needs an MI355X.

Backward: dL/dpoints for a random dL/dimage equals the model's autograd at the same hit sets to 1e-9 of the largest
entry; points that are a candidate of a pixel the forward model marks `near` (a decision at its threshold) are left
out.  SSIM: the HIP render itself is fed to both; loss, kept count and dL/dimage agree to 1e-12 relative."""
import ctypes as C

import numpy as np
import pytest

import render_grad_model as rgm
import render_model as rm

pytestmark = pytest.mark.gpu

RAD = 0.01          # a filled render of the 60x80 scene (as test_gpu_graphfit_renderimg.py)
K0 = np.array([[100.0, 0, 32.0], [0, 100.0, 24.0], [0, 0, 1]])


def _scene(seed=31):
    from super_amd import synth
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=seed, src_border=1, tgt_border=3)
    rng = np.random.default_rng(12)
    return sc, rng.uniform(size=(sc.N, 3)).astype(np.float32)


def _hip(P, cols, K, H, W, rad, g, n_track=rm.N_TRACK, bg=(0.0, 0.0, 0.0)):
    import torch
    from super_amd.renderer import RenderContext, render_backward, render_params, render_points
    ctx = RenderContext(H, W)
    p = render_params(torch.as_tensor(K)[None], H, W, 1.0, rad, bg)
    p.n_track = n_track
    img = render_points(ctx, p, torch.as_tensor(P).cuda(), torch.as_tensor(cols).cuda())
    gp = render_backward(ctx, p, torch.as_tensor(g).cuda())
    return ctx, p, img, gp


def _excluded(P, K, H, W, rad, near):
    """points with a candidate pixel (silhouette box padded by half a pixel) that is near"""
    P32 = np.asarray(P, np.float64).astype(np.float32).astype(np.float64)
    w, h, f, ccx, ccy = rm.camera(K, H, W)
    x0, x1 = rm._range(P32[:, 0], P32[:, 2], rad, f, ccx, w, 0.5)
    y0, y1 = rm._range(P32[:, 1], P32[:, 2], rad, f, ccy, h, 0.5)
    S = np.zeros((h + 1, w + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(near, 0), 1)
    ok = (x0 <= x1) & (y0 <= y1)
    a, b, c, d = np.clip(y0, 0, h), np.clip(y1 + 1, 0, h), np.clip(x0, 0, w), np.clip(x1 + 1, 0, w)
    cnt = S[b, d] - S[a, d] - S[b, c] + S[a, c]
    return ok & (cnt > 0)


def _model_grad(P, cols, K, H, W, rad, g, n_track=rm.N_TRACK, bg=(0.0, 0.0, 0.0)):
    import torch
    Pt = torch.from_numpy(np.asarray(P, np.float64)).requires_grad_(True)
    img = rgm.render(Pt, cols, K, H, W, rad, bg=bg, n_track=n_track)
    (img * torch.from_numpy(g)).sum().backward()
    return Pt.grad.numpy()


def _compare(P, cols, K, H, W, rad, n_track=rm.N_TRACK, bg=(0.0, 0.0, 0.0), seed=0):
    w, h = rm.camera(K, H, W)[:2]
    g = np.random.default_rng(seed).normal(size=(h, w, 3))
    _, _, _, gp = _hip(P, cols, K, H, W, rad, g, n_track, bg)
    got = gp.cpu().numpy()
    want = _model_grad(P, cols, K, H, W, rad, g, n_track, bg)
    near = rm.render(P, cols, K, H, W, rad, bg=bg, n_track=n_track)["near"]
    ex = _excluded(P, K, H, W, rad, near)
    assert ex.mean() < 0.05, ex.mean()
    scale = np.abs(want).max()
    assert scale > 0
    np.testing.assert_allclose(got[~ex], want[~ex], rtol=0, atol=1e-9 * scale)
    return got, want


@pytest.mark.parametrize("n_track", [rm.N_TRACK, 3])
def test_backward_matches_the_model(n_track):
    sc, cols = _scene()
    got, want = _compare(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, n_track, bg=(0.1, 0.2, 0.3))
    assert (np.abs(want).max(1) > 0).mean() > 0.5            # most points reach a pixel


def test_backward_on_the_overflow_path():
    """6000 surfels in one 16x16 tile: more keys than the 4096 the LDS sort holds"""
    rng = np.random.default_rng(4)
    n = 6000
    Z = rng.uniform(0.5, 3.0, n)
    u, v = rng.uniform(17.5, 30.5, n), rng.uniform(17.5, 30.5, n)
    P = np.stack([(u - 32.0) * Z / 100.0, (v - 24.0) * Z / 100.0, Z], 1)
    cols = rng.uniform(size=(n, 3)).astype(np.float32)
    rad = 1.0 * Z.min() / 100.0
    _compare(P, cols, K0, 48, 64, rad)


def test_backward_of_no_points_and_all_culled():
    g = np.ones((48, 64, 3))
    _, _, _, gp = _hip(np.zeros((0, 3)), np.zeros((0, 3), np.float32), K0, 48, 64, 0.02, g)
    assert tuple(gp.shape) == (0, 3)
    P = np.array([[0, 0, 0.005], [0, 0, 20.0], [0, 0, -1.0], [50.0, 0, 1.0]])
    _, _, _, gp = _hip(P, np.ones((4, 3), np.float32), K0, 48, 64, 0.02, g)
    assert tuple(gp.shape) == (4, 3) and (gp == 0).all()


def test_backward_is_bitwise_reproducible_and_refuses_a_mismatch():
    import torch
    from super_amd import _lib
    from super_amd.renderer import RenderContext, render_backward, render_params
    sc, cols = _scene()
    g = np.random.default_rng(1).normal(size=(sc.H, sc.W, 3))
    ctx, p, _, a = _hip(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, g)
    b = render_backward(ctx, p, torch.from_numpy(g).cuda())
    assert torch.equal(a, b)
    _, _, _, c = _hip(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, g)     # a fresh context
    assert torch.equal(a, c)
    gd = torch.from_numpy(g).cuda()
    out = torch.empty((sc.N, 3), dtype=torch.float64, device="cuda")
    q = render_params(torch.as_tensor(sc.K)[None], sc.H, sc.W, 1.0, RAD * 1.5)
    lib = ctx.lib
    rc = lib.slm_render_backward(ctx.h, C.byref(q), gd.data_ptr(), out.data_ptr(), None)
    assert rc == _lib.SLM_ERR_INVALID
    fresh = RenderContext(sc.H, sc.W)
    rc = lib.slm_render_backward(fresh.h, C.byref(p), gd.data_ptr(), out.data_ptr(), None)
    assert rc == _lib.SLM_ERR_INVALID
    torch.cuda.synchronize()


def test_gf_render_backward_by_surfel_row():
    import torch
    from helpers import GF_CORR_VARIANTS, torch_frame
    from oracle import graphfit_oracle as gfo
    from super_amd.deform_mesh import GraphFit
    from super_amd.renderer import render_backward
    sc, cols = _scene()
    stable = np.random.default_rng(12).uniform(size=sc.N) > 0.1
    sf, inputs, new_data = torch_frame(sc)
    sf.isStable = torch.from_numpy(stable).cuda()
    o = gfo.default_opt(**GF_CORR_VARIANTS["corr"])
    o.deform_udpate_method, o.sf_corr_match_renderimg, o.renderer, o.renderer_rad = "super_edg", True, "pulsar", RAD
    gf = GraphFit(o)
    gf._bind(0, inputs, sf, new_data, None, defer_flow=True)
    img, p = gf._render_deformed_hwc(inputs, torch.from_numpy(cols).cuda())
    g = np.random.default_rng(2).normal(size=(sc.H, sc.W, 3))
    got = render_backward(gf._render_ctx, p, torch.from_numpy(g).cuda()).cpu().numpy()
    assert got.shape == (sc.N, 3)
    assert (got[~stable] == 0).all()
    P = sc.sf_points[stable]
    want = _model_grad(P, cols[stable], sc.K, sc.H, sc.W, RAD, g)
    near = rm.render(P, cols[stable], sc.K, sc.H, sc.W, RAD)["near"]
    ex = _excluded(P, sc.K, sc.H, sc.W, RAD, near)
    np.testing.assert_allclose(got[stable][~ex], want[~ex], rtol=0, atol=1e-9 * np.abs(want).max())


def _ssim_inputs():
    """the HIP render of the scene and a target: the render of the scene moved by a few pixels, plus noise"""
    import torch
    sc, cols = _scene()
    _, _, img, _ = _hip(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, np.zeros((sc.H, sc.W, 3)))
    tg = rm.render(sc.sf_points + np.array([0.004, -0.002, 0.0]), cols, sc.K, sc.H, sc.W, RAD)["img"]
    tgt = np.transpose(tg, (2, 0, 1)) + 0.01 * np.random.default_rng(5).normal(size=(3, sc.H, sc.W))
    return img, torch.from_numpy(tgt.astype(np.float32))


def test_ssim_loss_matches_the_model():
    import torch
    from super_amd.renderer import ssim_render_loss
    img, tgt = _ssim_inputs()
    weight = 0.37
    loss, kept, grad = ssim_render_loss(img, tgt.cuda(), weight)
    x = img.cpu().double().requires_grad_(True)
    t64 = tgt.double()
    want, want_kept, m, v = rgm.ssim_loss(x, t64, weight)
    want.backward()
    # the scene keeps its decisions away from the thresholds (0.1 for m, 0 and 1 for the clamp)
    _, valid = rgm.ssim_parts(x.detach(), t64)
    valid = valid[0, 0].numpy()
    assert np.abs(m.numpy() - 0.1)[valid].min() > 1e-6
    assert np.minimum(np.abs(v.numpy()), np.abs(v.numpy() - 1)).transpose(1, 2, 0)[valid].min() > 1e-6
    assert kept == want_kept > 100
    want = float(want.detach())
    assert abs(loss - want) <= 1e-12 * abs(want)
    gw = x.grad.numpy()
    np.testing.assert_allclose(grad.cpu().numpy(), gw, rtol=0, atol=1e-12 * np.abs(gw).max())
    # bitwise reproducible; without the gradient the loss is the same
    loss2, kept2, grad2 = ssim_render_loss(img, tgt.cuda(), weight)
    assert loss2 == loss and kept2 == kept and torch.equal(grad, grad2)
    loss3, kept3, none = ssim_render_loss(img, tgt[None].cuda(), weight, with_grad=False)
    assert loss3 == loss and kept3 == kept and none is None


def test_ssim_loss_of_an_all_background_image_is_zero():
    import torch
    from super_amd.renderer import ssim_render_loss
    img = torch.zeros((48, 64, 3), device="cuda")
    loss, kept, grad = ssim_render_loss(img, torch.rand((3, 48, 64), device="cuda"), 1.0)
    assert loss == 0.0 and kept == 0 and (grad == 0).all()
