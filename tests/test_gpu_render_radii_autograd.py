"""``Pulsar`` with a per-point ``rad`` (super_amd/renderer.py): the plain forward, the autograd node with dL/drad, the
shapes that are refused, and ``render_img`` with ``opt.renderer_surfel_radii``.  Needs an MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest

import render_radii_cases as rc
import render_radii_model as rrm

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3)


def _inputs(s):
    import torch
    P = torch.as_tensor(s["P"]).cuda()
    cols = torch.as_tensor(s["cols"]).cuda()
    rad = torch.as_tensor(s["radii"]).cuda()
    return P, cols, rad, {"K": torch.as_tensor(s["K"]).float()[None].cuda()}


def _direct(s, g):
    """image and the three gradients through render_points / render_backward_ex"""
    import torch
    from super_amd.renderer import DEFAULT_RAD, RenderContext, render_backward_ex, render_params, render_points
    P, cols, rad, _ = _inputs(s)
    ctx = RenderContext(s["H"], s["W"])
    p = render_params(torch.as_tensor(s["K"]).float()[None], s["H"], s["W"], s["view_scale"], DEFAULT_RAD, BG)
    img = render_points(ctx, p, P, cols, radii=rad)
    return (img,) + render_backward_ex(ctx, p, g, radii=True)


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("name", ["mixed", "mixed_half"])
def test_pulsar_gives_the_radius_gradient(name, interleaved):
    import torch
    from super_amd.renderer import Pulsar
    f = rc.facts(name)
    s = f["scene"]
    g = torch.from_numpy(f["g"]).float().double().cuda()      # the image is float32: so is the gradient autograd hands back
    img0, gp0, gc0, gr0 = _direct(s, g)
    P, cols, rad, inputs = _inputs(s)
    r = Pulsar(SimpleNamespace(height=s["H"], width=s["W"]), differentiable=True)
    P.requires_grad_(True), cols.requires_grad_(True), rad.requires_grad_(True)
    img = r(inputs, SimpleNamespace(points=P, colors=cols), view_scale=s["view_scale"], rad=rad, bg_col=torch.tensor(BG))
    assert img.requires_grad and torch.equal(img.detach(), img0)
    if interleaved:     # another render moves the context's serial: the backward renders its saved inputs again
        other = r(inputs, SimpleNamespace(points=P.detach() + 0.01, colors=cols.detach()), view_scale=s["view_scale"],
                  rad=0.02)
        assert not torch.equal(other, img0)
    (img.double() * g).sum().backward()
    assert P.grad.dtype == torch.float64 and rad.grad.dtype == torch.float32 and tuple(rad.grad.shape) == tuple(rad.shape)
    assert torch.equal(P.grad, gp0) and torch.equal(cols.grad, gc0.float()) and torch.equal(rad.grad, gr0.float())
    assert float(rad.grad.abs().max()) > 0
    # only the radii require grad: the same dL/drad, nothing for the others
    P2, cols2, rad2, _ = _inputs(s)
    rad2 = rad2.double().requires_grad_(True)
    img = r(inputs, SimpleNamespace(points=P2, colors=cols2), view_scale=s["view_scale"], rad=rad2, bg_col=torch.tensor(BG))
    (img.double() * g).sum().backward()
    assert rad2.grad.dtype == torch.float64 and torch.equal(rad2.grad, gr0) and P2.grad is None and cols2.grad is None


def test_rad_shapes_and_refusals():
    import torch
    from super_amd.renderer import Pulsar, render_points, RenderContext, render_params
    s = rc.facts("inside")["scene"]
    P, cols, rad, inputs = _inputs(s)
    n = len(P)
    data = SimpleNamespace(points=P, colors=cols)
    plain = Pulsar(SimpleNamespace(height=48, width=64))
    diff = Pulsar(SimpleNamespace(height=48, width=64), differentiable=True)
    want = rrm.render(s["P"], s["cols"], s["radii"], s["K"], 48, 64, bg=BG)
    for r in (plain, diff):
        img, fid, cnt = r.render(inputs, data, rad=rad, bg_col=torch.tensor(BG), with_info=True)
        ok = ~want["near"]
        np.testing.assert_allclose(img.cpu().numpy()[ok], want["img"][ok], rtol=0, atol=1e-5)
        np.testing.assert_array_equal(cnt.cpu().numpy()[ok], want["count"][ok])
        # a number and a one-element tensor are the one radius, as before
        a = r(inputs, data, rad=0.02)
        assert torch.equal(a, r(inputs, data, rad=torch.tensor(0.02, dtype=torch.float64)))
        assert torch.equal(a, r(inputs, data, rad=torch.tensor([0.02], dtype=torch.float64, device="cuda")))
        for bad in (torch.ones(n + 1), torch.ones(n, 1), torch.ones(2, n), torch.ones(0)):
            with pytest.raises(ValueError, match="rad must be"):
                r(inputs, data, rad=bad)
    with pytest.raises(RuntimeError, match="forward only"):
        plain(inputs, data, rad=rad.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="rad is a constant"):
        diff(inputs, data, rad=torch.tensor([0.02], requires_grad=True))
    ctx = RenderContext(48, 64)
    p = render_params(inputs["K"], 48, 64, 1.0, 2e-4)
    with pytest.raises(ValueError, match="radii must be"):
        render_points(ctx, p, P, cols, radii=rad[:-1])


def test_render_img_with_the_surfels_own_radii():
    import torch
    from super_amd.renderer import conf2color, render_img
    sc, stable, cols, radii, _ = rc.graphfit_scene()
    confs = np.random.default_rng(8).uniform(0.0, 1.0, sc.N)
    scale = 1.5

    def surfels(**opt):
        return SimpleNamespace(points=torch.from_numpy(sc.sf_points).cuda(), colors=torch.from_numpy(cols).double().cuda(),
                               radii=torch.from_numpy(radii).cuda(), confs=torch.from_numpy(confs).cuda(),
                               isStable=torch.from_numpy(stable).cuda(),
                               opt=SimpleNamespace(height=sc.H, width=sc.W, renderer_rad=2e-3, **opt))

    inputs = {"K": torch.from_numpy(sc.K).float()[None].cuda()}
    sf = surfels(renderer_surfel_radii=True, renderer_radii_scale=scale)
    render_img(sf, inputs)
    heat = conf2color(torch.from_numpy(confs)).numpy()[stable]
    for img, c in ((sf.renderImg, cols[stable]), (sf.renderImg_conf_heat, heat)):
        want = rrm.render(sc.sf_points[stable], c, radii[stable] * scale, sc.K, sc.H, sc.W)
        got = img[0].permute(1, 2, 0).cpu().numpy()
        ok = ~want["near"]
        assert (~ok).sum() <= 0.005 * ok.size
        np.testing.assert_allclose(got[ok], want["img"][ok], rtol=0, atol=1e-5)
    # the flag absent or False: the one radius opt.renderer_rad, as before
    a, b = surfels(), surfels(renderer_surfel_radii=False, renderer_radii_scale=scale)
    render_img(a, inputs), render_img(b, inputs)
    assert torch.equal(a.renderImg, b.renderImg) and not torch.equal(a.renderImg, sf.renderImg)
