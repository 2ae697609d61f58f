"""The Python side of the N-channel render (super_amd/renderer.py): the autograd node with its recompute rule,
``Pulsar.render_channels``, ``render_points`` keeping its cut to three columns, and ``render_`` with
``opt.renderer_one_pass``.  Needs an MI355X."""
from types import SimpleNamespace

import numpy as np
import pytest

import render_channels_cases as cc
import render_channels_model as rcm
import render_radii_cases as rc

pytestmark = pytest.mark.gpu


def _inputs(s, nch):
    import torch
    P = torch.as_tensor(s["P"]).cuda()
    feat = torch.as_tensor(cc.features("mixed", nch)).cuda()
    rad = torch.as_tensor(s["radii"]).cuda()
    return P, feat, rad, {"K": torch.as_tensor(s["K"]).float()[None].cuda()}


@pytest.mark.parametrize("interleaved", [False, True])
def test_the_autograd_node_matches_the_model(interleaved):
    import torch
    from super_amd.renderer import DEFAULT_RAD, RenderContext, render_channels, render_channels_differentiable, render_params
    f = rc.facts("mixed")
    s, ex = f["scene"], f["ex"]
    # the image is float32, so autograd hands the node dL/dimage rounded to float32: the model gets the same numbers
    g64 = cc.grad_facts("mixed", 4)["g"].astype(np.float32).astype(np.float64)
    want = rcm.grads(s["P"], cc.features("mixed", 4), s["radii"], g64, f["hits"], s["K"], s["H"], s["W"], s["view_scale"],
                     bg=cc.bg(4))
    P, feat, rad, inputs = _inputs(s, 4)
    feat, rad = feat.double(), rad.double()                    # gradients come back in the inputs' dtypes
    P.requires_grad_(True), feat.requires_grad_(True), rad.requires_grad_(True)
    ctx = RenderContext(s["H"], s["W"])
    p = render_params(inputs["K"], s["H"], s["W"], s["view_scale"], DEFAULT_RAD)
    img = render_channels_differentiable(ctx, p, P, feat, bg=cc.bg(4), radii=rad)
    assert img.requires_grad and tuple(img.shape) == (100, 150, 4) and img.dtype == torch.float32
    ok = ~cc.want("mixed", 4)["near"]
    np.testing.assert_allclose(img.detach().cpu().numpy()[ok], cc.want("mixed", 4)["img"][ok], rtol=0, atol=1e-5)
    if interleaved:     # another render moves the context's serial: the backward renders its saved inputs again
        other = render_channels(ctx, p, P.detach() + 0.01, feat.detach()[:, :2], radii=rad.detach())
        assert tuple(other.shape) == (100, 150, 2)
    (img.double() * torch.from_numpy(g64).cuda()).sum().backward()
    assert all(t.grad.dtype == torch.float64 and tuple(t.grad.shape) == tuple(t.shape) for t in (P, feat, rad))
    for got, w, what in zip((P.grad, feat.grad, rad.grad), want, ("dL/dP", "dL/df", "dL/dr")):
        got = got.cpu().numpy()
        scale = np.abs(w).max()
        print(what, "scale", scale, "max err", np.abs(got[~ex] - w[~ex]).max() / scale)
        assert scale > 0
        np.testing.assert_allclose(got[~ex], w[~ex], rtol=0, atol=1e-9 * scale, err_msg=what)


def test_pulsar_render_channels_shapes_and_refusals():
    import torch
    from super_amd.renderer import Pulsar, RenderContext, render_channels, render_params
    s = rc.facts("mixed")["scene"]
    P, feat, rad, inputs = _inputs(s, 6)
    n = len(P)
    data = SimpleNamespace(points=P, colors=None)
    opt = SimpleNamespace(height=s["H"], width=s["W"])
    plain, diff = Pulsar(opt), Pulsar(opt, differentiable=True)
    want = cc.want("mixed", 6)
    ok = ~want["near"]
    for r in (plain, diff):
        img, fid, cnt = r.render_channels(inputs, data, feat, rad=rad, bg=cc.bg(6), with_info=True)
        assert tuple(img.shape) == (100, 150, 6) and tuple(fid.shape) == (100, 150) and not img.requires_grad
        np.testing.assert_allclose(img.cpu().numpy()[ok], want["img"][ok], rtol=0, atol=1e-5)
        np.testing.assert_array_equal(cnt.cpu().numpy()[ok], want["count"][ok])
        half = r.render_channels(inputs, data, feat[:, :1], view_scale=0.5, rad=0.02)       # one radius, bg zeros
        assert tuple(half.shape) == (50, 75, 1)
        for bad in (torch.ones(n, 9), torch.ones(n, 0), torch.ones(n), torch.ones(n + 1, 3), torch.ones(2, n, 3)):
            with pytest.raises(ValueError, match="features must be"):
                r.render_channels(inputs, data, bad.cuda(), rad=rad)
        with pytest.raises(ValueError, match="bg must have"):
            r.render_channels(inputs, data, feat, rad=rad, bg=(0.0, 0.0, 0.0))
        with pytest.raises(ValueError, match="rad must be"):
            r.render_channels(inputs, data, feat, rad=torch.ones(n + 1))
    with pytest.raises(RuntimeError, match="forward only"):
        plain.render_channels(inputs, data, feat.clone().requires_grad_(True), rad=rad)
    in_graph = diff.render_channels(inputs, data, feat.clone().requires_grad_(True), rad=rad, bg=cc.bg(6))
    assert in_graph.requires_grad and torch.equal(in_graph.detach(), img)
    with pytest.raises(RuntimeError, match="bg is a constant"):
        diff.render_channels(inputs, data, feat.clone().requires_grad_(True), rad=rad, bg=torch.zeros(6, requires_grad=True))
    ctx = RenderContext(s["H"], s["W"])
    p = render_params(inputs["K"], s["H"], s["W"], 1.0, 2e-4)
    with pytest.raises(RuntimeError, match="forward only"):
        render_channels(ctx, p, P, feat.clone().requires_grad_(True))


def test_render_points_still_renders_the_first_three_columns():
    import torch
    from super_amd.renderer import RenderContext, render_params, render_points
    s = rc.facts("mixed")["scene"]
    P, feat, rad, inputs = _inputs(s, 6)
    p = render_params(inputs["K"], s["H"], s["W"], 1.0, 2e-4, (0.1, 0.2, 0.3))
    wide = render_points(RenderContext(s["H"], s["W"]), p, P, feat, radii=rad)                       # in place, stride 6
    wide64 = render_points(RenderContext(s["H"], s["W"]), p, P, feat.double(), radii=rad)            # converted: cut to [:, :3]
    three = render_points(RenderContext(s["H"], s["W"]), p, P, feat[:, :3].contiguous(), radii=rad)
    assert tuple(wide.shape) == (100, 150, 3) and torch.equal(wide, three) and torch.equal(wide64, three)
    assert float((three != torch.tensor([0.1, 0.2, 0.3], device="cuda")).float().mean()) > 0.05


@pytest.mark.parametrize("surfel_radii", [False, True])
def test_render_img_in_one_pass_is_the_two_renders(surfel_radii):
    import torch
    from super_amd import synth
    from super_amd.renderer import render_img
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    rng = np.random.default_rng(12)
    stable = rng.uniform(size=sc.N) > 0.03
    cols = rng.uniform(size=(sc.N, 3))
    confs = rng.uniform(0.0, 1.0, sc.N)
    radii = rc.formula_radii(sc.sf_points, sc.sf_norms, sc.K[0, 0])

    def surfels(**opt):
        return SimpleNamespace(points=torch.from_numpy(sc.sf_points).cuda(), colors=torch.from_numpy(cols).cuda(),
                               radii=torch.from_numpy(radii).cuda(), confs=torch.from_numpy(confs).cuda(),
                               isStable=torch.from_numpy(stable).cuda(),
                               opt=SimpleNamespace(height=sc.H, width=sc.W, renderer_rad=0.01,
                                                   renderer_surfel_radii=surfel_radii, renderer_radii_scale=1.5, **opt))

    inputs = {"K": torch.from_numpy(sc.K).float()[None].cuda()}
    two, one, off = surfels(), surfels(renderer_one_pass=True), surfels(renderer_one_pass=False)
    for sf in (two, one, off):
        render_img(sf, inputs)
    for sf in (one, off):
        assert tuple(sf.renderImg.shape) == (1, 3, sc.H, sc.W) and sf.renderImg.stride() == two.renderImg.stride()
        assert torch.equal(sf.renderImg, two.renderImg)
        assert torch.equal(sf.renderImg_conf_heat, two.renderImg_conf_heat)
    assert float((two.renderImg.sum(1) > 0).float().mean()) > 0.3             # both images are filled ...
    assert not torch.equal(two.renderImg, two.renderImg_conf_heat)           # ... and differ
