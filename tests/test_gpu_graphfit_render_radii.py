"""GraphFit with ``opt.renderer_surfel_radii``: the renders of the render loss give every surfel its own radius
(slm_gf_render_radii), here the reference's formula Z / (sqrt(2) f clamp(|n_z|, 0.26, 1)).  One ``loss_and_grad``
evaluation against the oracle's geometric terms plus the CPU restatement of the per-point render
(tests/render_radii_model.py) and the SSIM loss (tests/render_grad_model.py) under autograd, with the tolerances of
test_gpu_graphfit_render_loss.py; and slm_gf_render_radii itself with unstable rows.  Needs an MI355X."""
import numpy as np
import pytest

import render_grad_model as rgm
import render_radii_cases as rc
import render_radii_model as rrm
from helpers import torch_frame
from oracle import graphfit_oracle as gfo

pytestmark = pytest.mark.gpu


def _opt(**kw):
    o = gfo.default_opt()
    o.deform_udpate_method = "super_edg"
    o.renderer = "pulsar"
    o.renderer_rad = rc.GF_UNIFORM_RAD
    o.render_loss = True
    o.render_loss_weight = rc.GF_WEIGHT
    o.renderer_surfel_radii = True
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _gpu_frame(sc, stable, cols, radii, tgt):
    import torch
    sf, inputs, new_data = torch_frame(sc)
    sf.isStable = torch.from_numpy(stable).cuda()
    sf.colors = torch.from_numpy(cols).double().cuda()
    r = radii.copy()
    r[~stable] = 1.0                            # rows of unstable surfels are not read: a 1 m sphere would cover the image
    sf.radii = torch.from_numpy(r).cuda()
    sf.rgb = torch.full((1, 3, sc.H, sc.W), 0.5, device="cuda")
    inputs[("color", 0)] = torch.from_numpy(tgt)[None].cuda()
    return sf, inputs, new_data


@pytest.mark.parametrize("perturbed", [False, True])
def test_loss_and_grad_match_the_model(perturbed):
    import torch
    from super_amd.deform_mesh import GraphFit
    sc, stable, cols, radii, tgt = rc.graphfit_scene()
    opt = _opt()
    dv = np.zeros((49, 7))
    dv[:, 0] = 1.0
    if perturbed:
        rng = np.random.default_rng(9)
        dv[:, :4] += 0.002 * rng.normal(size=(49, 4))
        dv[:, 4:] += 0.0005 * rng.normal(size=(49, 3))
    sf, inputs, new_data = _gpu_frame(sc, stable, cols, radii, tgt)
    gf = GraphFit(opt, native_render_loss=True)
    d, matched, grad = gf.loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv).cuda())
    pb = gfo.Problem(sc, stable=stable)
    dvt = torch.from_numpy(dv).requires_grad_(True)
    loss, terms = gfo.total_loss(pb, dvt, opt)
    _, P = gfo.deform(pb, dvt)
    R = torch.from_numpy(radii[stable])
    hits = rrm.hit_sets(P.detach().numpy(), radii[stable], sc.K, sc.H, sc.W)
    img = rrm.blend(P, torch.from_numpy(cols[stable].astype(np.float64)), R, hits, sc.K, sc.H, sc.W)
    img32 = img + (img.detach().float().double() - img.detach())
    lr, kept, _, _ = rgm.ssim_loss(img32, torch.from_numpy(tgt).double(), rc.GF_WEIGHT)
    (loss + lr).backward()
    want = dvt.grad.numpy().copy()
    want[-1] /= pb.J
    print("kept", kept, gf.last_render_kept, "render_loss", d["render_loss"], float(lr.detach()))
    assert kept == gf.last_render_kept > 0
    for k in ("arap_loss", "rot_loss", "point_plane_loss"):
        t = float(terms[k].detach())
        assert abs(d[k] - t) <= 1e-9 * abs(t), k
    t = float(lr.detach())
    assert abs(d["render_loss"] - t) <= 1e-9 * abs(t)
    assert matched == int(terms["_matched"])
    got = grad.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())
    if not perturbed:
        # the one default radius keeps no pixel of this scene: no loss, and the gradient is the geometric terms' alone
        one = GraphFit(_opt(renderer_surfel_radii=False), native_render_loss=True)
        d1, _, g1 = one.loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv).cuda())
        assert one.last_render_kept == 0 and d1["render_loss"] == 0.0
        assert np.abs(g1.cpu().numpy() - got).max() > 1e-3 * np.abs(want).max()


def test_gf_render_radii_by_surfel_row_with_unstable_rows():
    import torch
    from super_amd.deform_mesh import GraphFit
    from super_amd.renderer import render_backward_ex
    sc, stable, cols, radii, tgt = rc.graphfit_scene()
    scale = 1.5
    sf, inputs, new_data = _gpu_frame(sc, stable, cols, radii, tgt)
    gf = GraphFit(_opt(render_loss=False, renderer_radii_scale=scale))
    gf._bind(0, inputs, sf, new_data, None)
    img, p = gf._render_deformed_hwc(inputs, torch.from_numpy(cols).cuda())
    P, R = sc.sf_points[stable], (radii * scale)[stable]
    want = rrm.render(P, cols[stable], R, sc.K, sc.H, sc.W)
    ok = ~want["near"]
    assert (~ok).sum() <= 0.005 * ok.size
    np.testing.assert_allclose(img.cpu().numpy()[ok], want["img"][ok], rtol=0, atol=1e-5)
    g = np.random.default_rng(2).normal(size=(sc.H, sc.W, 3))
    gp, gc, gr = (t.cpu().numpy() for t in render_backward_ex(gf._render_ctx, p, torch.from_numpy(g).cuda(), radii=True))
    assert gr.shape == (sc.N,)
    for t in (gp, gc, gr):
        assert (t[~stable] == 0).all()
    hits = rrm.hit_sets(P, R, sc.K, sc.H, sc.W)
    wp, wc, wr = rrm.grads(P, cols[stable], R, g, hits, sc.K, sc.H, sc.W)
    ex = rrm.excluded(P, R, sc.K, sc.H, sc.W, want["near"])
    assert ex.mean() <= rc.MAX_EXCLUDED
    for got, w in ((gp, wp), (gc, wc), (gr, wr)):
        np.testing.assert_allclose(got[stable][~ex], w[~ex], rtol=0, atol=1e-9 * np.abs(w).max())
