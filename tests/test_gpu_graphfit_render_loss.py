"""GraphFit with the render loss (opt.render_loss, super/deform_mesh.py:113-123; opt-in: GraphFit(opt,
native_render_loss=True)).  Compared with the oracle's geometric terms (oracle.graphfit_oracle) plus the CPU
restatement of the render loss (tests/render_grad_model.py) under autograd, and with CPU loops built like
test_gpu_graphfit_renderimg._cpu_loop.  Needs an MI355X (-m gpu).

The CPU side feeds the float32-rounded model image to the SSIM loss, as the HIP side feeds its float32 render (the
gradient passes the rounding).  Tolerances: 1e-9 relative on the loss terms, 1e-8 of the largest entry on the
gradient; 1e-6 of the update's size after ten iterations."""
from types import SimpleNamespace

import numpy as np
import pytest

import render_grad_model as rgm
import render_model as rm
from helpers import GF_CORR_VARIANTS, torch_frame
from oracle import graphfit_oracle as gfo

pytestmark = pytest.mark.gpu

RAD = 0.01          # a filled render of the 60x80 scene
WEIGHT = 0.01       # the term's gradient comparable with the geometric terms' at this scene


def _flow_of(img):
    import torch
    import torch.nn.functional as F
    m = img.float().mean(1, keepdim=True)
    b = F.avg_pool2d(m, 5, stride=1, padding=2)
    return torch.cat([2.0 * b, -1.5 * b], 1)


def _scene():
    from super_amd import synth
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    rng = np.random.default_rng(12)
    stable = rng.uniform(size=sc.N) > 0.1
    cols = rng.uniform(size=(sc.N, 3)).astype(np.float32)
    # the colour frame: the model moved by a few pixels, plus noise (close enough for the m < 0.1 selection)
    tg = rm.render(sc.sf_points[stable] + np.array([0.004, -0.002, 0.0]), cols[stable], sc.K, sc.H, sc.W, RAD)["img"]
    tgt = (np.transpose(tg, (2, 0, 1)) + 0.01 * np.random.default_rng(5).normal(size=(3, sc.H, sc.W))).astype(np.float32)
    return sc, stable, cols, tgt


def _opt(tag=None, **kw):
    o = gfo.default_opt(**(GF_CORR_VARIANTS[tag] if tag else {}))
    o.deform_udpate_method = "super_edg"
    o.renderer = "pulsar"
    o.renderer_rad = RAD
    o.render_loss = True
    o.render_loss_weight = WEIGHT
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _gpu_frame(sc, stable, cols, tgt):
    import torch
    sf, inputs, new_data = torch_frame(sc)
    sf.isStable = torch.from_numpy(stable).cuda()
    sf.colors = torch.from_numpy(cols).double().cuda()
    sf.rgb = torch.full((1, 3, sc.H, sc.W), 0.5, device="cuda")
    inputs[("color", 0)] = torch.from_numpy(tgt)[None].cuda()
    calls = []

    def optical_flow(a, b):
        calls.append((a, b))
        return [torch.zeros(1, 2, sc.H, sc.W, device="cuda"), _flow_of(a)]

    return sf, inputs, new_data, SimpleNamespace(optical_flow=optical_flow, calls=calls)


def _render_loss(sc, stable, cols, tgt, P, weight, rad=RAD, hit_sets=rgm.hit_sets):
    import torch
    hits = hit_sets(P.detach().numpy(), sc.K, sc.H, sc.W, rad)
    img = rgm.blend(P, cols[stable], hits, sc.K, sc.H, sc.W, rad)        # rgm.render, with the hit sets' form chosen
    img32 = img + (img.detach().float().double() - img.detach())
    loss, kept, _, _ = rgm.ssim_loss(img32, torch.from_numpy(tgt).double(), weight)
    return loss, kept, img.detach()


def _cpu_loop(sc, stable, cols, tgt, opt, match_render):
    import torch
    pb = gfo.Problem(sc, stable=stable)
    if getattr(opt, "sf_corr", False) and not match_render:
        pb.flow = _flow_of(torch.full((1, 3, sc.H, sc.W), 0.5))
    dv = torch.zeros((pb.J + 1, 7), dtype=torch.float64)
    dv[:, 0] = 1.0
    dv.requires_grad_(True)
    optim = (torch.optim.SGD([dv], lr=opt.learning_rate, momentum=0.9) if opt.optimizer == "SGD"
             else torch.optim.Adam([dv], lr=opt.learning_rate))
    for _ in range(opt.num_optimize_iterations):
        optim.zero_grad()
        _, P = gfo.deform(pb, dv)
        lr, _, img = _render_loss(sc, stable, cols, tgt, P, opt.render_loss_weight)
        if match_render:
            pb.flow = _flow_of(img.float().permute(2, 0, 1)[None])
        loss, _ = gfo.total_loss(pb, dv, opt)
        (loss + lr).backward()
        dv.grad[-1] = dv.grad[-1] / pb.J
        optim.step()
    return dv.detach().numpy()


@pytest.mark.parametrize("perturbed", [False, True])
def test_loss_and_grad_match_the_oracle(perturbed):
    import torch
    from super_amd.deform_mesh import GraphFit
    sc, stable, cols, tgt = _scene()
    opt = _opt()
    dv = np.zeros((49, 7))
    dv[:, 0] = 1.0
    if perturbed:
        rng = np.random.default_rng(9)
        dv[:, :4] += 0.002 * rng.normal(size=(49, 4))
        dv[:, 4:] += 0.0005 * rng.normal(size=(49, 3))
    sf, inputs, new_data, _ = _gpu_frame(sc, stable, cols, tgt)
    gf = GraphFit(opt, native_render_loss=True)
    d, matched, grad = gf.loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv).cuda())
    pb = gfo.Problem(sc, stable=stable)
    dvt = torch.from_numpy(dv).requires_grad_(True)
    loss, terms = gfo.total_loss(pb, dvt, opt)
    _, P = gfo.deform(pb, dvt)
    lr, kept, _ = _render_loss(sc, stable, cols, tgt, P, WEIGHT)
    (loss + lr).backward()
    want = dvt.grad.numpy().copy()
    want[-1] /= pb.J
    assert kept == gf.last_render_kept > 50
    for k in ("arap_loss", "rot_loss", "point_plane_loss"):
        t = float(terms[k].detach())
        assert abs(d[k] - t) <= 1e-9 * abs(t), k
    t = float(lr.detach())
    assert abs(d["render_loss"] - t) <= 1e-9 * abs(t)
    assert matched == int(terms["_matched"])
    got = grad.cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())
    # the term is in the gradient: without it the gradient differs well beyond the tolerance
    plain = GraphFit(_opt(render_loss=False))
    _, _, g0 = plain.loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv).cuda())
    assert np.abs(g0.cpu().numpy() - got).max() > 1e-3 * np.abs(want).max()


@pytest.mark.parametrize("tag,optimizer", [(None, "SGD"), (None, "Adam"), ("corr", "SGD")])
def test_ten_iterations_match_the_cpu_loop(tag, optimizer):
    from super_amd.deform_mesh import GraphFit
    sc, stable, cols, tgt = _scene()
    match = tag is not None
    opt = _opt(tag, optimizer=optimizer, sf_corr_match_renderimg=match)
    sf, inputs, new_data, models = _gpu_frame(sc, stable, cols, tgt)
    dv = GraphFit(opt, native_render_loss=True)(inputs, sf, new_data, models).cpu().numpy()
    if match:   # one render per iteration feeds the flow network and the loss
        assert len(models.calls) == 10
        for a, b in models.calls:
            assert tuple(a.shape) == (1, 3, sc.H, sc.W) and a.is_cuda and b is inputs[("color", 0)]
    else:
        assert len(models.calls) == 0
    ref = _cpu_loop(sc, stable, cols, tgt, opt, match)
    step = np.abs(ref - np.eye(1, 7)).max()
    assert step > 1e-7
    np.testing.assert_allclose(dv, ref, rtol=0, atol=1e-6 * step)
    # without the term the result differs
    sf2, inputs2, new_data2, models2 = _gpu_frame(sc, stable, cols, tgt)
    dv2 = GraphFit(_opt(tag, optimizer=optimizer, sf_corr_match_renderimg=match, render_loss=False))(
        inputs2, sf2, new_data2, models2).cpu().numpy()
    assert np.abs(dv2 - dv).max() > 1e-3 * step


def test_opt_in_is_required_and_sharded_frames_are_refused():
    from super_amd.deform_mesh import GraphFit
    with pytest.raises(NotImplementedError, match="native_render_loss"):
        GraphFit(_opt())
    with pytest.raises(NotImplementedError, match="sharded"):
        GraphFit(_opt(), native_render_loss=True, shard_surfels=True)
    with pytest.raises(NotImplementedError, match="pulsar"):
        GraphFit(_opt(renderer=None), native_render_loss=True)
