"""GraphFit with ``opt.sf_corr_match_renderimg`` (super/deform_mesh.py:292-305): every iteration renders the current
deformed stable surfels (slm_gf_render), re-infers the flow from that render and steps.  Compared with a CPU loop
built from oracle.graphfit_oracle (autograd + torch.optim, ``Problem.flow`` set per iteration), the CPU render model
(tests/render_model.py) and the same stand-in flow network.  Needs an MI355X (-m gpu).

The stand-in flow network is a smooth function of the image it gets: a 5x5 box blur of the channel mean, scaled
per flow channel.  Tolerance on the final deform_verts: 1e-6 of the update's size (max |dv - identity|).  Renders
agree to float64 rounding (test_gpu_render.py); the blur runs on the GPU on one side and on the CPU on the other,
so the flows agree to float32 rounding (1e-7 relative), which enters the correspondence residuals linearly --
the other terms agree to 1e-9 like tests/test_gpu_graphfit_corr.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import render_model as rm
from helpers import GF_CORR_VARIANTS, torch_frame
from oracle import graphfit_oracle as gfo

pytestmark = pytest.mark.gpu

RAD = 0.01          # about 1.2 px at this scene's focal length (110) and depth (~1): a filled render


def _flow_of(img):
    import torch.nn.functional as F
    import torch
    m = img.float().mean(1, keepdim=True)
    b = F.avg_pool2d(m, 5, stride=1, padding=2)
    return torch.cat([2.0 * b, -1.5 * b], 1)


def _scene():
    from super_amd import synth
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    rng = np.random.default_rng(12)
    stable = rng.uniform(size=sc.N) > 0.1
    cols = rng.uniform(size=(sc.N, 3)).astype(np.float32)
    return sc, stable, cols


def _opt(tag, **kw):
    o = gfo.default_opt(**GF_CORR_VARIANTS[tag])
    o.deform_udpate_method = "super_edg"
    o.sf_corr_match_renderimg = True
    o.renderer = "pulsar"
    o.renderer_rad = RAD
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _gpu_frame(sc, stable, cols):
    import torch
    sf, inputs, new_data = torch_frame(sc)
    sf.isStable = torch.from_numpy(stable).cuda()
    sf.colors = torch.from_numpy(cols).double().cuda()
    sf.rgb = torch.full((1, 3, sc.H, sc.W), 0.5, device="cuda")
    calls = []

    def optical_flow(a, b):
        calls.append((a, b))
        return [torch.zeros(1, 2, sc.H, sc.W, device="cuda"), _flow_of(a)]   # list: last wins

    return sf, inputs, new_data, SimpleNamespace(optical_flow=optical_flow, calls=calls)


def _cpu_loop(sc, stable, cols, opt):
    import torch
    pb = gfo.Problem(sc, stable=stable)
    dv = torch.zeros((pb.J + 1, 7), dtype=torch.float64)
    dv[:, 0] = 1.0
    dv.requires_grad_(True)
    optim = (torch.optim.SGD([dv], lr=opt.learning_rate, momentum=0.9) if opt.optimizer == "SGD"
             else torch.optim.Adam([dv], lr=opt.learning_rate))
    for _ in range(opt.num_optimize_iterations):
        optim.zero_grad()
        _, P = gfo.deform(pb, dv.detach())
        img = rm.render(P.numpy(), cols[stable], sc.K, sc.H, sc.W, RAD)["img"]
        pb.flow = _flow_of(torch.from_numpy(img).permute(2, 0, 1)[None])
        loss, _ = gfo.total_loss(pb, dv, opt)
        loss.backward()
        dv.grad[-1] = dv.grad[-1] / pb.J
        optim.step()
    return dv.detach().numpy()


@pytest.mark.parametrize("tag", ["corr", "corradam", "corrpp"])
def test_ten_iterations_match_the_cpu_loop(tag):
    from super_amd.deform_mesh import GraphFit
    sc, stable, cols = _scene()
    opt = _opt(tag)
    sf, inputs, new_data, models = _gpu_frame(sc, stable, cols)
    dv = GraphFit(opt)(inputs, sf, new_data, models).cpu().numpy()
    assert len(models.calls) == 10
    for a, b in models.calls:
        assert tuple(a.shape) == (1, 3, sc.H, sc.W) and a.is_cuda and b is inputs[("color", 0)]
    ref = _cpu_loop(sc, stable, cols, opt)
    step = np.abs(ref - np.eye(1, 7)).max()
    assert step > 1e-7
    np.testing.assert_allclose(dv, ref, rtol=0, atol=1e-6 * step)
    # the flow follows the render: without re-inference (flow of src.rgb) the result differs
    plain = _opt(tag, sf_corr_match_renderimg=False)
    sf2, inputs2, new_data2, models2 = _gpu_frame(sc, stable, cols)
    dv2 = GraphFit(plain)(inputs2, sf2, new_data2, models2).cpu().numpy()
    assert np.abs(dv2 - dv).max() > 1e-3 * step


def test_render_of_the_deformed_model_at_identity():
    import torch
    from super_amd.deform_mesh import GraphFit
    sc, stable, cols = _scene()
    sf, inputs, new_data, models = _gpu_frame(sc, stable, cols)
    gf = GraphFit(_opt("corr"))
    gf._bind(0, inputs, sf, new_data, models, defer_flow=True)
    img = gf.render_deformed(inputs, torch.from_numpy(cols).cuda())
    assert tuple(img.shape) == (1, 3, sc.H, sc.W)
    want = rm.render(sc.sf_points[stable], cols[stable], sc.K, sc.H, sc.W, RAD)
    ok = ~want["near"]
    got = img[0].permute(1, 2, 0).cpu().numpy()
    np.testing.assert_allclose(got[ok], want["img"][ok], rtol=0, atol=1e-5)
    assert (want["count"] > 0).mean() > 0.5


def test_render_loss_still_raises():
    from super_amd.deform_mesh import GraphFit
    with pytest.raises(NotImplementedError, match="render_loss"):
        GraphFit(_opt("corr", render_loss=True))
    with pytest.raises(NotImplementedError, match="pulsar"):
        GraphFit(_opt("corr", renderer=None))


def test_without_the_flag_the_net_sees_src_rgb_once():
    from super_amd.deform_mesh import GraphFit
    sc, stable, cols = _scene()
    sf, inputs, new_data, models = _gpu_frame(sc, stable, cols)
    GraphFit(_opt("corr", sf_corr_match_renderimg=False))(inputs, sf, new_data, models)
    assert len(models.calls) == 1
    assert models.calls[0][0] is sf.rgb and models.calls[0][1] is inputs[("color", 0)]
