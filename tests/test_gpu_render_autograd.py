"""The renderer's colour gradient (slm_render_backward_ex) and its autograd node (renderer.render_differentiable,
Pulsar(opt, differentiable=True)) against the CPU restatement of tests/render_color_grad_model.py.  Needs an MI355X.

Scenes and tolerances as test_gpu_render_grad.py: 1e-9 of the largest entry, points that are a candidate of a pixel the
forward model marks `near` left out.  The ABI outputs are bitwise reproducible, so the autograd gradients are compared
with them bitwise.  grad_image is float32-representable (the image is float32, so autograd hands the kernel g cast)."""
from types import SimpleNamespace

import numpy as np
import pytest

import render_color_grad_model as rcm
import render_grad_model as rgm
import render_model as rm
from test_gpu_render_grad import K0, RAD, _excluded, _scene

pytestmark = pytest.mark.gpu


def _g(h, w, seed=0):
    return np.random.default_rng(seed).normal(size=(h, w, 3)).astype(np.float32).astype(np.float64)


def _hip_ex(P, cols, K, H, W, rad, g, n_track=rm.N_TRACK, bg=(0.0, 0.0, 0.0), points=True, colors=True):
    import torch
    from super_amd.renderer import RenderContext, render_backward_ex, render_params, render_points
    ctx = RenderContext(H, W)
    p = render_params(torch.as_tensor(K)[None], H, W, 1.0, rad, bg)
    p.n_track = n_track
    render_points(ctx, p, torch.as_tensor(P).cuda(), torch.as_tensor(cols).cuda())
    gp, gc = render_backward_ex(ctx, p, torch.as_tensor(g).cuda(), points, colors)
    return ctx, p, gp, gc


def _excluded_vs(P, K, H, W, rad, near, view_scale):
    """_excluded at a view scale (H, W are the scaled image's size there)"""
    if view_scale == 1.0:
        return _excluded(P, K, H, W, rad, near)
    Ks = np.array(K, np.float64)
    Ks[:2] *= view_scale
    w, h, f, ccx, ccy = rm.camera(K, H, W, view_scale)
    assert rm.camera(Ks, h, w)[2:] == (f, ccx, ccy)
    return _excluded(P, Ks, h, w, rad, near)


def _compare_cols(P, cols, K, H, W, rad, n_track=rm.N_TRACK, bg=(0.0, 0.0, 0.0), seed=0):
    w, h = rm.camera(K, H, W)[:2]
    g = _g(h, w, seed)
    _, _, gp, gc = _hip_ex(P, cols, K, H, W, rad, g, n_track, bg)
    want_p, want_c = rcm.grads(P, np.asarray(cols, np.float64), g, K, H, W, rad, bg=bg, n_track=n_track)
    near = rm.render(P, cols, K, H, W, rad, bg=bg, n_track=n_track)["near"]
    ex = _excluded(P, K, H, W, rad, near)
    assert ex.mean() < 0.05, ex.mean()
    for got, want in ((gc, want_c), (gp, want_p)):
        scale = np.abs(want).max()
        assert scale > 0
        np.testing.assert_allclose(got.cpu().numpy()[~ex], want[~ex], rtol=0, atol=1e-9 * scale)
    return gp, gc


# ---- 1. the colour gradient against the model ---------------------------------------------------------------------

@pytest.mark.parametrize("n_track", [rm.N_TRACK, 2])
def test_colour_gradient_matches_the_model(n_track):
    sc, cols = _scene()
    _, gc = _compare_cols(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, n_track, bg=(0.1, 0.2, 0.3))
    assert (np.abs(gc.cpu().numpy()).max(1) > 0).mean() > 0.5      # most points reach a pixel


def test_colour_gradient_on_the_overflow_path():
    """6000 surfels in one 16x16 tile: more keys than the 4096 the LDS sort holds"""
    rng = np.random.default_rng(4)
    n = 6000
    Z = rng.uniform(0.5, 3.0, n)
    u, v = rng.uniform(17.5, 30.5, n), rng.uniform(17.5, 30.5, n)
    P = np.stack([(u - 32.0) * Z / 100.0, (v - 24.0) * Z / 100.0, Z], 1)
    cols = rng.uniform(size=(n, 3)).astype(np.float32)
    _compare_cols(P, cols, K0, 48, 64, 1.0 * Z.min() / 100.0)


def test_colour_gradient_of_no_points_and_all_culled():
    g = np.ones((48, 64, 3))
    _, _, gp, gc = _hip_ex(np.zeros((0, 3)), np.zeros((0, 3), np.float32), K0, 48, 64, 0.02, g)
    assert tuple(gp.shape) == tuple(gc.shape) == (0, 3)
    P = np.array([[0, 0, 0.005], [0, 0, 20.0], [0, 0, -1.0], [50.0, 0, 1.0]])
    for points in (True, False):
        _, _, gp, gc = _hip_ex(P, np.ones((4, 3), np.float32), K0, 48, 64, 0.02, g, points=points)
        assert tuple(gc.shape) == (4, 3) and (gc == 0).all()
        assert (gp is None) if not points else (gp == 0).all()


# ---- 2. both outputs, one output, reproducibility, refusals -------------------------------------------------------

def test_both_outputs_equal_the_single_calls_bitwise():
    import ctypes as C

    import torch
    from super_amd import _lib
    from super_amd.renderer import render_backward, render_backward_ex
    sc, cols = _scene()
    g = torch.from_numpy(_g(sc.H, sc.W, 1)).cuda()
    ctx, p, gp, gc = _hip_ex(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, g.cpu().numpy())
    assert torch.equal(gp, render_backward(ctx, p, g))
    none, gc_only = render_backward_ex(ctx, p, g, points=False)
    assert none is None and torch.equal(gc, gc_only)
    gp_only, none = render_backward_ex(ctx, p, g, colors=False)
    assert none is None and torch.equal(gp, gp_only)
    gp2, gc2 = render_backward_ex(ctx, p, g)
    assert torch.equal(gp, gp2) and torch.equal(gc, gc2)
    _, _, gp3, gc3 = _hip_ex(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, g.cpu().numpy())    # a fresh context
    assert torch.equal(gp, gp3) and torch.equal(gc, gc3)
    # the refusals of slm_render_backward
    lib = ctx.lib
    out = torch.empty((sc.N, 3), dtype=torch.float64, device="cuda")
    assert lib.slm_render_backward_ex(ctx.h, C.byref(p), g.data_ptr(), None, None, None) == _lib.SLM_ERR_INVALID
    q = _lib.SlmRenderParams.from_buffer_copy(p)
    q.radius = RAD * 1.5
    assert lib.slm_render_backward_ex(ctx.h, C.byref(q), g.data_ptr(), None, out.data_ptr(), None) == _lib.SLM_ERR_INVALID
    from super_amd.renderer import RenderContext
    fresh = RenderContext(sc.H, sc.W)
    assert lib.slm_render_backward_ex(fresh.h, C.byref(p), g.data_ptr(), out.data_ptr(), None, None) == _lib.SLM_ERR_INVALID
    torch.cuda.synchronize()


# ---- 3. Pulsar(opt, differentiable=True) under autograd -----------------------------------------------------------

def _pulsar(H, W, differentiable=True):
    from super_amd.renderer import Pulsar
    return Pulsar(SimpleNamespace(height=H, width=W), differentiable=differentiable)


def _inputs(K):
    import torch
    return {"K": torch.from_numpy(np.asarray(K, np.float64))[None].cuda()}


CASES = [   # (points grad, colours grad, points dtype, colours form, view_scale)
    (True, False, "f64", "f32", 1.0),
    (False, True, "f64", "f32", 1.0),
    (True, True, "f32", "f32", 1.0),
    (True, True, "f64", "f64", 1.0),
    (True, True, "f64", "wide", 1.0),
    (True, True, "f32", "f64", 0.5),
]


@pytest.mark.parametrize("want_p,want_c,pdt,cform,view_scale", CASES)
def test_pulsar_autograd_matches_the_abi_and_the_model(want_p, want_c, pdt, cform, view_scale):
    import torch
    from super_amd.renderer import RenderContext, render_backward_ex, render_params, render_points
    sc, cols = _scene()
    P = torch.from_numpy(sc.sf_points).cuda()
    P = P.float() if pdt == "f32" else P
    C64 = torch.from_numpy(cols.astype(np.float64)).cuda()
    if cform == "f32":
        Cin = C64.float()
    elif cform == "f64":
        Cin = C64.clone()
    else:
        Cin = torch.cat([C64.float(), torch.full((sc.N, 1), 7.0, device="cuda")], 1)[:, :3]
        assert Cin.stride() == (4, 1)
    leafP, leafC = P.clone().requires_grad_(want_p), Cin.detach().clone() if cform != "wide" else None
    if cform == "wide":
        wide = torch.cat([C64.float(), torch.full((sc.N, 1), 7.0, device="cuda")], 1).requires_grad_(want_c)
        cin = wide[:, :3]
    else:
        leafC.requires_grad_(want_c)
        cin = leafC
    r = _pulsar(sc.H, sc.W)
    inputs = _inputs(sc.K)
    img = r(inputs, SimpleNamespace(points=leafP, colors=cin), rad=RAD, view_scale=view_scale)
    assert img.requires_grad and img.dtype == torch.float32
    h, w = img.shape[:2]
    g = _g(h, w, 3)
    (img.double() * torch.from_numpy(g).cuda()).sum().backward()
    # the ABI on a fresh context
    ctx = RenderContext(h, w)
    p = render_params(inputs["K"], sc.H, sc.W, view_scale, RAD)
    ref = render_points(ctx, p, P, Cin)
    assert torch.equal(ref, img.detach())
    gp, gc = render_backward_ex(ctx, p, torch.from_numpy(g).cuda())
    if want_p:
        assert leafP.grad.dtype == P.dtype and leafP.grad.shape == P.shape
        assert torch.equal(leafP.grad, gp.to(P.dtype))
    else:
        assert leafP.grad is None
    if want_c:
        if cform == "wide":
            cg = wide.grad
            assert cg.shape == (sc.N, 4) and cg.dtype == torch.float32 and (cg[:, 3] == 0).all()
            cg = cg[:, :3]
        else:
            cg = leafC.grad
            assert cg.dtype == Cin.dtype and cg.shape == Cin.shape
        assert torch.equal(cg, gc.to(cg.dtype))
    else:
        assert (leafC if cform != "wide" else wide).grad is None
    # the model (float64 outputs only: a float32 gradient is the float64 one rounded)
    want_p_m, want_c_m = rcm.grads(sc.sf_points, cols.astype(np.float64), g, sc.K, sc.H, sc.W, RAD, view_scale)
    near = rm.render(sc.sf_points, cols, sc.K, sc.H, sc.W, RAD, view_scale)["near"]
    ex = _excluded_vs(sc.sf_points, sc.K, sc.H, sc.W, RAD, near, view_scale)
    assert ex.mean() < 0.05
    for got, want in ((gp, want_p_m), (gc, want_c_m)):
        np.testing.assert_allclose(got.cpu().numpy()[~ex], want[~ex], rtol=0, atol=1e-9 * np.abs(want).max())


def test_pulsar_without_grad_inputs_takes_the_plain_forward():
    import torch
    sc, cols = _scene()
    inputs = _inputs(sc.K)
    data = SimpleNamespace(points=torch.from_numpy(sc.sf_points).cuda(), colors=torch.from_numpy(cols).cuda())
    a = _pulsar(sc.H, sc.W)(inputs, data, rad=RAD)
    b = _pulsar(sc.H, sc.W, differentiable=False)(inputs, data, rad=RAD)
    assert not a.requires_grad and torch.equal(a, b)
    leaf = data.points.clone().requires_grad_(True)
    with torch.no_grad():
        c = _pulsar(sc.H, sc.W)(inputs, SimpleNamespace(points=leaf, colors=data.colors), rad=RAD)
    assert not c.requires_grad and torch.equal(a, c)


# ---- 4. a shared context ------------------------------------------------------------------------------------------

def _alone(sc, cols, g, view_scale=1.0):
    """A's gradients from a Pulsar that renders nothing else"""
    import torch
    PA = torch.from_numpy(sc.sf_points).cuda().requires_grad_(True)
    CA = torch.from_numpy(cols).cuda().requires_grad_(True)
    img = _pulsar(sc.H, sc.W)(_inputs(sc.K), SimpleNamespace(points=PA, colors=CA), rad=RAD, view_scale=view_scale)
    (img.double() * g).sum().backward()
    return img.detach(), PA.grad, CA.grad


@pytest.mark.parametrize("other", ["render", "render_img", "more_points", "larger_view_scale"])
def test_backward_after_another_render_on_the_context(other):
    import torch
    from super_amd.renderer import render_img
    sc, cols = _scene()
    vs = 0.5 if other == "larger_view_scale" else 1.0
    g = torch.from_numpy(_g(int(sc.H * vs), int(sc.W * vs), 4)).cuda()
    want_img, want_p, want_c = _alone(sc, cols, g, vs)
    r = _pulsar(sc.H, sc.W)
    inputs = _inputs(sc.K)
    PA = torch.from_numpy(sc.sf_points).cuda().requires_grad_(True)
    CA = torch.from_numpy(cols).cuda().requires_grad_(True)
    imgA = r(inputs, SimpleNamespace(points=PA, colors=CA), rad=RAD, view_scale=vs)
    ctxA, capA = r._ctx, r._ctx.cap
    rng = np.random.default_rng(6)
    PB = torch.from_numpy(sc.sf_points + 0.003 * rng.normal(size=sc.sf_points.shape)).cuda()
    CB = torch.from_numpy(rng.uniform(size=(sc.N, 3)).astype(np.float32)).cuda()
    if other == "render":
        imgB = r(inputs, SimpleNamespace(points=PB.requires_grad_(True), colors=CB), rad=RAD)
        assert imgB.requires_grad
    elif other == "render_img":
        n = sc.N
        sf = SimpleNamespace(points=PB, colors=CB.double(), confs=torch.rand(n, device="cuda", dtype=torch.float64),
                             isStable=torch.ones(n, dtype=torch.bool, device="cuda"),
                             opt=SimpleNamespace(height=sc.H, width=sc.W, renderer_rad=RAD),
                             models=SimpleNamespace(renderer=r))
        render_img(sf, inputs)
        assert r._ctx is ctxA
    elif other == "more_points":
        big = torch.cat([PB, PB + 0.001], 0)
        r(inputs, SimpleNamespace(points=big, colors=torch.cat([CB, CB], 0)), rad=RAD)
        assert r._ctx is ctxA and ctxA.cap > capA          # reserve recreated the handle
    else:
        r(inputs, SimpleNamespace(points=PB, colors=CB), rad=RAD, view_scale=1.0)
        assert r._ctx is not ctxA                          # Pulsar.context replaced the context
    assert ctxA.serial > 1 or r._ctx is not ctxA
    (imgA.double() * g).sum().backward()
    assert torch.equal(imgA.detach(), want_img)
    assert torch.equal(PA.grad, want_p) and torch.equal(CA.grad, want_c)


def test_in_place_change_after_the_forward_is_caught_and_bg_col_is_refused():
    import torch
    sc, cols = _scene()
    r = _pulsar(sc.H, sc.W)
    inputs = _inputs(sc.K)
    PA = torch.from_numpy(sc.sf_points).cuda().requires_grad_(True)
    img = r(inputs, SimpleNamespace(points=PA, colors=torch.from_numpy(cols).cuda()), rad=RAD)
    with torch.no_grad():
        PA.add_(0.001)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        img.sum().backward()
    bg = torch.tensor([0.1, 0.2, 0.3], requires_grad=True)
    with pytest.raises(RuntimeError, match="bg_col"):
        r(inputs, SimpleNamespace(points=PA, colors=torch.from_numpy(cols).cuda()), rad=RAD, bg_col=bg)
    with pytest.raises(RuntimeError, match="forward only"):            # plain Pulsar keeps refusing
        _pulsar(sc.H, sc.W, differentiable=False)(inputs, SimpleNamespace(points=PA, colors=torch.from_numpy(cols).cuda()),
                                                  rad=RAD)


# ---- 5. the reference's GraphFit loop with only the renderer swapped ----------------------------------------------

def _pulsar_loop(sc, stable, cols, tgt, opt, match_render, inputs):
    """test_gpu_graphfit_render_loss._cpu_loop with the model render replaced by Pulsar(opt, differentiable=True): the
    reference's deform_superedg, which renders new_data every iteration (`if True:`, deform_mesh.py:294-298)."""
    import torch
    from oracle import graphfit_oracle as gfo
    from test_gpu_graphfit_render_loss import _flow_of
    pb = gfo.Problem(sc, stable=stable)
    if getattr(opt, "sf_corr", False) and not match_render:
        pb.flow = _flow_of(torch.full((1, 3, sc.H, sc.W), 0.5))
    r = _pulsar(sc.H, sc.W)
    colors = torch.from_numpy(cols[stable]).cuda()
    tgt64 = torch.from_numpy(tgt).double()
    dv = torch.zeros((pb.J + 1, 7), dtype=torch.float64)
    dv[:, 0] = 1.0
    dv.requires_grad_(True)
    optim = (torch.optim.SGD([dv], lr=opt.learning_rate, momentum=0.9) if opt.optimizer == "SGD"
             else torch.optim.Adam([dv], lr=opt.learning_rate))
    for _ in range(opt.num_optimize_iterations):
        optim.zero_grad()
        _, P = gfo.deform(pb, dv)
        img = r(inputs, SimpleNamespace(points=P.cuda(), colors=colors), rad=opt.renderer_rad)
        assert img.requires_grad
        if match_render:
            pb.flow = _flow_of(img.detach().cpu().permute(2, 0, 1)[None])
        loss, _ = gfo.total_loss(pb, dv, opt)
        if opt.render_loss:
            lr, _, _, _ = rgm.ssim_loss(img.cpu().double(), tgt64, opt.render_loss_weight)
            loss = loss + lr
        loss.backward()
        dv.grad[-1] = dv.grad[-1] / pb.J
        optim.step()
    return dv.detach().numpy()


@pytest.mark.parametrize("tag,optimizer", [(None, "SGD"), (None, "Adam"), ("corr", "SGD")])
def test_reference_loop_with_the_pulsar_swapped_in(tag, optimizer):
    from super_amd.deform_mesh import GraphFit
    from test_gpu_graphfit_render_loss import _cpu_loop, _gpu_frame, _opt
    from test_gpu_graphfit_render_loss import _scene as _gf_scene
    sc, stable, cols, tgt = _gf_scene()
    match = tag is not None
    opt = _opt(tag, optimizer=optimizer, sf_corr_match_renderimg=match)
    sf, inputs, new_data, models = _gpu_frame(sc, stable, cols, tgt)
    got = _pulsar_loop(sc, stable, cols, tgt, opt, match, inputs)
    native = GraphFit(opt, native_render_loss=True)(inputs, sf, new_data, models).cpu().numpy()
    ref = _cpu_loop(sc, stable, cols, tgt, opt, match)
    step = np.abs(ref - np.eye(1, 7)).max()
    assert step > 1e-7
    np.testing.assert_allclose(got, native, rtol=0, atol=1e-6 * step)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6 * step)


def test_reference_loop_without_the_render_loss_equals_the_oracle():
    from oracle import graphfit_oracle as gfo
    from test_gpu_graphfit_render_loss import _gpu_frame, _opt
    from test_gpu_graphfit_render_loss import _scene as _gf_scene
    sc, stable, cols, tgt = _gf_scene()
    opt = _opt(render_loss=False)
    _, inputs, _, _ = _gpu_frame(sc, stable, cols, tgt)
    got = _pulsar_loop(sc, stable, cols, tgt, opt, False, inputs)
    want = gfo.graphfit(gfo.Problem(sc, stable=stable), opt)
    assert np.abs(want - np.eye(1, 7)).max() > 1e-7
    np.testing.assert_array_equal(got, want)
