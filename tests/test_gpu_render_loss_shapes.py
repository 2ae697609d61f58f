"""The render-loss chain at the driver's size and at the shapes where tiled kernels go wrong: the SSIM-11 loss
(slm_render_ssim_loss) over a sweep of image sizes, the renderer backward (slm_render_backward / _ex) at 480x640 with
300 000 surfels and on hand-built geometry, and GraphFit(opt, native_render_loss=True) once at that size.  Against the
float64 models of tests/render_grad_model.py and tests/render_color_grad_model.py.  Needs an MI355X.

Inputs and the conditions on them (which SSIM branches they reach, how many pixels sit at a threshold) are those of
tests/render_loss_cases.py; test_render_loss_cases.py checks them without a GPU and the tests here repeat them on the
model's outputs before they compare, so an input that stops reaching a branch fails instead of passing vacuously.

Tolerances, all the project's own: SSIM loss 1e-12 relative, dL/dimage 1e-12 of the largest entry, kept count exact
(test_gpu_render_grad.test_ssim_loss_matches_the_model); backward, points and colours, 1e-9 of the largest entry
(test_gpu_render_grad._compare).  Full-size scenes leave out the points that are a candidate of a `near` pixel, at most
5 % of them; the model alone gives, for seed 5 (f32 and f64 centres round to the same float32, so they share a row):

    rad      view_scale   pixels covered   most hits   pixels near   points left out
    1e-3     1.0          98.6 %           7           0.091 %       0.73 %
    1.5e-3   1.0          99.2 %           10          0.23 %        2.8 %
    1e-3     0.5          98.5 %           6           0.089 %       0.31 %
    1.5e-3   0.5          98.9 %           9           0.21 %        1.2 %
    (2e-3    1.0: 7.3 % left out, over the cap; not used)

Hand-built scenes leave no point out; dL/dimage is zero on the `near` pixels instead (at most 1 % of the pixels): big
splats 0.62 %, overflow with neighbours 0.88 %, ties none."""

import numpy as np
import pytest

import render_grad_model as rgm
import render_loss_cases as rc
import render_model as rm
from test_gpu_render_autograd import _excluded_vs

pytestmark = pytest.mark.gpu


# ---- 1. the SSIM loss over a shape sweep ------------------------------------------------------------------------------

@pytest.mark.parametrize("h,w,holes", rc.SSIM_CASES)
def test_ssim_loss_over_shapes(h, w, holes):
    import torch
    from super_amd.renderer import ssim_render_loss
    img, tgt = rc.ssim_inputs(h, w, holes)
    mod = rc.ssim_model(img, tgt)
    b = rc.assert_ssim_branches(h, w, holes, img, mod)
    x, t = torch.from_numpy(img).cuda(), torch.from_numpy(tgt).cuda()
    loss, kept, grad = ssim_render_loss(x, t, rc.SSIM_WEIGHT)
    got, want = grad.cpu().numpy(), mod["grad"]
    scale = np.abs(want).max()
    print(f"ssim {h}x{w} holes={holes}: {b} loss {loss!r} want {mod['loss']!r} rel "
          f"{abs(loss - mod['loss']) / max(abs(mod['loss']), 1e-300):.2e} grad err / max "
          f"{np.abs(got - want).max() / max(scale, 1e-300):.2e}")
    assert kept == mod["kept"]
    assert abs(loss - mod["loss"]) <= 1e-12 * abs(mod["loss"])
    assert got.shape == (h, w, 3)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12 * scale)
    if mod["kept"]:
        assert scale > 0 and (np.abs(got).max(2) > 0).sum() > mod["kept"]       # the gradient spreads over the windows
    # bitwise reproducible; without the gradient the loss is the same
    loss2, kept2, grad2 = ssim_render_loss(x, t, rc.SSIM_WEIGHT)
    assert loss2 == loss and kept2 == kept and torch.equal(grad, grad2)
    loss3, kept3, none = ssim_render_loss(x, t[None], rc.SSIM_WEIGHT, with_grad=False)
    assert loss3 == loss and kept3 == kept and none is None


@pytest.mark.parametrize("h,w,holes", [(6, 6, False), (10, 17, True)])
def test_ssim_gradient_matches_finite_differences_of_the_model(h, w, holes):
    """where a pixel lies three times in a reflected window: the HIP gradient against central differences of the model's
    float64 loss (1e-6 of the largest entry, as test_render_grad_model.py), independent of autograd's reflection pad"""
    import torch
    from super_amd.renderer import ssim_render_loss
    img, tgt = rc.ssim_inputs(h, w, holes)
    _, _, grad = ssim_render_loss(torch.from_numpy(img).cuda(), torch.from_numpy(tgt).cuda(), rc.SSIM_WEIGHT)
    got = grad.cpu().numpy()
    x, t = img.astype(np.float64), tgt.astype(np.float64)
    scale = np.abs(rc.ssim_model(img, tgt)["grad"]).max()
    pts = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (h // 2, w - 1), (0, w // 2), (h // 2, w // 2), (h - 1, w // 2 + 1)]
    pts = [p for p in pts if x[p].min() > 0]
    assert len(pts) >= 6 and scale > 0
    step, checked = 1e-6, 0
    for i, j in pts:
        for c in range(3):
            a, b = x.copy(), x.copy()
            a[i, j, c] += step
            b[i, j, c] -= step
            fd = (rc.ssim_loss_only(a, t) - rc.ssim_loss_only(b, t)) / (2 * step)
            assert abs(fd - got[i, j, c]) <= 1e-6 * scale, (i, j, c, fd, got[i, j, c])
            checked += abs(fd) > 1e-3 * scale
    assert checked >= 6


def test_ssim_refuses_sizes_below_six_and_null_pointers():
    import torch
    from super_amd import _lib
    lib = _lib.load()
    x = torch.rand((16, 16, 3), device="cuda")
    t = torch.rand((3, 16, 16), device="cuda")
    out = torch.full((2,), -7.0, dtype=torch.float64, device="cuda")
    for h, w in ((5, 16), (16, 5), (5, 5)):         # the buffers hold 16 x 16: nothing is read either way
        rc_ = lib.slm_render_ssim_loss(h, w, x.data_ptr(), t.data_ptr(), 1.0, out.data_ptr(), None, None)
        assert rc_ == _lib.SLM_ERR_INVALID and b"slm_render_ssim_loss" in lib.slm_last_error()
    for a, b, o in ((None, t.data_ptr(), out.data_ptr()), (x.data_ptr(), None, out.data_ptr()), (x.data_ptr(), t.data_ptr(), None)):
        assert lib.slm_render_ssim_loss(16, 16, a, b, 1.0, o, None, None) == _lib.SLM_ERR_INVALID
        assert b"slm_render_ssim_loss" in lib.slm_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all()                       # a refused call writes nothing
    assert lib.slm_render_ssim_loss(6, 6, x.data_ptr(), t.data_ptr(), 1.0, out.data_ptr(), None, None) == 0
    torch.cuda.synchronize()


# ---- 2. the renderer backward -----------------------------------------------------------------------------------------

def _hip_both(P, cols, K, H, W, rad, g, view_scale=1.0, n_track=rm.N_TRACK, ctx=None):
    """render, then slm_render_backward_ex (both outputs) and slm_render_backward on the same forward"""
    import torch
    from super_amd.renderer import RenderContext, render_backward, render_backward_ex, render_params, render_points
    w, h = rm.camera(K, H, W, view_scale)[:2]
    ctx = ctx or RenderContext(h, w)
    p = render_params(torch.as_tensor(K)[None], H, W, view_scale, rad)
    p.n_track = n_track
    img = render_points(ctx, p, torch.as_tensor(P).cuda(), torch.as_tensor(cols).cuda())
    gd = torch.as_tensor(g).cuda()
    gp, gc = render_backward_ex(ctx, p, gd)
    assert torch.equal(render_backward(ctx, p, gd), gp)          # the point half, bitwise
    return img, gp, gc


def _assert_close(name, got, want, keep):
    scale = np.abs(want).max()
    assert scale > 0
    err = np.abs(got[keep] - want[keep]).max()
    print(f"  {name}: max err / max|want| = {err / scale:.2e} over {int(keep.sum())} of {len(keep)} points")
    np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=1e-9 * scale)


@pytest.fixture(scope="module")
def full():
    """the scene of test_gpu_render.py, and per (rad, view_scale) what the models say about it (cached: the f32 and the
    f64 centres round to the same float32, so they share hit sets, `near` pixels and gradients)"""
    from super_amd import synth
    sc = synth.make_scene(N=300_000, J=512, H=480, W=640, seed=5, src_border=2)
    cols = np.random.default_rng(2).uniform(size=(sc.N, 3)).astype(np.float32)
    P32 = sc.sf_points.astype(np.float32)
    # float64 centres that are not float32 numbers, and round to the same ones
    P64 = P32.astype(np.float64) * (1.0 + 1e-9 * np.random.default_rng(3).uniform(-1, 1, size=P32.shape))
    assert (P64.astype(np.float32) == P32).all() and (P64 != P32).mean() > 0.9
    cache = {}

    def model(rad, view_scale):
        if (rad, view_scale) not in cache:
            w, h = rm.camera(sc.K, sc.H, sc.W, view_scale)[:2]
            want = rm.render(P32, cols, sc.K, sc.H, sc.W, rad, view_scale)
            ex = _excluded_vs(P32, sc.K, sc.H, sc.W, rad, want["near"], view_scale)
            hits = rgm.hit_sets_fast(P32, sc.K, sc.H, sc.W, rad, view_scale)
            g = np.random.default_rng(0).normal(size=(h, w, 3)).astype(np.float32).astype(np.float64)
            gp, gc = rc.model_grads(P32, cols, g, hits, sc.K, sc.H, sc.W, rad, view_scale)
            cache[(rad, view_scale)] = dict(want=want, ex=ex, g=g, gp=gp, gc=gc)
        return cache[(rad, view_scale)]

    return dict(sc=sc, cols=cols, f32=P32, f64=P64, model=model)


FULL_CASES = [("f32", 1e-3, 1.0), ("f64", 1e-3, 1.0), ("f64", 1.5e-3, 1.0), ("f32", 1e-3, 0.5), ("f64", 1e-3, 0.5),
              ("f64", 1.5e-3, 0.5)]


@pytest.mark.parametrize("dtype,rad,view_scale", FULL_CASES)
def test_backward_at_full_size(full, dtype, rad, view_scale):
    sc, cols, P = full["sc"], full["cols"], full[dtype]
    m = full["model"](rad, view_scale)
    ex, want = m["ex"], m["want"]
    print(f"full size {dtype} rad {rad} view_scale {view_scale}: covered {(want['count'] > 0).mean():.4f} most hits "
          f"{want['count'].max()} near {want['near'].mean():.5f} left out {ex.mean():.4f}")
    assert ex.mean() < 0.05, ex.mean()
    assert (want["count"] > 0).mean() > 0.9 and want["count"].max() > 4          # a filled image, real blends
    img, gp, gc = _hip_both(P, cols, sc.K, sc.H, sc.W, rad, m["g"], view_scale)
    assert tuple(img.shape) == (int(sc.H * view_scale), int(sc.W * view_scale), 3)
    ok = ~want["near"]
    np.testing.assert_allclose(img.cpu().numpy()[ok], want["img"][ok], rtol=0, atol=1e-5)     # the forward it differentiates
    _assert_close("points", gp.cpu().numpy(), m["gp"], ~ex)
    _assert_close("colours", gc.cpu().numpy(), m["gc"], ~ex)
    assert (np.abs(m["gp"]).max(1) > 0).mean() > 0.5             # most points reach a pixel


def _hand(scene, n_track=rm.N_TRACK, max_lost=0.0):
    P, cols, K, H, W, rad = scene
    fact = rc.hand_scene_facts(P, cols, K, H, W, rad, n_track, max_lost=max_lost)
    g = rc.masked_grad(fact["near"])
    want_p, want_c = rc.model_grads(P, cols, g, fact["hits"], K, H, W, rad)
    _, gp, gc = _hip_both(P, cols, K, H, W, rad, g, n_track=n_track)
    gp, gc = gp.cpu().numpy(), gc.cpu().numpy()
    print(f"  near {fact['near_share']:.4f} of the pixels, {fact['lost']} surfels lost, {int(fact['taken'].sum())} taken")
    every = np.ones(len(P), bool)
    _assert_close("points", gp, want_p, every)
    _assert_close("colours", gc, want_c, every)
    return fact, gp, gc


def test_backward_of_big_splats_clipped_by_every_border():
    """boxes 40..120 px wide on 100 x 150: three to eight tiles per axis, eight of them centred outside the image"""
    fact, gp, gc = _hand(rc.big_splats())
    assert fact["taken"].all()
    assert (np.abs(gp).max(1) > 0).all() and (np.abs(gc).max(1) > 0).all()


def test_backward_on_the_overflow_path_with_neighbours():
    """more than RN_SORT_CAP keys in tile (1,1), whose surfels also lie in the eight neighbours' lists and theirs in its"""
    sc = rc.overflow_with_neighbours()
    lists = rc.tile_lists(sc[0], *sc[2:])
    assert len(lists[(1, 1)]) > 4096
    assert all(len(lists[t] & lists[(1, 1)]) > 0 for t in lists if max(abs(t[0] - 1), abs(t[1] - 1)) == 1)
    fact, gp, gc = _hand(sc, max_lost=rc.OVERFLOW_MAX_LOST)
    assert (gp[~fact["taken"]] == 0).all() and (gc[~fact["taken"]] == 0).all()       # behind the cut everywhere: exactly 0


@pytest.mark.parametrize("n_track", [rm.N_TRACK, 3])
def test_backward_with_depth_ties_at_the_cut(n_track):
    """70 coincident surfels, the n_track cut inside the group: equal depth goes by row, as the keys do"""
    sc = rc.ties()
    fact, gp, gc = _hand(sc, n_track)
    assert fact["near_share"] == 0.0
    behind_the_cut = ~fact["taken"]
    assert 0 < behind_the_cut.sum() < len(behind_the_cut)
    assert (gp[behind_the_cut] == 0).all() and (gc[behind_the_cut] == 0).all()
    assert (np.abs(gc[fact["taken"]]).max(1) > 0).all()


def test_a_context_reused_across_sizes(full):
    """full size, a small scene, full size again on one context: the third result equals the first bitwise (nothing of the
    small render's lists, slab or pixel records survives into the next backward)"""
    import torch
    from super_amd.renderer import RenderContext
    sc, cols, P = full["sc"], full["cols"], full["f64"]
    m = full["model"](1e-3, 1.0)
    ctx = RenderContext(sc.H, sc.W)
    first = _hip_both(P, cols, sc.K, sc.H, sc.W, 1e-3, m["g"], ctx=ctx)
    small = rc.ties()
    fact = rc.hand_scene_facts(*small)
    g = rc.masked_grad(fact["near"])
    _, gp, gc = _hip_both(*small, g, ctx=ctx)
    want_p, want_c = rc.model_grads(small[0], small[1], g, fact["hits"], *small[2:])
    _assert_close("points", gp.cpu().numpy(), want_p, np.ones(len(want_p), bool))
    _assert_close("colours", gc.cpu().numpy(), want_c, np.ones(len(want_c), bool))
    third = _hip_both(P, cols, sc.K, sc.H, sc.W, 1e-3, m["g"], ctx=ctx)
    for a, b in zip(first, third):
        assert torch.equal(a, b)
    _assert_close("points", third[1].cpu().numpy(), m["gp"], ~m["ex"])


# ---- 3. the chain once at the driver's size ---------------------------------------------------------------------------

def test_graphfit_render_loss_at_full_size(full):
    """test_gpu_graphfit_render_loss.test_loss_and_grad_match_the_oracle at 480x640 with 300 000 surfels (its helpers,
    with the radius and the vectorised hit sets passed in): one evaluation of loss and dv gradient at a perturbed dv.
    rad = 2e-3 fills the image (at 1e-3 only 8 % of the windows are free of background); the perturbation and the
    target's shift are a tenth of the 60x80 test's, half a pixel here, so that m stays below 0.1 (294 654 pixels kept);
    weight 1e-4 puts the term's gradient at a few times the geometric terms' (3.6 by the models).
    Tolerances as there: 1e-9 relative on the loss terms, 1e-8 of the largest entry on the gradient."""
    import torch
    import test_gpu_graphfit_render_loss as T
    from oracle import graphfit_oracle as gfo
    from super_amd.deform_mesh import GraphFit
    sc, cols = full["sc"], full["cols"]
    rad, weight = 2e-3, 1e-4
    stable = np.random.default_rng(12).uniform(size=sc.N) > 0.1
    tg = rm.render(sc.sf_points[stable] + np.array([0.0001, -0.00005, 0.0]), cols[stable], sc.K, sc.H, sc.W, rad)["img"]
    tgt = (np.transpose(tg, (2, 0, 1)) + 0.01 * np.random.default_rng(5).normal(size=(3, sc.H, sc.W))).astype(np.float32)
    opt = T._opt(renderer_rad=rad, render_loss_weight=weight)
    J = 512
    dv = np.zeros((J + 1, 7))
    dv[:, 0] = 1.0
    rng = np.random.default_rng(9)
    dv[:, :4] += 0.0002 * rng.normal(size=(J + 1, 4))
    dv[:, 4:] += 0.00005 * rng.normal(size=(J + 1, 3))
    sf, inputs, new_data, _ = T._gpu_frame(sc, stable, cols, tgt)
    gf = GraphFit(opt, native_render_loss=True)
    d, matched, grad = gf.loss_and_grad(inputs, sf, new_data, torch.from_numpy(dv).cuda())
    pb = gfo.Problem(sc, stable=stable)
    assert pb.J == J
    dvt = torch.from_numpy(dv).requires_grad_(True)
    loss, terms = gfo.total_loss(pb, dvt, opt)
    _, P = gfo.deform(pb, dvt)
    lr, kept, _ = T._render_loss(sc, stable, cols, tgt, P, weight, rad=rad, hit_sets=rgm.hit_sets_fast)
    g_geo = torch.autograd.grad(loss, dvt, retain_graph=True)[0].numpy().copy()
    (loss + lr).backward()
    want = dvt.grad.numpy().copy()
    want[-1] /= pb.J
    g_geo[-1] /= pb.J
    got = grad.cpu().numpy()
    print(f"chain: kept {kept} render_loss {d['render_loss']!r} want {float(lr.detach())!r}; grad err / max "
          f"{np.abs(got - want).max() / np.abs(want).max():.2e}; render share of the gradient "
          f"{np.abs(want - g_geo).max() / np.abs(want).max():.2e}, geometric {np.abs(g_geo).max() / np.abs(want).max():.2e}")
    assert kept == gf.last_render_kept > 100_000
    for k in ("arap_loss", "rot_loss", "point_plane_loss"):
        t = float(terms[k].detach())
        assert abs(d[k] - t) <= 1e-9 * abs(t), k
    t = float(lr.detach())
    assert abs(d["render_loss"] - t) <= 1e-9 * abs(t)
    assert matched == int(terms["_matched"])
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-8 * np.abs(want).max())
    # the term and the geometric terms are both in the gradient well beyond the tolerance
    assert np.abs(want - g_geo).max() > 1e-3 * np.abs(want).max() and np.abs(g_geo).max() > 1e-3 * np.abs(want).max()
