"""The HIP renderer with one radius per point (slm_render_points_radii, slm_render_backward_radii) against the CPU
restatement tests/render_radii_model.py, on the scenes of tests/render_radii_cases.py (their facts are checked on the CPU by
test_render_radii_cases.py).  Needs an MI355X.

Tolerances are those of the one-radius tests for the same arithmetic: 1e-5 absolute on colours, front-most row and hit
count exactly, pixels with a decision at its threshold (`near`) excluded (test_gpu_render.py); gradients to 1e-9 of the
largest entry, rows with a `near` candidate pixel left out, at most 5 % of them (test_gpu_render_grad.py)."""
import ctypes as C

import numpy as np
import pytest

import render_radii_cases as rc

pytestmark = pytest.mark.gpu

BG = (0.1, 0.2, 0.3)


def _forward(s, dtype="f64", radii=True, rad=2e-4):
    """-> (ctx, params, (img, front_id, hit_count)) of the scene with its own radii, or with the one radius `rad`"""
    import torch
    from super_amd.renderer import RenderContext, render_params, render_points
    ctx = RenderContext(s["H"], s["W"])
    p = render_params(torch.as_tensor(s["K"])[None], s["H"], s["W"], s["view_scale"], rad, BG)
    p.n_track = s["n_track"]
    P = torch.as_tensor(s["P"].astype(np.float32 if dtype == "f32" else np.float64)).cuda()
    r = torch.as_tensor(s["radii"]).cuda() if radii else None
    return ctx, p, render_points(ctx, p, P, torch.as_tensor(s["cols"]).cuda(), with_info=True, radii=r)


def _check_image(got, want, max_excluded=0.005):
    img, fid, cnt = (t.cpu().numpy() for t in got)
    ok = ~want["near"]
    assert (~ok).sum() <= max(3, max_excluded * ok.size), int((~ok).sum())
    assert img.shape == want["img"].shape
    np.testing.assert_allclose(img[ok], want["img"][ok], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(fid[ok], want["front"][ok])
    np.testing.assert_array_equal(cnt[ok], want["count"][ok])
    return fid


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(rc.SCENES))
def test_forward_matches_the_model(name, dtype):
    f = rc.facts(name)
    s = f["scene"]
    _, _, got = _forward(s, dtype)
    fid = _check_image(got, f["want"])
    bad = np.nonzero(~np.isfinite(s["radii"]) | ~(s["radii"] > 0))[0]
    assert not np.isin(fid, bad).any()               # a culled row is never named, `near` pixels included
    if name == "mixed":
        assert len(bad) == 4


def test_equal_radii_are_bitwise_the_one_radius_path():
    import torch
    from super_amd.renderer import render_backward_ex
    s = rc.facts("link")["scene"]
    r32 = float(np.float32(rc.LINK_RAD))
    g = torch.from_numpy(rc.facts("link")["g"]).cuda()
    for dtype in ("f32", "f64"):
        ca, pa, a = _forward(s, dtype)
        ga = render_backward_ex(ca, pa, g)
        cb, pb, b = _forward(s, dtype, radii=False, rad=r32)
        gb = render_backward_ex(cb, pb, g)
        for x, y in zip(a + ga, b + gb):
            assert torch.equal(x, y)
        assert float(ga[0].abs().max()) > 0 and float(ga[1].abs().max()) > 0
    # and the one-radius path at 0.01, which is not a float32 value, is another render
    _, _, c = _forward(s, "f64", radii=False, rad=rc.LINK_RAD)
    assert not torch.equal(c[0], a[0])


@pytest.mark.parametrize("name", list(rc.SCENES))
def test_backward_matches_the_model(name):
    import torch
    from super_amd.renderer import render_backward, render_backward_ex
    f = rc.facts(name)
    s, ex = f["scene"], f["ex"]
    assert ex.mean() <= rc.MAX_EXCLUDED
    g = torch.from_numpy(f["g"]).cuda()
    ctx, p, _ = _forward(s)
    gp, gc, gr = render_backward_ex(ctx, p, g, radii=True)
    assert tuple(gr.shape) == (len(s["P"]),) and gr.dtype == torch.float64
    for got, want, what in zip((gp, gc, gr), f["grads"], ("dL/dP", "dL/dc", "dL/dr")):
        got = got.cpu().numpy()
        scale = np.abs(want).max()
        print(name, what, "scale", scale, "max err", np.abs(got[~ex] - want[~ex]).max() / scale, "left out", ex.mean())
        assert scale > 0
        np.testing.assert_allclose(got[~ex], want[~ex], rtol=0, atol=1e-9 * scale, err_msg=what)
    bad = ~np.isfinite(s["radii"]) | ~(s["radii"] > 0) | ~f["taken"]
    for t in (gp, gc, gr):                                    # culled rows (and rows hit nowhere): zero rows
        assert (t[torch.from_numpy(bad & ~ex).cuda()] == 0).all()
    # the old entry points use the stored radii: the same dL/dP and dL/dc, bit for bit
    assert torch.equal(render_backward(ctx, p, g), gp)
    p2, c2 = render_backward_ex(ctx, p, g)
    assert torch.equal(p2, gp) and torch.equal(c2, gc)
    # every output is the same whichever others are requested
    for wp, wc in ((False, False), (True, False), (False, True)):
        qp, qc, qr = render_backward_ex(ctx, p, g, wp, wc, radii=True)
        assert torch.equal(qr, gr) and (qp is None or torch.equal(qp, gp)) and (qc is None or torch.equal(qc, gc))
    assert torch.equal(render_backward_ex(ctx, p, g, True, False)[0], gp)
    assert torch.equal(render_backward_ex(ctx, p, g, False, True)[1], gc)
    # a second run on a fresh context is bitwise the same
    ctx2, p2, _ = _forward(s)
    for a, b in zip(render_backward_ex(ctx2, p2, g, radii=True), (gp, gc, gr)):
        assert torch.equal(a, b)


def test_two_forwards_are_bitwise_equal():
    import torch
    s = rc.facts("mixed")["scene"]
    _, _, a = _forward(s)
    _, _, b = _forward(s)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_the_radius_gradient_is_refused_after_a_one_radius_forward():
    import torch
    from super_amd import _lib
    f = rc.facts("link")
    s = f["scene"]
    g = torch.from_numpy(f["g"]).cuda()
    n = len(s["P"])
    gp = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    gr = torch.empty(n, dtype=torch.float64, device="cuda")
    ctx, p, _ = _forward(s, radii=False, rad=0.01)
    lib = ctx.lib
    rc_ = lib.slm_render_backward_radii(ctx.h, C.byref(p), g.data_ptr(), gp.data_ptr(), None, gr.data_ptr(), None)
    assert rc_ == _lib.SLM_ERR_INVALID
    assert lib.slm_last_error() == b"slm_render_backward_radii: grad_radii after a forward with one radius"
    # without grad_radii it serves the one-radius forward like slm_render_backward_ex
    assert lib.slm_render_backward_radii(ctx.h, C.byref(p), g.data_ptr(), gp.data_ptr(), None, None, None) == 0
    from super_amd.renderer import render_backward
    assert torch.equal(gp, render_backward(ctx, p, g))
    rc_ = lib.slm_render_backward_radii(ctx.h, C.byref(p), g.data_ptr(), None, None, None, None)
    assert rc_ == _lib.SLM_ERR_INVALID
    assert lib.slm_last_error() == b"slm_render_backward_radii: null grad_points, grad_colors and grad_radii"
    torch.cuda.synchronize()


def test_no_points():
    import torch
    from super_amd.renderer import render_backward_ex
    s = dict(rc.facts("inside")["scene"])
    s["P"], s["cols"], s["radii"] = s["P"][:0], s["cols"][:0], s["radii"][:0]
    ctx, p, (img, fid, cnt) = _forward(s)
    np.testing.assert_array_equal(img.cpu().numpy(), np.tile(np.float32(BG), (48, 64, 1)))
    assert (fid == -1).all() and (cnt == 0).all()
    gp, gc, gr = render_backward_ex(ctx, p, torch.ones((48, 64, 3), dtype=torch.float64, device="cuda"), radii=True)
    assert tuple(gp.shape) == (0, 3) and tuple(gr.shape) == (0,)
