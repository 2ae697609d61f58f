"""The HIP renderer with N-channel features (slm_render_points_channels, slm_render_backward_channels) against the float64
model tests/render_channels_model.py, on the scenes of tests/render_radii_cases.py with the features of
tests/render_channels_cases.py.  Needs an MI355X.

Tolerances are those of the three-channel tests for the same arithmetic: 1e-5 absolute on a channel of values in [0,1] (1e-5
of the column's largest magnitude for a depth column), front-most row and hit count exactly, `near` pixels excluded (at most
0.5 %); gradients to 1e-9 of the largest entry on the rows render_radii_cases leaves in (at most 5 % left out).  The channel
rule -- a channel is what the three-channel entry gives for the same column -- is checked bitwise."""
import ctypes as C

import numpy as np
import pytest

import render_channels_cases as cc
import render_radii_cases as rc

pytestmark = pytest.mark.gpu

CHANNELS = [1, 2, 4, 6, 8]


def _params(s, rad=2e-4, bg3=(0.0, 0.0, 0.0)):
    import torch
    from super_amd.renderer import render_params
    p = render_params(torch.as_tensor(s["K"])[None], s["H"], s["W"], s["view_scale"], rad, bg3)
    p.n_track = s["n_track"]
    return p


def _points(s, dtype="f64"):
    import torch
    return torch.as_tensor(s["P"].astype(np.float32 if dtype == "f32" else np.float64)).cuda()


def _forward(s, feat, bg, dtype="f64", radii=True, rad=2e-4, ctx=None):
    """-> (ctx, params, (img, front_id, hit_count)) of the scene with its own radii, or with the one radius `rad`"""
    import torch
    from super_amd.renderer import RenderContext, render_channels
    ctx = ctx or RenderContext(s["H"], s["W"])
    p = _params(s, rad)
    r = torch.as_tensor(s["radii"]).cuda() if radii else None
    return ctx, p, render_channels(ctx, p, _points(s, dtype), torch.as_tensor(feat).cuda(), bg=bg, with_info=True, radii=r)


def _forward3(s, cols, bg3, radii=True, rad=2e-4, ctx=None):
    """the existing three-channel entries on the same scene"""
    import torch
    from super_amd.renderer import RenderContext, render_points
    ctx = ctx or RenderContext(s["H"], s["W"])
    p = _params(s, rad, bg3)
    r = torch.as_tensor(s["radii"]).cuda() if radii else None
    return ctx, p, render_points(ctx, p, _points(s), torch.as_tensor(cols).cuda(), with_info=True, radii=r)


def _check_image(got, want, atol=1e-5, max_excluded=0.005):
    img, fid, cnt = (t.cpu().numpy() for t in got)
    ok = ~want["near"]
    assert (~ok).sum() <= max(3, max_excluded * ok.size), int((~ok).sum())
    assert img.shape == want["img"].shape and img.dtype == np.float32
    print("max err", np.abs(img[ok] - want["img"][ok]).max(initial=0.0), "near", int((~ok).sum()))
    np.testing.assert_allclose(img[ok], want["img"][ok], rtol=0, atol=atol)
    np.testing.assert_array_equal(fid[ok], want["front"][ok])
    np.testing.assert_array_equal(cnt[ok], want["count"][ok])
    return fid


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", list(rc.SCENES))
@pytest.mark.parametrize("nch", CHANNELS)
def test_forward_matches_the_model(nch, name, dtype):
    s = rc.facts(name)["scene"]
    _, _, got = _forward(s, cc.features(name, nch), cc.bg(nch), dtype)
    fid = _check_image(got, cc.want(name, nch))
    bad = np.nonzero(~np.isfinite(s["radii"]) | ~(s["radii"] > 0))[0]
    assert not np.isin(fid, bad).any()               # a culled row is never named
    if name == "overflow":
        assert (cc.want(name, nch)["near"]).sum() == 0


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("nch", CHANNELS)
def test_forward_with_one_radius_matches_the_model(nch, dtype):
    s = rc.facts("link")["scene"]
    want = cc.want("link", nch, True)
    assert (want["count"] > 0).any()                 # this radius covers pixels
    _, _, got = _forward(s, cc.features("link", nch), cc.bg(nch), dtype, radii=False, rad=cc.ONE_RADIUS)
    _check_image(got, want)


def test_a_depth_column():
    import render_channels_model as rcm
    s = rc.facts("mixed")["scene"]
    feat = np.stack([cc.features("mixed", 1)[:, 0], s["P"][:, 2].astype(np.float32)], 1)
    bg = np.float32([0.25, 0.0])
    want = rcm.render(s["P"], feat, s["radii"], s["K"], s["H"], s["W"], s["view_scale"], bg=bg, n_track=s["n_track"])
    _, _, got = _forward(s, feat, bg)
    img = got[0].cpu().numpy()
    ok = ~want["near"]
    top = float(np.abs(feat[:, 1]).max())
    assert 0.8 < top < 1.2
    np.testing.assert_allclose(img[ok][:, 0], want["img"][ok][:, 0], rtol=0, atol=1e-5)
    np.testing.assert_allclose(img[ok][:, 1], want["img"][ok][:, 1], rtol=0, atol=1e-5 * top)
    assert img[ok][:, 1].max() > 0.9                 # depths were blended, not only the background


@pytest.mark.parametrize("name", ["mixed", "overflow"])
def test_a_channel_is_bitwise_the_three_channel_render_of_its_column(name):
    import torch
    s = rc.facts(name)["scene"]
    feat, bg = cc.features(name, 8), cc.bg(8)
    _, _, (img8, fid8, cnt8) = _forward(s, feat, bg)
    for c0 in (0, 3, 6):
        k = min(3, 8 - c0)
        cols = np.zeros((len(feat), 3), np.float32)
        cols[:, :k] = feat[:, c0:c0 + k]
        bg3 = np.zeros(3, np.float32)
        bg3[:k] = bg[c0:c0 + k]
        _, _, (img3, fid3, cnt3) = _forward3(s, cols, bg3)
        assert torch.equal(img8[..., c0:c0 + k], img3[..., :k]), c0
        assert torch.equal(fid8, fid3) and torch.equal(cnt8, cnt3)
    assert float((cnt8 > 0).float().mean()) > 0.05


@pytest.mark.parametrize("name,radii", [("mixed", True), ("overflow", True), ("link", False)])
def test_three_channels_are_bitwise_the_existing_entry(name, radii):
    import torch
    f = rc.facts(name)
    s = f["scene"]
    bg3 = np.float32([0.1, 0.2, 0.3])
    _, _, a = _forward(s, s["cols"], bg3, radii=radii, rad=cc.ONE_RADIUS)
    _, _, b = _forward3(s, s["cols"], bg3, radii=radii, rad=cc.ONE_RADIUS)
    for x, y in zip(a, b):
        assert x.shape == y.shape and torch.equal(x, y)
    assert float((a[2] > 0).float().mean()) > 0.05


def _check_grads(got, want, ex, label):
    for g, w, what in zip(got, want, ("dL/dP", "dL/df", "dL/dr")):
        g = g.cpu().numpy()
        scale = np.abs(w).max()
        print(label, what, "scale", scale, "max err", np.abs(g[~ex] - w[~ex]).max() / scale, "left out", ex.mean())
        assert scale > 0 and g.shape == w.shape
        np.testing.assert_allclose(g[~ex], w[~ex], rtol=0, atol=1e-9 * scale, err_msg=what)


@pytest.mark.parametrize("name", list(rc.SCENES))
@pytest.mark.parametrize("nch", [1, 4, 8])
def test_backward_matches_the_model(nch, name):
    import torch
    from super_amd.renderer import render_backward_channels
    f = rc.facts(name)
    s, ex = f["scene"], f["ex"]
    assert ex.mean() <= rc.MAX_EXCLUDED
    gf = cc.grad_facts(name, nch)
    g = torch.from_numpy(gf["g"]).cuda()
    ctx, p, _ = _forward(s, cc.features(name, nch), cc.bg(nch))
    got = render_backward_channels(ctx, p, g, radii=True)
    assert tuple(got[1].shape) == (len(s["P"]), nch) and all(t.dtype == torch.float64 for t in got)
    _check_grads(got, gf["grads"], ex, f"{name} C={nch}")
    bad = ~np.isfinite(s["radii"]) | ~(s["radii"] > 0) | ~f["taken"]
    for t in got:                                             # culled rows (and rows hit nowhere): zero rows
        assert (t[torch.from_numpy(bad & ~ex).cuda()] == 0).all()


@pytest.mark.parametrize("name", list(rc.SCENES))
def test_backward_with_three_channels_is_the_existing_backward(name):
    import torch
    from super_amd.renderer import render_backward_channels, render_backward_ex
    f = rc.facts(name)
    s = f["scene"]
    bg3 = np.float32([0.1, 0.2, 0.3])
    g = torch.from_numpy(f["g"]).cuda()
    ctx, p, _ = _forward(s, s["cols"], bg3)
    got = render_backward_channels(ctx, p, g, radii=True)
    ctx3, p3, _ = _forward3(s, s["cols"], bg3)
    old = render_backward_ex(ctx3, p3, g, radii=True)
    none = np.zeros(len(s["P"]), bool)
    _check_grads(got, [t.cpu().numpy() for t in old], none, name + " C=3 against slm_render_backward_radii")
    _check_grads(got, f["grads"], f["ex"], name + " C=3 against the model")


@pytest.mark.parametrize("name,nch", [("mixed", 8), ("overflow", 5), ("cut64", 1)])
def test_outputs_do_not_depend_on_each_other_and_runs_are_bitwise_equal(name, nch):
    import torch
    from super_amd.renderer import render_backward_channels
    s = rc.facts(name)["scene"]
    g = torch.from_numpy(cc.grad_facts(name, nch)["g"] if nch in (1, 4, 8) else
                         np.random.default_rng(nch).normal(size=rc.facts(name)["want"]["near"].shape + (nch,))).cuda()
    ctx, p, fwd = _forward(s, cc.features(name, nch), cc.bg(nch))
    full = render_backward_channels(ctx, p, g, radii=True)
    assert all(float(t.abs().max()) > 0 for t in full)
    for wp in (False, True):
        for wf in (False, True):
            for wr in (False, True):
                if not (wp or wf or wr):
                    continue
                part = render_backward_channels(ctx, p, g, wp, wf, wr)
                for want_it, a, b in zip((wp, wf, wr), part, full):
                    assert (a is None) == (not want_it)
                    assert a is None or torch.equal(a, b), (wp, wf, wr)
    ctx2, p2, fwd2 = _forward(s, cc.features(name, nch), cc.bg(nch))     # a second run on a fresh context
    for a, b in zip(fwd2 + render_backward_channels(ctx2, p2, g, radii=True), fwd + full):
        assert torch.equal(a, b)


def _raw_backward(ctx, p, nch, g, n, radii=False):
    import torch
    gp = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    gr = torch.empty(n, dtype=torch.float64, device="cuda")
    rc_ = ctx.lib.slm_render_backward_channels(ctx.h, C.byref(p), nch, g.data_ptr(), gp.data_ptr(), None,
                                               gr.data_ptr() if radii else None, None)
    return rc_, ctx.lib.slm_last_error()


def test_refusals_that_need_a_context():
    import torch
    from super_amd import _lib
    from super_amd.renderer import RenderContext, render_backward, render_backward_channels, render_backward_ex
    f = rc.facts("link")
    s = f["scene"]
    n, INVALID = len(s["P"]), _lib.SLM_ERR_INVALID
    g4 = torch.from_numpy(cc.grad_facts("link", 4)["g"]).cuda()
    g3 = torch.from_numpy(f["g"]).cuda()
    who = b"slm_render_backward_channels: "
    fresh = RenderContext(s["H"], s["W"])
    assert _raw_backward(fresh, _params(s), 4, g4, n) == (INVALID, who + b"no completed forward on this context")
    # after a channels forward (also at C = 3) the three-channel backward entries refuse, naming the new one
    for nch in (4, 3):
        ctx, p, _ = _forward(s, cc.features("link", 4)[:, :nch], cc.bg(nch))
        for call in (lambda: render_backward(ctx, p, g3), lambda: render_backward_ex(ctx, p, g3),
                     lambda: render_backward_ex(ctx, p, g3, radii=True)):
            with pytest.raises(_lib.SuperLMError, match="use slm_render_backward_channels"):
                call()
    gp = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    assert ctx.lib.slm_render_backward(ctx.h, C.byref(p), g3.data_ptr(), gp.data_ptr(), None) == INVALID
    assert ctx.lib.slm_last_error() == (b"slm_render_backward: the last forward had N-channel features: "
                                        b"use slm_render_backward_channels")
    # after a three-channel forward the channels backward refuses
    ctx3, p3, _ = _forward3(s, s["cols"], (0.0, 0.0, 0.0))
    assert _raw_backward(ctx3, p3, 3, g3, n) == (INVALID, who + b"the last forward was not slm_render_points_channels")
    # another channel count, other parameters, the radius gradient after a one-radius forward
    ctx, p, _ = _forward(s, cc.features("link", 4), cc.bg(4))
    assert _raw_backward(ctx, p, 3, g3, n) == (INVALID, who + b"channels differ from those of the last forward")
    q = _params(s, 3e-4)
    assert _raw_backward(ctx, q, 4, g4, n) == (INVALID, who + b"parameters differ from those of the last forward")
    assert _raw_backward(ctx, p, 4, g4, n)[0] == 0
    rc_ = ctx.lib.slm_render_backward_channels(ctx.h, C.byref(p), 4, g4.data_ptr(), None, None, None, None)
    assert (rc_, ctx.lib.slm_last_error()) == (INVALID, who + b"null grad_points, grad_features and grad_radii")
    ctx1, p1, _ = _forward(s, cc.features("link", 4), cc.bg(4), radii=False, rad=cc.ONE_RADIUS)
    assert _raw_backward(ctx1, p1, 4, g4, n, radii=True) == (INVALID, who + b"grad_radii after a forward with one radius")
    gp1, gf1, _ = render_backward_channels(ctx1, p1, g4)            # without it the one-radius forward is served
    assert float(gp1.abs().max()) > 0 and float(gf1.abs().max()) > 0
    with pytest.raises(ValueError, match="features must be"):
        _forward(s, np.zeros((n, 9), np.float32), np.zeros(9, np.float32))
    torch.cuda.synchronize()


def test_no_points():
    import torch
    from super_amd.renderer import render_backward_channels
    s = dict(rc.facts("inside")["scene"])
    s["P"], s["radii"] = s["P"][:0], s["radii"][:0]
    bg = cc.bg(5)
    ctx, p, (img, fid, cnt) = _forward(s, np.zeros((0, 5), np.float32), bg)
    np.testing.assert_array_equal(img.cpu().numpy(), np.tile(bg, (48, 64, 1)))
    assert (fid == -1).all() and (cnt == 0).all()
    gp, gf, gr = render_backward_channels(ctx, p, torch.ones((48, 64, 5), dtype=torch.float64, device="cuda"), radii=True)
    assert tuple(gp.shape) == (0, 3) and tuple(gf.shape) == (0, 5) and tuple(gr.shape) == (0,)


def test_a_context_serves_a_three_channel_render_afterwards():
    import torch
    from super_amd.renderer import render_backward_ex
    f = rc.facts("mixed")
    s = f["scene"]
    bg3 = (0.1, 0.2, 0.3)
    ctx, _, _ = _forward(s, cc.features("mixed", 8), cc.bg(8))
    _, p, got = _forward3(s, s["cols"], bg3, ctx=ctx)
    _, p0, ref = _forward3(s, s["cols"], bg3)
    for x, y in zip(got, ref):
        assert torch.equal(x, y)
    _check_image(got, f["want"])
    g = torch.from_numpy(f["g"]).cuda()
    got_g = render_backward_ex(ctx, p, g, radii=True)
    _check_grads(got_g, f["grads"], f["ex"], "mixed after a channels render")
    # and a channels render on it again, narrower than the first
    _, _, again = _forward(s, cc.features("mixed", 2), cc.bg(2), ctx=ctx)
    _check_image(again, cc.want("mixed", 2))
