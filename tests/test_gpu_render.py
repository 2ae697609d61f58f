"""The HIP surfel renderer (slm_render_points / slm_gf_render, python-super_amd/csrc/slm_render.hip) against the CPU
restatement of its spec (tests/render_model.py), through the C ABI and the ``Pulsar`` mirror.  Needs an MI355X.

Tolerance: 1e-5 absolute on colours; front-most row and hit count exactly.  Kernel and model evaluate the same
float64 expressions from the same float32 centres, so they differ by a few float64 roundings -- except at pixels
where a decision sits at its threshold (a sphere with |rho/rad - 1| < 1e-4, or an n_track cut between hits that
differ by less than 1e-4 gamma): those are excluded, and their number is asserted small."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import render_model as rm

pytestmark = pytest.mark.gpu


def _check(got, want, max_excluded=0.005):
    img, fid, cnt = (t.cpu().numpy() for t in got)
    ok = ~want["near"]
    assert (~ok).sum() <= max(3, max_excluded * ok.size), int((~ok).sum())
    assert img.shape == want["img"].shape
    np.testing.assert_allclose(img[ok], want["img"][ok], rtol=0, atol=1e-5)
    np.testing.assert_array_equal(fid[ok], want["front"][ok])
    np.testing.assert_array_equal(cnt[ok], want["count"][ok])


def _pulsar(H, W):
    from super_amd.renderer import Pulsar
    return Pulsar(SimpleNamespace(height=H, width=W))


def _render(P, cols, K, H, W, rad, view_scale=1.0, bg=(0.0, 0.0, 0.0), r=None):
    import torch
    r = r or _pulsar(H, W)
    data = SimpleNamespace(points=torch.as_tensor(P).cuda(), colors=torch.as_tensor(cols).float().cuda())
    inputs = {"K": torch.as_tensor(K).float()[None].cuda()}
    return r.render(inputs, data, view_scale=view_scale, rad=rad, bg_col=torch.tensor(bg), with_info=True)


K0 = np.array([[100.0, 0, 32.0], [0, 100.0, 24.0], [0, 0, 1]])
GAP = float(np.float32(1.0 + 0.5 * rm.GAMMA * (rm.Z_FAR - rm.Z_NEAR)))
HAND = {
    "one": ([[0, 0, 1.0]], 0.025),
    "front": ([[0, 0, 2.0], [0, 0, 1.0]], 0.02),
    "half_gamma": ([[0, 0, GAP], [0, 0, 1.0]], 0.02),
    "near_in": ([[0, 0, 0.011]], 1e-4),
    "near_out": ([[0, 0, 0.009]], 1e-4),
    "far_in": ([[0, 0, 14.99]], 0.2),
    "far_out": ([[0, 0, 15.01]], 0.2),
    "seventy": ([[0, 0, 1.0]] * 70, 0.02),
    "spread": ([[0.05 * (k % 7 - 3), 0.04 * (k // 7 - 2), 1.0 + 0.01 * k] for k in range(35)], 0.03),
}


@pytest.mark.parametrize("name", list(HAND))
def test_hand_scenes(name):
    P, rad = HAND[name]
    P = np.array(P, np.float64)
    cols = np.random.default_rng(len(P)).uniform(size=(len(P), 3)).astype(np.float32)
    want = rm.render(P, cols, K0, 48, 64, rad, bg=(0.1, 0.2, 0.3))
    _check(_render(P, cols, K0, 48, 64, rad, bg=(0.1, 0.2, 0.3)), want)
    if name == "seventy":
        assert want["count"][24, 32] == 64


@pytest.fixture(scope="module")
def scene():
    from super_amd import synth
    sc = synth.make_scene(N=300_000, J=512, H=480, W=640, seed=5, src_border=2)
    cols = np.random.default_rng(2).uniform(size=(sc.N, 3)).astype(np.float32)
    return sc, cols


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("rad", [2e-4, 2e-3])
def test_make_scene_full_size(scene, dtype, rad):
    sc, cols = scene
    P = sc.sf_points.astype(np.float32) if dtype == "f32" else sc.sf_points.astype(np.float64)
    want = rm.render(P, cols, sc.K, sc.H, sc.W, rad)
    got = _render(P, cols, sc.K, sc.H, sc.W, rad)
    _check(got, want)
    assert (want["count"] > 0).mean() > (0.1 if rad < 1e-3 else 0.8)
    if rad > 1e-3:
        assert want["count"].max() > 4                      # overlapping splats: a real blend


def test_view_scale_half(scene):
    sc, cols = scene
    want = rm.render(sc.sf_points, cols, sc.K, sc.H, sc.W, 2e-3, view_scale=0.5)
    got = _render(sc.sf_points, cols, sc.K, sc.H, sc.W, 2e-3, view_scale=0.5)
    assert tuple(got[0].shape) == (240, 320, 3)
    _check(got, want)


def test_a_tile_of_100k_surfels_takes_the_overflow_path():
    """100 000 surfels in one 16x16 tile (RN_SORT_CAP = 4096 keys fit in LDS): sorted runs merged in global memory"""
    rng = np.random.default_rng(4)
    n = 100_000
    Z = rng.uniform(0.5, 3.0, n)
    u, v = rng.uniform(17.5, 30.5, n), rng.uniform(17.5, 30.5, n)      # inside tile (1,1), its box stays there
    P = np.stack([(u - 32.0) * Z / 100.0, (v - 24.0) * Z / 100.0, Z], 1)
    cols = rng.uniform(size=(n, 3)).astype(np.float32)
    rad = 1.0 * Z.min() / 100.0                                        # <= 1 px
    want = rm.render(P, cols, K0, 48, 64, rad)
    _check(_render(P, cols, K0, 48, 64, rad), want)
    assert want["count"][18:30, 18:30].min() == rm.N_TRACK         # every pixel of the tile interior is cut at 64


def test_no_points_and_all_culled():
    import torch
    bg = (0.25, 0.5, 0.75)
    img, fid, cnt = _render(np.zeros((0, 3)), np.zeros((0, 3), np.float32), K0, 48, 64, 0.02, bg=bg)
    np.testing.assert_array_equal(img.cpu().numpy(), np.tile(np.float32(bg), (48, 64, 1)))
    assert (fid == -1).all() and (cnt == 0).all()
    P = np.array([[0, 0, 0.005], [0, 0, 20.0], [0, 0, -1.0], [50.0, 0, 1.0]])
    img, fid, cnt = _render(P, np.ones((4, 3), np.float32), K0, 48, 64, 0.02, bg=bg)
    np.testing.assert_array_equal(img.cpu().numpy(), np.tile(np.float32(bg), (48, 64, 1)))
    assert (fid == -1).all() and (cnt == 0).all()
    del torch


def test_two_renders_are_bitwise_equal(scene):
    import torch
    sc, cols = scene
    r = _pulsar(sc.H, sc.W)
    a = _render(sc.sf_points, cols, sc.K, sc.H, sc.W, 2e-3, r=r)
    b = _render(sc.sf_points, cols, sc.K, sc.H, sc.W, 2e-3, r=r)
    c = _render(sc.sf_points, cols, sc.K, sc.H, sc.W, 2e-3)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_pulsar_forward_matches_the_reference_surface():
    import torch
    from super_amd.renderer import Pulsar
    r = Pulsar(SimpleNamespace(height=48, width=64))
    P = torch.tensor([[0, 0, 1.0]], dtype=torch.float64, device="cuda")
    data = SimpleNamespace(points=P, colors=torch.tensor([[0.5, 0.25, 1.0]], device="cuda"))
    inputs = {"K": torch.from_numpy(K0).float()[None].cuda()}
    out = r(inputs, data, rad=0.025)
    assert out.dtype == torch.float32 and tuple(out.shape) == (48, 64, 3) and out.is_cuda
    assert out[24, 32].tolist() == [0.5, 0.25, 1.0]
    wide = torch.tensor([[0.5, 0.25, 1.0, 9.0]], device="cuda")[:, :3]          # strided colours, no copy needed
    assert torch.equal(r(inputs, data, colors=wide, rad=0.025), out)
    with pytest.raises(RuntimeError, match="forward only"):
        r(inputs, SimpleNamespace(points=P.clone().requires_grad_(True), colors=data.colors), rad=0.025)


def test_render_img_sets_both_images(scene):
    import torch
    from super_amd.renderer import conf2color, render_img
    sc, cols = scene
    n = 20_000
    rng = np.random.default_rng(8)
    stable = rng.uniform(size=n) > 0.3
    confs = rng.uniform(-0.1, 1.1, n)
    sf = SimpleNamespace(points=torch.from_numpy(sc.sf_points[:n]).cuda(), colors=torch.from_numpy(cols[:n]).double().cuda(),
                         confs=torch.from_numpy(confs).cuda(), isStable=torch.from_numpy(stable).cuda(),
                         opt=SimpleNamespace(height=sc.H, width=sc.W, renderer_rad=2e-3))
    inputs = {"K": torch.from_numpy(sc.K).float()[None].cuda()}
    render_img(sf, inputs)
    assert tuple(sf.renderImg.shape) == (1, 3, sc.H, sc.W) and tuple(sf.renderImg_conf_heat.shape) == (1, 3, sc.H, sc.W)
    heat = conf2color(torch.from_numpy(confs)).numpy()[stable]
    for img, c in ((sf.renderImg, cols[:n][stable]), (sf.renderImg_conf_heat, heat)):
        want = rm.render(sc.sf_points[:n][stable], c, sc.K, sc.H, sc.W, 2e-3)
        got = img[0].permute(1, 2, 0).cpu().numpy()
        ok = ~want["near"]
        np.testing.assert_allclose(got[ok], want["img"][ok], rtol=0, atol=1e-5)


def test_bad_arguments_are_refused():
    import torch
    from super_amd import _lib
    from super_amd.renderer import RenderContext, render_params
    lib = _lib.load()
    ctx = RenderContext(48, 64, 10)
    img = torch.empty((48, 64, 3), device="cuda")
    p = render_params(K0, 48, 64, 1.0, 0.02)
    pts = torch.zeros((20, 3), device="cuda")
    assert lib.slm_render_points(ctx.h, C.byref(p), 20 + ctx.cap, pts.data_ptr(), pts.data_ptr(), 3, img.data_ptr(),
                                 None, None, None) != 0
    p2 = render_params(K0, 96, 64, 1.0, 0.02)                    # larger than the context
    assert lib.slm_render_points(ctx.h, C.byref(p2), 1, pts.data_ptr(), pts.data_ptr(), 3, img.data_ptr(),
                                 None, None, None) != 0
    p.n_track = 65
    assert lib.slm_render_points(ctx.h, C.byref(p), 1, pts.data_ptr(), pts.data_ptr(), 3, img.data_ptr(),
                                 None, None, None) != 0 and b"n_track" in lib.slm_last_error()
