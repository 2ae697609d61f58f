"""The CPU restatement of the surfel renderer (tests/render_model.py) pinned with hand-computed scenes, the pixel
alignment with pcd2depth, conf2color against matplotlib, and the slm_render_params layout.  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import render_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = 100.0


def _K(f=F, cx=32.0, cy=24.0):
    return np.array([[f, 0, cx], [0, f, cy], [0, 0, 1.0]])


def _one(P, c, rad, **kw):
    return rm.render(np.array(P, np.float64).reshape(-1, 3), np.array(c, np.float64).reshape(-1, 3),
                     _K(), 48, 64, rad, **kw)


def test_camera_follows_the_reference_call():
    assert rm.camera(_K(cx=32.4, cy=23.6), 48, 64) == (64, 48, F, 33.0, 24.0)
    assert rm.camera(_K(cx=319.5, cy=239.5), 480, 640, 0.5) == (320, 240, 50.0, 160.0, 120.0)
    assert rm.camera(_K(cx=10.0, cy=10.0), 21, 31, 1.0) == (31, 21, F, 10.5, 10.5)   # odd sizes: half-pixel centre


def test_one_sphere_covers_the_pixels_within_its_radius():
    # centre on the optical axis: rho = (r/f) / sqrt(1 + (r/f)^2) for a pixel r pixels from (cx, cy)
    c = (0.2, 0.5, 0.9)
    out = _one([0, 0, 1.0], c, 0.025)
    ii, jj = np.mgrid[0:48, 0:64]
    want = (ii - 24) ** 2 + (jj - 32) ** 2 <= 6          # 2.5 px: the integer offsets with a^2 + b^2 <= 6
    assert want.sum() == 21
    np.testing.assert_array_equal(out["count"] > 0, want)
    np.testing.assert_allclose(out["img"][want], np.tile(np.float32(c), (21, 1)), rtol=0, atol=1e-15)
    assert (out["img"][~want] == 0).all() and (out["front"][want] == 0).all() and (out["front"][~want] == -1).all()
    assert not out["near"].any()


def test_front_sphere_wins():
    out = _one([[0, 0, 2.0], [0, 0, 1.0]], [[1, 0, 0], [0, 1, 0]], 0.02)
    assert out["front"][24, 32] == 1 and out["count"][24, 32] == 2
    np.testing.assert_array_equal(out["img"][24, 32], [0, 1, 0])     # exp(-(1/14.99)/1e-5) == 0


def test_two_spheres_half_gamma_apart_blend_with_the_hand_weights():
    z2 = float(np.float32(1.0 + 0.5 * rm.GAMMA * (rm.Z_FAR - rm.Z_NEAR)))
    c1, c2 = np.array([1.0, 0, 0]), np.array([0, 0.5, 1.0])
    out = _one([[0, 0, z2], [0, 0, 1.0]], [c2, c1], 0.02)
    e = math.exp(-(z2 - 1.0) / (rm.Z_FAR - rm.Z_NEAR) / rm.GAMMA)    # rho = 0 on the axis: d = 1 for both
    assert abs(e - math.exp(-0.5)) < 1e-3
    np.testing.assert_allclose(out["img"][24, 32], (c1 + e * c2) / (1 + e), rtol=0, atol=1e-10)
    # one pixel to the right: d_k = 1 - rho_k / rad with rho from the closed form
    r = lambda z: z * (1 / F) / math.sqrt(1 + 1 / F ** 2)
    d1, d2 = 1 - r(1.0) / 0.02, 1 - r(z2) / 0.02
    np.testing.assert_allclose(out["img"][24, 33], (d1 * c1 + d2 * e * c2) / (d1 + d2 * e), rtol=0, atol=1e-10)


def test_background_only():
    out = rm.render(np.zeros((0, 3)), np.zeros((0, 3)), _K(), 48, 64, 0.02, bg=(0.2, 0.3, 0.4))
    np.testing.assert_array_equal(out["img"], np.tile([0.2, 0.3, 0.4], (48, 64, 1)))
    assert (out["front"] == -1).all() and (out["count"] == 0).all()


@pytest.mark.parametrize("z,rad,seen", [(0.009, 1e-4, False), (0.011, 1e-4, True), (15.01, 0.2, False), (14.99, 0.2, True)])
def test_culling_at_z_near_and_z_far(z, rad, seen):
    out = _one([0, 0, z], [1, 1, 1], rad)
    assert (out["count"][24, 32] == 1) == seen


def test_seventy_coincident_spheres_exactly_64_take_part():
    rng = np.random.default_rng(0)
    c = rng.uniform(size=(70, 3)).astype(np.float32)
    out = _one(np.tile([0, 0, 1.0], (70, 1)), c, 0.02)
    assert out["count"][24, 32] == 64 and out["front"][24, 32] == 0
    np.testing.assert_allclose(out["img"][24, 32], c[:64].astype(np.float64).mean(0), rtol=0, atol=1e-10)


def test_view_scale_half():
    K = _K(cx=31.0, cy=23.0)
    P = np.array([[0.1, -0.06, 1.0]])
    out = rm.render(P, [[1, 1, 1]], K, 48, 64, 0.03, view_scale=0.5)
    assert out["img"].shape == (24, 32, 3)
    w, h, f, ccx, ccy = rm.camera(K, 48, 64, 0.5)
    assert (w, h, f, ccx, ccy) == (32, 24, 50.0, 16.0, 12.0)      # 16 + ceil(15.5 - 16), 12 + ceil(11.5 - 12)
    # centre at (u,v) = (0.1*50 + 16, -0.06*50 + 12) = (21, 9), radius 1.5 px: the 3x3 block around it
    want = np.zeros((24, 32), bool)
    want[8:11, 20:23] = True
    np.testing.assert_array_equal(out["count"] > 0, want)


def test_float64_points_are_rounded_to_float32_first():
    dz = 0.5 * rm.GAMMA * (rm.Z_FAR - rm.Z_NEAR)
    z2f = float(np.float32(1.0 + dz))
    z2 = z2f + 0.45 * 2.0 ** -23                               # not a float32 value: rounds down to z2f
    assert float(np.float32(z2)) == z2f
    c1, c2 = np.array([1.0, 0, 0]), np.array([0, 0.5, 1.0])
    out = _one([[0, 0, z2], [0, 0, 1.0]], [c2, c1], 0.02)
    ef = math.exp(-(z2f - 1.0) / (rm.Z_FAR - rm.Z_NEAR) / rm.GAMMA)
    e64 = math.exp(-(z2 - 1.0) / (rm.Z_FAR - rm.Z_NEAR) / rm.GAMMA)
    np.testing.assert_allclose(out["img"][24, 32], (c1 + ef * c2) / (1 + ef), rtol=0, atol=1e-10)
    assert np.abs(out["img"][24, 32] - (c1 + e64 * c2) / (1 + e64)).max() > 1e-6
    same = _one(np.float32([[0, 0, z2], [0, 0, 1.0]]), [c2, c1], 0.02)
    np.testing.assert_array_equal(out["img"], same["img"])


def test_surfel_centre_lands_on_the_pixel_pcd2depth_rounds_it_to():
    """With ccx = cx and ccy = cy (integer principal point, even sizes) the ray closest to a surfel's centre is
    the one through the pixel utils/utils.py:pcd2depth rounds its projection to."""
    rng = np.random.default_rng(3)
    K = _K(f=500.0, cx=40.0, cy=30.0)
    w, h, f, ccx, ccy = rm.camera(K, 60, 80)
    assert (ccx, ccy) == (40.0, 30.0)
    n = 500
    u = rng.integers(2, 78, n) + rng.uniform(-0.4, 0.4, n)
    v = rng.integers(2, 58, n) + rng.uniform(-0.4, 0.4, n)
    Z = rng.uniform(0.5, 2.0, n)
    P = np.stack([(u - 40.0) * Z / 500.0, (v - 30.0) * Z / 500.0, Z], 1).astype(np.float32).astype(np.float64)
    X, Y, Zz = P.T
    ur = np.round(X * 500.0 / (Zz + 1e-8) + 40.0).astype(int)   # pcd2depth
    vr = np.round(Y * 500.0 / (Zz + 1e-8) + 30.0).astype(int)
    best = np.full(n, np.inf)
    arg = np.zeros((n, 2), int)
    for di in (-1, 0, 1):
        for dj in (-1, 0, 1):
            r = rm.rho(P, vr + di, ur + dj, f, ccx, ccy)
            better = r < best
            best[better] = r[better]
            arg[better] = np.stack([vr + di, ur + dj], 1)[better]
    np.testing.assert_array_equal(arg, np.stack([vr, ur], 1))
    # and a render of each surfel alone (radius 1 px at its depth) hits that pixel
    for k in range(0, n, 50):
        out = rm.render(P[k:k + 1], [[1, 1, 1]], K, 60, 80, 1.0 * P[k, 2] / 500.0)
        assert out["front"][vr[k], ur[k]] == 0


def test_conf2color_matches_matplotlib_magma():
    import matplotlib.pyplot as plt
    import torch
    from super_amd.renderer import conf2color
    rng = np.random.default_rng(1)
    x = np.concatenate([[-0.5, -1e-9, 0.0, 1 / 256, 0.5, 255 / 256, 1 - 1e-12, 1.0, 1.0 + 1e-9, 3.0],
                        rng.uniform(-0.2, 1.2, 1000), np.arange(257) / 256, np.arange(256) / 255])
    want = plt.get_cmap("magma")(x)[:, :3]
    got = conf2color(torch.from_numpy(x))
    assert got.dtype == torch.float64 and tuple(got.shape) == (len(x), 3)
    np.testing.assert_array_equal(got.numpy(), want)
    x32 = x.astype(np.float32)
    np.testing.assert_array_equal(conf2color(torch.from_numpy(x32)).numpy(), plt.get_cmap("magma")(x32)[:, :3])
    np.testing.assert_array_equal(conf2color(torch.tensor([float("nan")], dtype=torch.float64)).numpy(),
                                  plt.get_cmap("magma")(np.array([np.nan]))[:, :3])


def test_render_params_layout_matches_the_header(tmp_path):
    from super_amd import _lib
    assert C.sizeof(_lib.SlmRenderParams) == 4 * 4 + 8 * 8 + 3 * 4 + 4
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "super_lm.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %d\\n", sizeof(slm_render_params), offsetof(slm_render_params, focal), '
                   'offsetof(slm_render_params, bg), SLM_RENDER_MAX_TRACK);\n  return 0;\n}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    size, off_f, off_bg, mt = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_lib.SlmRenderParams)
    assert off_f == _lib.SlmRenderParams.focal.offset and off_bg == _lib.SlmRenderParams.bg.offset
    assert mt == _lib.SLM_RENDER_MAX_TRACK
