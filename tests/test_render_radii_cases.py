"""The facts the GPU tests of the per-point-radius renderer rely on, decided by the CPU model alone
(tests/render_radii_cases.py): the branches each scene reaches, the share of rows left out of the gradient comparisons
(at most 5 %), and the kept pixels of the GraphFit scene with the formula's radii and with the one default radius."""
import numpy as np
import pytest

import render_grad_model as rgm
import render_model as rm
import render_radii_cases as rc
import render_radii_model as rrm


@pytest.mark.parametrize("name", list(rc.SCENES))
def test_the_share_left_out_is_small_and_the_gradients_are_not_trivial(name):
    f = rc.facts(name)
    assert f["ex"].mean() <= rc.MAX_EXCLUDED, f["ex"].mean()
    assert f["want"]["near"].mean() <= 0.005
    keep = f["taken"] & ~f["ex"]
    assert keep.sum() >= 0.85 * f["taken"].sum() > 0
    for gk in f["grads"]:          # dL/dP, dL/dc, dL/dr: carried by the rows that stay in the comparison
        assert np.abs(gk[keep]).max() > 1e-3 * np.abs(gk).max() > 0
    gr = f["grads"][2]
    assert (np.abs(gr[keep]) > 1e-6 * np.abs(gr).max()).mean() > 0.3          # overlapping spheres at blending depths


def test_branches_of_the_scenes():
    s = rc.facts("link")["scene"]
    assert (s["radii"] == np.float32(rc.LINK_RAD)).all() and float(np.float32(rc.LINK_RAD)) != rc.LINK_RAD
    # mixed: under one pixel to over 40 px, splats cut by every border, bad radii culled, sizes no multiple of 16
    f = rc.facts("mixed")
    s, want = f["scene"], f["want"]
    px = 100.0 * s["radii"][:-4].astype(np.float64) / s["P"][:-4, 2]
    assert px.min() < 1.0 and px.max() > 40.0 and s["H"] % 16 and s["W"] % 16
    ids = set(f["hits"][1].tolist())
    assert set(range(2, 10)) <= ids                         # the eight centred outside reach into the image
    pixset = f["hits"][0]
    for edge in (pixset // 150 == 0, pixset // 150 == 99, pixset % 150 == 0, pixset % 150 == 149):
        assert edge.any()
    n = len(s["P"])
    assert not (ids & set(range(n - 4, n))) and not np.isin(want["front"], np.arange(n - 4, n)).any()
    assert rc.facts("mixed_half")["want"]["img"].shape == (50, 75, 3)
    # overflow: one list beyond the LDS sort's 4096 keys; the large spheres are in it and in its eight neighbours
    f = rc.facts("overflow")
    te = rc.tile_entries(f["scene"])
    assert te[(1, 1)] > 4096 and max(v for k, v in te.items() if k != (1, 1)) < 4096
    assert not f["want"]["near"].any() and not f["ex"][-6:].any() and f["taken"][-6:].all()
    w = 64
    big_tiles = {(p // w // 16, p % w // 16) for p, k in zip(f["hits"][0].tolist(), f["hits"][1].tolist())
                 if k >= len(f["scene"]["P"]) - 6}
    assert {(ty, tx) for ty in range(3) for tx in range(3)} <= big_tiles
    # cut64: the 64-hit cut falls between spheres of different radii
    f = rc.facts("cut64")
    cnt = f["want"]["count"]
    assert cnt.max() == 64 and set(np.unique(cnt)) == {0, 27, 53, 64}
    full = rrm.hit_sets(f["scene"]["P"], f["scene"]["radii"], rc.K0, 48, 64, n_track=1 << 30)
    assert np.bincount(full[0]).max() == 80
    r = f["scene"]["radii"]
    assert r[63] != r[64] and r[62] != r[63]
    # inside: Z <= r, every pixel hit by row 0
    f = rc.facts("inside")
    s = f["scene"]
    assert s["P"][0, 2] <= s["radii"][0] and (f["want"]["count"] >= 1).all() and (f["want"]["front"] == 0).mean() > 0.5
    assert f["want"]["count"].max() >= 3


def test_graphfit_scene_keeps_pixels_only_with_the_surfels_own_radii():
    import torch
    sc, stable, cols, radii, tgt = rc.graphfit_scene()
    assert 0 < (~stable).sum() < 0.1 * sc.N
    np.testing.assert_array_equal(radii, sc.sf_points[:, 2] / (np.sqrt(2.0) * sc.K[0, 0] *
                                                                 np.clip(np.abs(sc.sf_norms[:, 2]), 0.26, 1.0)))
    P = sc.sf_points[stable]
    own = rrm.render(P, cols[stable], radii[stable], sc.K, sc.H, sc.W)
    one = rm.render(P, cols[stable], sc.K, sc.H, sc.W, rc.GF_UNIFORM_RAD)
    t = torch.from_numpy(tgt).double()
    kept_own = rgm.ssim_loss(torch.from_numpy(own["img"]).float().double(), t, rc.GF_WEIGHT)[1]
    kept_one = rgm.ssim_loss(torch.from_numpy(one["img"]).float().double(), t, rc.GF_WEIGHT)[1]
    assert kept_own > 100 and kept_one == 0
    assert (own["count"] > 0).mean() > 0.9 and own["count"].max() <= 8          # closed, a few hits per pixel
