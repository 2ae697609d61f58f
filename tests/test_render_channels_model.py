"""tests/render_channels_model.py, the float64 model of the N-channel render, pinned without a GPU: at C = 3 it is
render_radii_model (images exactly, gradients to 1e-12), a channel of a C-channel render is the render of that column
alone, and its feature gradient is the derivative of its blend (central differences)."""
import numpy as np
import pytest

import render_channels_model as rcm
import render_radii_cases as rc
import render_radii_model as rrm

BG3 = (0.1, 0.2, 0.3)


def _geo(s):
    return s["K"], s["H"], s["W"], s["view_scale"]


@pytest.mark.parametrize("name", ["mixed", "cut64", "inside"])
def test_three_channels_are_the_radii_model(name):
    f = rc.facts(name)
    s = f["scene"]
    got = rcm.render(s["P"], s["cols"], s["radii"], *_geo(s), bg=BG3, n_track=s["n_track"])
    for k in ("img", "front", "count", "near"):
        np.testing.assert_array_equal(got[k], f["want"][k], err_msg=k)
    grads = rcm.grads(s["P"], s["cols"], s["radii"], f["g"], f["hits"], *_geo(s), bg=BG3)
    for a, b, what in zip(grads, f["grads"], ("dL/dP", "dL/df", "dL/dr")):
        assert np.abs(b).max() > 0
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-12 * np.abs(b).max(), err_msg=what)


def test_one_radius_is_the_one_radius_model():
    import render_model as rm
    s = rc.facts("link")["scene"]
    got = rcm.render(s["P"], s["cols"], None, *_geo(s), bg=BG3, radius=2e-3)
    want = rm.render(s["P"], s["cols"], s["K"], s["H"], s["W"], rad=2e-3, bg=BG3)
    assert (want["count"] > 0).any()                 # this radius covers pixels (2e-4 covers none)
    for k in ("img", "front", "count", "near"):
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)


@pytest.mark.parametrize("C", [1, 5, 8])
def test_a_channel_is_the_render_of_its_column(C):
    s = rc.facts("mixed")["scene"]
    rng = np.random.default_rng(C)
    feat = rng.uniform(size=(len(s["P"]), C)).astype(np.float32)
    bg = 0.1 + 0.1 * np.arange(C)
    all_ = rcm.render(s["P"], feat, s["radii"], *_geo(s), bg=bg)
    assert all_["img"].shape == (100, 150, C)
    for c in range(C):
        one = rcm.render(s["P"], feat[:, c:c + 1], s["radii"], *_geo(s), bg=bg[c:c + 1])
        np.testing.assert_array_equal(all_["img"][..., c], one["img"][..., 0])
        np.testing.assert_array_equal(all_["front"], one["front"])
    # and the torch blend at the hit sets is the numpy render
    hits = rc.facts("mixed")["hits"]
    import torch
    img = rcm.blend(torch.from_numpy(s["P"]), torch.from_numpy(feat).double(), torch.from_numpy(s["radii"]).double(), hits,
                    *_geo(s), bg=bg).numpy()
    np.testing.assert_allclose(img, all_["img"], rtol=0, atol=1e-12)


def test_feature_gradient_matches_finite_differences():
    import torch
    f = rc.facts("cut64")                       # 48 x 64
    s = f["scene"]
    C, n = 5, len(s["P"])
    rng = np.random.default_rng(11)
    feat = rng.uniform(size=(n, C)).astype(np.float32).astype(np.float64)
    bg = 0.1 + 0.1 * np.arange(C)
    g = rng.normal(size=(48, 64, C))
    gf = rcm.grads(s["P"], feat, s["radii"], g, f["hits"], *_geo(s), bg=bg)[1]
    assert gf.shape == (n, C) and np.abs(gf).max() > 0
    P, R, gt = torch.from_numpy(s["P"]), torch.from_numpy(s["radii"]).double(), torch.from_numpy(g)

    def loss(ft):
        # the blend rounds its features to float32; the differences below step by float32-exact amounts from float32 values
        return float((rcm.blend(P, torch.from_numpy(ft), R, f["hits"], *_geo(s), bg=bg) * gt).sum())

    taken = np.nonzero(f["taken"])[0]
    step = 2.0 ** -7
    for _ in range(20):
        k, c = int(rng.choice(taken)), int(rng.integers(C))
        base = np.float64(np.float32(feat[k, c] * 0.5 + 0.25))      # room for the step inside float32-exact values
        a, b = feat.copy(), feat.copy()
        a[k, c], b[k, c] = base + step, base - step
        fd = (loss(a) - loss(b)) / (2 * step)                      # the blend is linear in a feature: exact up to rounding
        assert abs(fd - gf[k, c]) <= 1e-6 * max(abs(gf[k, c]), np.abs(gf).max() * 1e-3), (k, c, fd, gf[k, c])
