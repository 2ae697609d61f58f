"""Input builders for the render-loss tests at edge shapes and at the driver's size (test_gpu_render_loss_shapes.py), and the
facts about them that the CPU models alone decide (test_render_loss_cases.py checks those without a GPU): which SSIM
branches an image / target pair reaches, how many pixels of a hand-built scene sit at a threshold.  Everything is built
from seeds; nothing here reads a kernel's output."""
import numpy as np

import render_grad_model as rgm
import render_model as rm

SSIM_SHAPES = [(6, 6), (6, 23), (10, 17), (11, 16), (15, 15), (16, 16), (17, 33), (33, 47), (60, 81), (240, 320),
               (480, 640), (481, 643)]
# (h, w, holes): at 6x6 every clipped window is the whole image, so one hole masks every pixel; that shape also runs
# without holes so that its gradient is not all zero
SSIM_CASES = [(h, w, True) for h, w in SSIM_SHAPES] + [(6, 6, False)]
SSIM_WEIGHT = 0.37
R = 5                # the window's radius


def ssim_holes(h, w):
    """[(i0, i1, j0, j1, channel or None)]: zero-valued boxes [i0,i1) x [j0,j1) of the image: one pixel in a corner, one
    on the opposite border, and from 33x33 on single pixels and blocks inside, near and on the borders (one of them
    in one channel only: the mask takes the minimum over the channels)."""
    holes = [(0, 1, 0, 1, None)]
    if max(h, w) >= 15:
        holes.append((h - 1, h, w - 1, w, 1))
    if h >= 33 and w >= 33:
        holes += [(h // 2, h // 2 + 3, w // 2, w // 2 + 4, None),          # a block inside
                  (h // 3, h // 3 + 1, 2 * w // 3, 2 * w // 3 + 1, 2),     # one pixel, one channel
                  (2, 3, w // 2, w // 2 + 1, None),                        # 2 from the top border
                  (h // 2 + 8, h // 2 + 10, w - 2, w, None)]               # a block on the right border
    return holes


def ssim_inputs(h, w, holes=True):
    """-> (image (h,w,3) float32 in [0.05, 1] with zero holes, target (3,h,w) float32).  The target is the image plus 5 %
    noise (those pixels are kept) except in a band of columns, where it is the inverted image (m well above 0.1)."""
    rng = np.random.default_rng(1000 * h + w)
    img = rng.uniform(0.05, 1.0, size=(h, w, 3)).astype(np.float32)
    if holes:
        for i0, i1, j0, j1, c in ssim_holes(h, w):
            img[i0:i1, j0:j1, slice(None) if c is None else c] = 0.0
    x = np.transpose(img, (2, 0, 1)).astype(np.float64)
    tgt = x + 0.05 * rng.normal(size=x.shape)
    j0 = w - 2 if w < 15 else w // 2 - 1
    j1 = min(j0 + max(w // 4, 8), w)
    tgt[:, :, j0:j1] = 1.0 - x[:, :, j0:j1]
    return img, tgt.astype(np.float32)


def ssim_model(img, tgt, weight=SSIM_WEIGHT):
    """rgm.ssim_loss + autograd on the float32 inputs -> dict(loss, kept, grad (h,w,3), m (h,w), v (3,h,w), valid (h,w))"""
    import torch
    x = torch.from_numpy(img).double().requires_grad_(True)
    t = torch.from_numpy(tgt).double()
    loss, kept, m, v = rgm.ssim_loss(x, t, weight)
    loss.backward()
    valid = rgm.ssim_parts(x.detach(), t)[1][0, 0].numpy()
    return dict(loss=float(loss.detach()), kept=kept, grad=x.grad.numpy(), m=m.numpy(), v=v.numpy(), valid=valid)


def ssim_branches(img, mod):
    """Which branches of the loss the pair reaches, from the image and the model's outputs alone -> dict of counts:
    kept / masked / deselected (valid, m >= 0.1) pixels; `clipped`: masked pixels closer than 5 to a border whose window
    holds holes only in that border's strip of 5 (the part of the window that the reflection repeats and the mask's
    pool clips); `valid_at_border`: valid pixels closer than 5 to a border (a clipped window without a hole)."""
    h, w = img.shape[:2]
    hole = img.min(2) <= 0
    valid, m = mod["valid"], mod["m"]
    ii, jj = np.mgrid[0:h, 0:w]
    border = (ii < R) | (ii >= h - R) | (jj < R) | (jj >= w - R)
    strip = np.zeros((h, w), bool)
    strip[:R], strip[h - R:], strip[:, :R], strip[:, w - R:] = True, True, True, True
    inner = hole & ~strip
    clipped = 0
    for i, j in zip(*np.nonzero(~valid & border)):
        clipped += not inner[max(i - R, 0):i + R + 1, max(j - R, 0):j + R + 1].any()
    return dict(kept=int((valid & (m < 0.1)).sum()), masked=int((~valid).sum()), deselected=int((valid & (m >= 0.1)).sum()),
                clipped=int(clipped), valid_at_border=int((valid & border).sum()),
                m_margin=float(np.abs(m - 0.1)[valid].min()) if valid.any() else np.inf,
                clamp_margin=float(np.minimum(np.abs(mod["v"]), np.abs(mod["v"] - 1))[:, valid].min()) if valid.any() else np.inf)


def assert_ssim_branches(h, w, holes, img, mod):
    """the conditions on an SSIM case, decided by the model alone (the GPU test repeats them before it compares)"""
    b = ssim_branches(img, mod)
    assert b["kept"] == mod["kept"]
    assert b["m_margin"] > 1e-6 and b["clamp_margin"] > 1e-6, b       # no decision at its threshold
    if holes:
        assert b["masked"] > 0 and b["clipped"] > 0, b
        assert len(ssim_holes(h, w)) == (1 if max(h, w) < 15 else 2 if min(h, w) < 33 else 6)
    else:
        assert b["masked"] == 0, b
    if holes and max(h, w) <= 2 * R + 1:      # every clipped window reaches the corner hole: nothing is valid
        assert b["kept"] == b["deselected"] == 0 and b["masked"] == h * w, b
    else:
        assert 0 < b["kept"] < h * w and b["deselected"] > 0 and b["valid_at_border"] > 0, b
    return b


def ssim_loss_only(img64, tgt64, weight=SSIM_WEIGHT):
    """the model's loss as a plain float function of float64 arrays (finite differences)"""
    import torch
    return float(rgm.ssim_loss(torch.from_numpy(img64), torch.from_numpy(tgt64), weight)[0])


# ---- hand-built scenes for the renderer backward ----------------------------------------------------------------------

K0 = np.array([[100.0, 0, 32.0], [0, 100.0, 24.0], [0, 0, 1]])        # 48 x 64, as test_gpu_render_grad.py
K_BIG = np.array([[100.0, 0, 75.0], [0, 100.0, 50.0], [0, 0, 1]])     # 100 x 150


def big_splats(seed=4, n=120):
    """-> (P, cols, K, H, W, rad): surfels at 0.05..0.15 m with rad = 0.03 m: silhouettes of 20..60 px radius (boxes
    40..120 px wide, three to eight tiles per axis) on a 100 x 150 image (neither a multiple of 16); the first eight are
    centred outside the image, two beyond each side, the rest anywhere up to 30 px outside.  One radius serves every
    surfel, so the depth range is the one that gives those widths at f = 100."""
    rng = np.random.default_rng(seed)
    H, W, rad = 100, 150, 0.03
    Z = 100.0 * rad / rng.uniform(20.0, 60.0, n)
    u, v = rng.uniform(-30.0, W + 30.0, n), rng.uniform(-30.0, H + 30.0, n)
    u[:8] = [-12.0, -25.0, W + 10.0, W + 22.0, 40.0, 100.0, 30.0, 120.0]
    v[:8] = [30.0, 70.0, 20.0, 80.0, -15.0, -8.0, H + 12.0, H + 20.0]
    P = np.stack([(u - 75.0) * Z / 100.0, (v - 50.0) * Z / 100.0, Z], 1)
    return P, rng.uniform(size=(n, 3)).astype(np.float32), K_BIG, H, W, rad


def overflow_with_neighbours(seed=0):
    """-> (P, cols, K, H, W, rad): 6500 surfels centred in tile (1,1) of a 48 x 64 image with silhouettes of 2..3 px
    radius, so those near the tile's four borders also enter the neighbours' lists (and the neighbours' surfels enter
    its list, which overflows RN_SORT_CAP = 4096); 300 in each of the eight surrounding tiles.  A second tile of thousands
    would put more than 1 % of the pixels at a threshold (every pixel with 64 hits adds its share)."""
    rng = np.random.default_rng(seed)
    H, W, rad = 48, 64, 0.03
    parts = []
    for ty in range(3):
        for tx in range(3):
            n = 6500 if (ty, tx) == (1, 1) else 300
            parts.append(np.stack([rng.uniform(16.0 * tx, 16.0 * tx + 16.0, n), rng.uniform(16.0 * ty, 16.0 * ty + 16.0, n)], 1))
    uv = np.concatenate(parts)
    uv = uv[rng.permutation(len(uv))]
    Z = rng.uniform(1.0, 1.5, len(uv))
    P = np.stack([(uv[:, 0] - 32.0) * Z / 100.0, (uv[:, 1] - 24.0) * Z / 100.0, Z], 1)
    return P, rng.uniform(size=(len(P), 3)).astype(np.float32), K0, H, W, rad


OVERFLOW_MAX_LOST = 0.01      # share of the taken surfels whose every taken hit is a `near` pixel (see hand_scene_facts)


def tile_lists(P, K, H, W, rad):
    """-> {(ty, tx): set of surfel ids}: the tiles of 16 x 16 pixels in which each surfel has a hit (model's hit list,
    before the n_track cut): a lower bound of the kernel's per-tile lists, which hold every box that touches the tile."""
    pix, ids, _ = rgm.hit_sets_fast(P, K, H, W, rad, n_track=1 << 30)
    w = rm.camera(K, H, W)[0]
    out = {}
    for t, k in set(zip(((pix // w) // 16 * 1000 + (pix % w) // 16).tolist(), ids.tolist())):
        out.setdefault((t // 1000, t % 1000), set()).add(k)
    return out


TIE_FRONT, TIE_BEHIND = (3, 40), (0, 20, 74)        # rows of the surfels in front of and behind the 70 coincident ones


def ties(n_tie=70):
    """-> (P, cols, K, H, W, rad): 70 coincident surfels (equal keys but for the row), two surfels 1e-4 m in front (0.67
    gamma in zt: a real blend) and three behind, shifted sideways so that some pixels see the tie group alone; the rows
    are interleaved, the order inside the tie group is by row."""
    n = n_tie + len(TIE_FRONT) + len(TIE_BEHIND)
    P = np.tile(np.array([[0.0031, -0.0022, 1.0]]), (n, 1))
    P[list(TIE_FRONT)] = [[0.0131, -0.0022, 0.9999], [-0.0069, 0.0078, 0.9999]]
    P[list(TIE_BEHIND)] = [[0.0031, 0.0108, 1.0001], [-0.0099, -0.0022, 1.0001], [0.0081, -0.0082, 1.0002]]
    cols = np.random.default_rng(7).uniform(size=(n, 3)).astype(np.float32)
    return P, cols, K0, 48, 64, 0.02


def hand_scene_facts(P, cols, K, H, W, rad, n_track=rm.N_TRACK, view_scale=1.0, max_lost=0.0):
    """What the models say about a hand-built scene -> dict(near (h,w) bool, near_share, hits, count (h*w,), taken (N,)
    bool: the surfel is among the first n_track hits of a pixel that is not `near`, `lost`: surfels whose taken hits
    are all in `near` pixels).  Asserts the cap: at most 1 % of the pixels are `near`, and leaving them out takes no
    surfel out of the comparison -- up to ``max_lost`` of the surfels that are taken anywhere, for a scene of thousands of
    surfels a few pixels wide: there a surfel whose only taken hit is the rim pixel that it makes `near` itself is
    bound to occur, and it has no gradient that does not hang on that threshold."""
    near = rm.render(P, cols, K, H, W, rad, view_scale, n_track=n_track)["near"]
    hits = rgm.hit_sets_fast(P, K, H, W, rad, view_scale, n_track)
    pix, ids, _ = hits
    taken = np.zeros(len(P), bool)
    taken[ids[~near.ravel()[pix]]] = True
    everywhere = np.zeros(len(P), bool)
    everywhere[ids] = True
    assert near.mean() <= 0.01, near.mean()
    lost = int((everywhere & ~taken).sum())
    assert lost <= max_lost * everywhere.sum(), (lost, int(everywhere.sum()))
    return dict(near=near, near_share=float(near.mean()), hits=hits, lost=lost, count=np.bincount(pix, minlength=near.size), taken=taken)


def masked_grad(near, seed=0):
    """dL/dimage for a hand-built scene: float32-representable normal values, zero on the model's `near` pixels (the
    kernel skips a pixel whose gradient is zero and the model's sum loses the same terms)"""
    h, w = near.shape
    g = np.random.default_rng(seed).normal(size=(h, w, 3)).astype(np.float32).astype(np.float64)
    g[near] = 0.0
    return g


def model_grads(P, cols, g, hits, K, H, W, rad, view_scale=1.0, bg=(0.0, 0.0, 0.0)):
    """(dL/dpoints, dL/dcolors) of L = sum(image * g) at the given hit sets: render_color_grad_model.grads with the hit
    sets passed in (its point half is render_grad_model.blend's, see test_render_color_grad_model.py)"""
    import torch
    import render_color_grad_model as rcm
    Pt = torch.from_numpy(np.asarray(P, np.float64)).requires_grad_(True)
    Ct = torch.from_numpy(np.asarray(cols, np.float64)).requires_grad_(True)
    img = rcm.blend(Pt, Ct, hits, K, H, W, rad, view_scale, bg)
    (img * torch.from_numpy(g)).sum().backward()
    z = np.zeros((len(Pt), 3))
    return (z if Pt.grad is None else Pt.grad.numpy()), Ct.grad.numpy()
