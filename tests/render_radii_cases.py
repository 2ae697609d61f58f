"""Input builders for the per-point-radius renderer tests (test_gpu_render_radii.py, test_gpu_render_radii_autograd.py,
test_gpu_graphfit_render_radii.py) and the facts about them that the CPU model alone decides
(test_render_radii_cases.py checks those without a GPU): the branches each scene reaches, the share of rows left out
of a gradient comparison because a decision of theirs sits at its threshold (at most 5 %), the kept pixels of the
GraphFit scene.  Everything is built from seeds; nothing here reads a kernel's output.

A scene is a dict(P (N,3), cols (N,3) float32, radii (N,) float32, K, H, W, view_scale, n_track)."""
import functools

import numpy as np

import render_model as rm
import render_radii_model as rrm

K0 = np.array([[100.0, 0, 32.0], [0, 100.0, 24.0], [0, 0, 1]])        # 48 x 64
K_BIG = np.array([[100.0, 0, 75.0], [0, 100.0, 50.0], [0, 0, 1]])     # 100 x 150
MAX_EXCLUDED = 0.05
BAD_RADII = (0.0, -1e-3, np.nan, np.inf)
LINK_RAD = 0.01       # the filled render of the 60 x 80 scene (test_gpu_render_grad.py); float32(0.01) != 0.01


def _scene(P, cols, radii, K, H, W, view_scale=1.0, n_track=rm.N_TRACK):
    return dict(P=np.asarray(P, np.float64), cols=np.asarray(cols, np.float32), radii=np.asarray(radii, np.float32), K=K, H=H,
                W=W, view_scale=view_scale, n_track=n_track)


def link():
    """the pinned 60 x 80 scene of test_gpu_render_grad.py with every radius float32(0.01)"""
    from super_amd import synth
    sc = synth.make_scene(N=3000, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    cols = np.random.default_rng(12).uniform(size=(sc.N, 3)).astype(np.float32)
    return _scene(sc.sf_points, cols, np.full(sc.N, LINK_RAD, np.float32), sc.K, sc.H, sc.W)


# Depths: with gamma = 1e-5 a sphere 1e-3 m behind another has e^-7 of its weight, so a scene whose gradients are to say
# anything keeps the spheres that overlap within a few 1e-4 m of depth (surfels of one surface are like that).


def mixed(view_scale=1.0, seed=3):
    """silhouettes from 0.6 px to 45 px radius on a 100 x 150 image (neither a multiple of 16: seven by ten tiles, the last
    ones cut), all within 4e-4 m of depth: 300 of 0.6 .. 4 px, 20 of 4 .. 12 px, and ten large ones first: two of 41 .. 45 px
    inside and eight of 15 .. 25 px centred beyond the borders, two per side (cut by every border).  Few are large
    because a large rim crosses a threshold pixel of its own more often than not.  Four more rows carry the radii 0,
    negative, NaN and inf over the image centre, in front of everything."""
    rng = np.random.default_rng(seed)
    H, W = 100, 150
    px = np.concatenate([rng.uniform(41.0, 45.0, 2), rng.uniform(15.0, 25.0, 8), rng.uniform(4.0, 12.0, 20),
                         np.exp(rng.uniform(np.log(0.6), np.log(4.0), 300))])
    n = len(px)
    Z = 1.0 + rng.uniform(0.0, 4e-4, n)
    u, v = rng.uniform(-5.0, W + 5.0, n), rng.uniform(-5.0, H + 5.0, n)
    u[2:10] = [-12.0, -14.0, W + 10.0, W + 13.0, 40.0, 100.0, 30.0, 120.0]
    v[2:10] = [30.0, 70.0, 20.0, 80.0, -12.0, -8.0, H + 8.0, H + 12.0]
    P = np.stack([(u - 75.0) * Z / 100.0, (v - 50.0) * Z / 100.0, Z], 1)
    radii = px * Z / 100.0
    bad = np.tile(np.array([[0.0, 0.0, 0.9]]), (len(BAD_RADII), 1))
    P, radii = np.concatenate([P, bad]), np.concatenate([radii, BAD_RADII])
    return _scene(P, rng.uniform(size=(len(P), 3)), radii, K_BIG, H, W, view_scale)


def overflow(seed=4):
    """tile (1,1) of a 48 x 64 image holds 5600 spheres of 0.4 .. 0.9 px radius (those that cover a pixel centre are more
    than the 4096 keys of the LDS sort); each of the eight tiles around it holds 40 of the same kind; six spheres of
    12 .. 22 px radius, centred in tile (1,1) and up to 1e-4 m in front of the rest (they blend with it), enter the lists
    of all nine tiles.

    The seed is hand-picked: of the seeds 0 .. 13 it is the only one at which the model marks no pixel `near`; at the
    others one to nine `near` pixels in the dense tile leave out 2.7 .. 11.5 % of the rows, the six large spheres (whose
    boxes hold every pixel of that tile) always among them.  test_render_radii_cases.py asserts the facts relied on (no
    `near` pixel, the large spheres compared), so a change of the model's `near` rule or of this builder that breaks
    them shows there, on the CPU, and the remedy is another seed, not a wider share."""
    rng = np.random.default_rng(seed)
    H, W = 48, 64
    parts = []
    for ty in range(3):
        for tx in range(3):
            m = 5600 if (ty, tx) == (1, 1) else 40
            parts.append(np.stack([rng.uniform(16.0 * tx + 1.0, 16.0 * tx + 15.0, m),
                                   rng.uniform(16.0 * ty + 1.0, 16.0 * ty + 15.0, m)], 1))
    uv = np.concatenate(parts)
    uv = uv[rng.permutation(len(uv))]
    Z = 1.0 + rng.uniform(0.0, 3e-4, len(uv))
    px = rng.uniform(0.4, 0.9, len(uv))
    big = 6
    uv = np.concatenate([uv, np.stack([rng.uniform(18.0, 30.0, big), rng.uniform(18.0, 30.0, big)], 1)])
    Z = np.concatenate([Z, 1.0 - rng.uniform(0.0, 1e-4, big)])
    px = np.concatenate([px, rng.uniform(12.0, 22.0, big)])
    P = np.stack([(uv[:, 0] - 32.0) * Z / 100.0, (uv[:, 1] - 24.0) * Z / 100.0, Z], 1)
    return _scene(P, rng.uniform(size=(len(P), 3)), px * Z / 100.0, K0, H, W)


def cut64(n=80):
    """80 spheres on one line of sight, 2e-6 m apart (17 float32 steps; the 64th still has e^-0.85 of the first's weight),
    radii cycling through 1.5, 4 and 2.5 px: the centre pixels have 80 hits and are cut at 64 between spheres of
    different radii; pixels further out see the wider ones only (53 and 27 hits, no cut)."""
    Z = 1.0 + 2e-6 * np.arange(n)
    P = np.stack([0.0031 * Z, -0.0022 * Z, Z], 1)         # the same line of sight: a third of a pixel off a pixel centre
    px = np.array([1.5, 4.0, 2.5])[np.arange(n) % 3]
    cols = np.random.default_rng(7).uniform(size=(n, 3))
    return _scene(P, cols, px * Z / 100.0, K0, 48, 64)


def inside():
    """a sphere that holds the camera centre (|P| < r, so Z <= r: the whole-image candidate branch, hit by every pixel) and
    twelve ordinary ones of 2 .. 6 px within 2e-4 m of its depth"""
    rng = np.random.default_rng(5)
    n = 12
    Z = 0.05 + rng.uniform(-1e-4, 1e-4, n)
    u, v = rng.uniform(4.0, 60.0, n), rng.uniform(4.0, 44.0, n)
    P = np.stack([(u - 32.0) * Z / 100.0, (v - 24.0) * Z / 100.0, Z], 1)
    P = np.concatenate([[[0.004, -0.003, 0.05]], P])
    radii = np.concatenate([[0.06], rng.uniform(2.0, 6.0, n) * Z / 100.0])
    return _scene(P, rng.uniform(size=(n + 1, 3)), radii, K0, 48, 64)


SCENES = {"link": link, "mixed": mixed, "mixed_half": functools.partial(mixed, view_scale=0.5), "overflow": overflow,
          "cut64": cut64, "inside": inside}


@functools.lru_cache(maxsize=None)
def facts(name):
    """What the model says about a scene, computed once and shared (treat as read-only) -> dict(scene, want: the model's
    render, hits, g: a dL/dimage, grads: the model's (dL/dP, dL/dc, dL/dr) for it, ex: rows left out of a gradient comparison,
    taken: rows among the hits)."""
    s = SCENES[name]()
    geo = (s["K"], s["H"], s["W"], s["view_scale"])
    want = rrm.render(s["P"], s["cols"], s["radii"], *geo, bg=(0.1, 0.2, 0.3), n_track=s["n_track"])
    hits = rrm.hit_sets(s["P"], s["radii"], *geo, n_track=s["n_track"])
    h, w = want["near"].shape
    g = np.random.default_rng(len(s["P"])).normal(size=(h, w, 3))
    grads = rrm.grads(s["P"], s["cols"], s["radii"], g, hits, *geo, bg=(0.1, 0.2, 0.3))
    ex = rrm.excluded(s["P"], s["radii"], s["K"], s["H"], s["W"], want["near"], s["view_scale"])
    taken = np.zeros(len(s["P"]), bool)
    taken[hits[1]] = True
    return dict(scene=s, want=want, hits=hits, g=g, grads=grads, ex=ex, taken=taken)


def tile_entries(s):
    """{(ty, tx): number of rows whose (model) candidate box touches the 16 x 16 tile}: what the kernel's lists hold, up to
    the padding of the boxes"""
    P = s["P"].astype(np.float32).astype(np.float64)
    R, ok = rrm.radii32(s["radii"])
    w, h, f, ccx, ccy = rm.camera(s["K"], s["H"], s["W"], s["view_scale"])
    Rs = np.where(ok, R, 1.0)
    x0, x1 = rm._range(P[:, 0], P[:, 2], Rs, f, ccx, w, 0.0)
    y0, y1 = rm._range(P[:, 1], P[:, 2], Rs, f, ccy, h, 0.0)
    live = ok & (P[:, 2] >= rm.Z_NEAR) & (P[:, 2] <= rm.Z_FAR) & (x0 <= x1) & (y0 <= y1)
    out = {}
    for k in np.nonzero(live)[0]:
        for ty in range(y0[k] // 16, y1[k] // 16 + 1):
            for tx in range(x0[k] // 16, x1[k] // 16 + 1):
                out[(ty, tx)] = out.get((ty, tx), 0) + 1
    return out


# ---- the GraphFit scene: radii of the reference's formula ----------------------------------------------------------------

GF_WEIGHT = 0.01
GF_UNIFORM_RAD = 2e-4      # opt.renderer_rad's default: keeps no pixel


def formula_radii(P, norms, fx):
    """the reference's surfel radius (utils/data_loader.py:467-468): Z / (sqrt(2) fx clamp(|n_z|, 0.26, 1))"""
    nz = np.clip(np.abs(np.asarray(norms, np.float64)[:, 2]), 0.26, 1.0)
    return np.asarray(P, np.float64)[:, 2] / (np.sqrt(2.0) * fx * nz)


@functools.lru_cache(maxsize=None)
def graphfit_scene():
    """-> (sc, stable, cols, radii float64 (N,), tgt (3,H,W) float32): a 60 x 80 scene like that of
    test_gpu_graphfit_render_loss.py, with a surfel on nearly every interior pixel (the formula's radii, 0.64 .. 0.96 px
    here, close the image only then) and 3 % unstable rows; the colour frame is the model's per-point render of the
    surfels moved by a few pixels, plus noise."""
    from super_amd import synth
    sc = synth.make_scene(N=4400, J=48, H=60, W=80, seed=31, src_border=1, tgt_border=3)
    rng = np.random.default_rng(12)
    stable = rng.uniform(size=sc.N) > 0.03
    cols = rng.uniform(size=(sc.N, 3)).astype(np.float32)
    radii = formula_radii(sc.sf_points, sc.sf_norms, sc.K[0, 0])
    tg = rrm.render(sc.sf_points[stable] + np.array([0.004, -0.002, 0.0]), cols[stable], radii[stable], sc.K, sc.H, sc.W)["img"]
    tgt = (np.transpose(tg, (2, 0, 1)) + 0.01 * np.random.default_rng(5).normal(size=(3, sc.H, sc.W))).astype(np.float32)
    return sc, stable, cols, radii, tgt
