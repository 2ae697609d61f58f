"""Scenes of the surfel-fusion edge tests: pure NumPy, no GPU, no torch.  test_fusion_edge_cases.py pins them on the CPU (the
oracle reproduces the reference's recording tests/golden/fu_edges.npz, every scene exercises what it claims, no decision
sits on a knife edge); test_gpu_fusion_edges.py runs them through super_amd.fusion on the device.

Every scene is a 16 x 24 image (16 x 32 for ``pow2``: 512 pixels, a power of two for the sort's end bit) seen by a camera with
fx = fy = 20, depth near 1, th_dist = 0.015, and holds

* pixel A: 40 stable surfels on one pixel, 0.03 apart in depth (none merge): 24 fall off the 16 layer maps;
* pixel B: 20 surfels 0.002 apart: chains of pairwise merges in which the surviving surfel moves;
* pixel C with exactly 16 and pixel D with exactly 17 surfels, 0.04 apart: the boundary of the layer maps itself;
* one surfel on about half of the other pixels (most new points merge into layer 0), surfels that round to the pixel just
  outside each border and to the last one inside, a few per cent unstable surfels, time stamps on both sides of
  th_time_steps;
* a new frame whose points mostly merge, partly miss the distance test (appended) and partly lie farther from every node than
  its radius (rejected);
* ED nodes on a gx x gy grid over the image in SHUFFLED index order (``knn_ties``: ``make_tie_nodes``, compact runs that
  share a column of nodes at bit-identical positions).

Only +, -, *, / and sqrt are applied to the generator's uniform numbers, so the arrays are the same bits on every machine;
``digest`` is recorded in the golden file in place of the inputs (the recorded outputs alone fill most of the size a
committed file may have)."""
import hashlib

import numpy as np

H = 16
FX = 20.0
CY = 8.0
TH_DIST = 0.015
TIME = 41
NUM_CLASSES = 3
PIX = {"A": (5, 4), "B": (15, 9), "C": (9, 11), "D": (19, 3)}          # (u, v)
GROUP = {"A": (40, 0.03, 0.25), "B": (20, 0.002, 0.04), "C": (16, 0.04, 0.25), "D": (17, 0.04, 0.25)}   # count, depth step, jitter (pixels)

_SEM = dict(method="semantic-super", num_classes=NUM_CLASSES)
# name -> K, node grid (gx, gy), option overrides, flags
CASES = {
    "k1": dict(K=1), "k2": dict(K=2), "k3": dict(K=3), "k5": dict(K=5), "k7": dict(K=7), "k8": dict(K=8),
    "k4_j70": dict(K=4, grid=(10, 7)), "k5_j65": dict(K=5, grid=(13, 5)), "k8_j129": dict(K=8, grid=(43, 3)),
    "k8_j8": dict(K=8, grid=(4, 2)), "k4_j4": dict(K=4, grid=(2, 2)),
    "nomerge_exist": dict(K=4, okw=dict(disable_merging_exist_surfels=True)),
    "nomerge_new": dict(K=4, okw=dict(disable_merging_new_surfels=True)),
    "noadd": dict(K=4, okw=dict(disable_adding_new_surfels=True)),
    "pow2": dict(K=4, W=32),
    "sem_k3": dict(K=3, seg=True, okw=dict(_SEM)),
    "hard_k3": dict(K=3, seg=True, okw=dict(_SEM, hard_seg=True)),
    "hard_k4_j70": dict(K=4, grid=(10, 7), seg=True, okw=dict(_SEM, hard_seg=True)),
    "v1seg_k5": dict(K=5, seg=True, okw=dict(data="superv1", num_classes=NUM_CLASSES)),
    "track": dict(K=4, track=True),
    "train": dict(K=4, okw=dict(phase="train")),
}
RECORDED = tuple(CASES)                     # in tests/golden/fu_edges.npz, from the reference itself
MULTI_RUN = ("k4_j70", "k5_j65", "k8_j129", "hard_k4_j70")
# the reference does not pin these (torch.sort(descending=True) is not stable; knn_points' order among equal distances is
# the stub's): the oracle's documented "lower index first" is the project's convention
ORACLE_ONLY = {
    "ties": dict(K=4, ties=True),
    "knn_ties": dict(K=4, knn_ties=True),
    "knn_ties_k6": dict(K=6, knn_ties=True),
}
# frames carried from one fuse + swap into the next (the oracle carries its own state, the device its own)
CARRIED = {
    "carry_k4": dict(K=4), "carry_k7": dict(K=7), "carry_sem_k4": dict(K=4, seg=True, okw=dict(_SEM)),
    "carry_sem_k7": dict(K=7, seg=True, okw=dict(_SEM)),
}
DEGENERATE = ("empty_model", "empty_frame", "none_project", "all_dropped")
SEEDS = {}                                   # case -> seed, where the default (3) put a decision on a knife edge

MODEL_FIELDS = ("sf_points", "sf_norms", "sf_colors", "sf_radii", "sf_confs", "sf_time_stamp", "sf_isStable", "sf_knn_idx",
                "sf_knn_w")
SEG_FIELDS = ("sf_seg", "sf_seg_conf", "sf_dist2edge")


def _uni(rng, lo, hi, size=None):
    return lo + (hi - lo) * rng.random(size)


def surface(u, v, W):
    """Depth of the scene's surface at pixel (u, v): a low polynomial."""
    a, c = (u - W / 2) / (W / 2), (v - CY) / CY
    return 1.0 + 0.04 * a * a - 0.03 * a * c


def backproject(u, v, z, W):
    return np.stack([(u - W / 2) / FX * z, (v - CY) / FX * z, z], -1)


def _unit(x):
    return x / np.sqrt((x * x).sum(-1, keepdims=True))


def _normals(rng, n, spread=0.2):
    return _unit(np.stack([_uni(rng, -spread, spread, n), _uni(rng, -spread, spread, n), -np.ones(n)], 1))


def _knn(points, nodes, k):
    d2 = ((points[:, None, :] - nodes[None, :, :]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
    return np.sqrt(np.take_along_axis(d2, idx, 1)), idx


def _class_conf(rng, u, W, noise=1.3):
    """Class confidences of points at image column u: three vertical bands, noisy enough that some points change class."""
    band = np.clip((np.asarray(u) * NUM_CLASSES / W).astype(np.int64), 0, NUM_CLASSES - 1)
    c = noise * rng.random((len(band), NUM_CLASSES))
    c[np.arange(len(band)), band] += 1.0
    return c / c.sum(1, keepdims=True)


def _grid_nodes(rng, W, u, v):
    U, V = np.meshgrid(np.asarray(u, np.float64), np.asarray(v, np.float64), indexing="xy")
    U, V = U.reshape(-1), V.reshape(-1)
    n = len(U)
    U = U + _uni(rng, -0.3, 0.3, n)
    V = V + _uni(rng, -0.3, 0.3, n)
    return backproject(U, V, surface(U, V, W) + _uni(rng, -0.01, 0.01, n), W), U


def make_nodes(rng, W, grid):
    """(points, radii, image column) of ED nodes on a gx x gy grid over the image, on the surface, in shuffled index order."""
    gx, gy = grid
    P, U = _grid_nodes(rng, W, (np.arange(gx) + 0.5) * W / gx, (np.arange(gy) + 0.5) * H / gy)
    perm = rng.permutation(len(P))
    lo, hi = (0.25, 0.45) if len(P) <= 8 else (0.12, 0.3)
    return P[perm], _uni(rng, lo, hi, len(P)), U[perm]


TIE_COLUMNS = (12, 13)        # the pixel columns just right of the shared node column of ``make_tie_nodes``


def make_tie_nodes(rng, W):
    """130 ED nodes with 18 pairs at bit-identical positions whose indices lie in different runs of 64, laid out so that the
    candidate search meets the HIGHER index of a pair first and has to put the lower one in front of it afterwards.
    Run 0 (0..63): 4 columns x 16 rows over the left half of the image, shuffled inside the run.  Run 1 (64..127): copies of
    run 0's rightmost column (u = 11.4) and 3 columns of its own over the right half, shuffled inside the run.  A point just
    right of the shared column is inside run 1's bounding box and outside run 0's, so run 1 is scanned first.  Run 2: node
    128 copies a node of run 1 and node 129 one of run 0 (the tail loop of the scan against its four-at-a-time loop).
    Returns (points, radii, image column, pairs (18, 2) as (lower index, higher index))."""
    rows = np.arange(16) + 0.5
    PL, UL = _grid_nodes(rng, W, [1.5, 4.8, 8.1, 11.4], rows)          # column index = position % 4
    PR, UR = _grid_nodes(rng, W, [13.2, 16.8, 20.4], rows)
    pl = rng.permutation(64)
    PL, UL = PL[pl], UL[pl]
    shared = np.nonzero(pl % 4 == 3)[0]                                  # run-0 indices of the u = 11.4 column
    pr = rng.permutation(64)
    P1, U1 = np.concatenate([PL[shared], PR])[pr], np.concatenate([UL[shared], UR])[pr]
    where1 = np.empty(64, np.int64)
    where1[pr] = np.arange(64)                                           # row of the concatenation -> place in run 1
    pairs = [(int(j), 64 + int(where1[i])) for i, j in enumerate(shared)]
    a, c = 64 + int(where1[16 + 3 * 7 + 1]), int(np.nonzero(pl == 4 * 8 + 1)[0][0])     # interior nodes of run 1 / run 0
    P = np.concatenate([PL, P1, P1[a - 64][None], PL[c][None]])
    U = np.concatenate([UL, U1, U1[a - 64][None], UL[c][None]])
    pairs += [(a, 128), (c, 129)]
    return P, _uni(rng, 0.12, 0.3, len(P)), U, np.array(pairs, np.int64)


def make_frame(rng, W, occupied, time, seg, miss_columns=()):
    """A new frame: one point on the ray of every valid pixel.  ``occupied`` (H, W): depth of the surfel a point should
    meet, NaN where there is none (fewer of those pixels are valid, so that the appended rows stay few).  Every pixel of
    ``miss_columns`` is valid and misses th_dist (a new surfel there for certain)."""
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    has = ~np.isnan(occupied)
    valid = rng.random((H, W)) < np.where(has, 0.85, 0.15)
    base = np.where(has, occupied, surface(uu, vv, W))
    r = rng.random((H, W))
    sign = np.where(rng.random((H, W)) < 0.5, -1.0, 1.0)
    for u in miss_columns:
        valid[:, u], r[:, u] = True, 0.8
    z = np.where(r < 0.78, base + _uni(rng, -0.003, 0.003, (H, W)),            # meets the surfel
                 np.where(r < 0.9, base + sign * _uni(rng, 0.03, 0.08, (H, W)),    # misses th_dist: a new surfel
                          base + 0.7))                                              # farther than every node radius
    T = int(valid.sum())
    index_map = -np.ones((H, W), np.int64)
    index_map[valid] = np.arange(T)
    norms = _normals(rng, T)
    flip = rng.random(T) < 0.04                                                # fails the normal test
    norms[flip] = -norms[flip]
    f = dict(new_points=backproject(uu[valid], vv[valid], z[valid], W), new_norms=norms,
             new_colors=_uni(rng, 0.0, 255.0, (T, 3)).astype(np.float32), new_radii=_uni(rng, 0.002, 0.004, T),
             new_confs=_uni(rng, 0.05, 1.0, T).astype(np.float32), new_valid=valid.reshape(-1), new_index_map=index_map,
             time=time)
    if seg:
        conf = _class_conf(rng, uu[valid], W)
        f.update(new_seg=np.argmax(conf, 1).astype(np.int64), new_seg_conf=conf, new_dist2edge=_uni(rng, 0.0, 20.0, T))
    return f


def second_frame(b, seed=101, time=42):
    """Another frame of the same scene (its points meet the surface, not particular surfels)."""
    W = int(b["W"])
    vv, uu = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    occupied = np.where(np.random.default_rng(seed + 1).random((H, W)) < 0.7, surface(uu, vv, W), np.nan)
    return make_frame(np.random.default_rng(seed), W, occupied, time, "sf_seg" in b)


def _make(K=4, grid=(7, 5), W=24, seg=False, track=False, ties=False, knn_ties=False, seed=3):
    rng = np.random.default_rng(seed)
    pts, groups, n = [], {}, 0
    if knn_ties:
        ed_points, ed_radii, ed_u, groups["knn_pairs"] = make_tie_nodes(rng, W)
    else:
        ed_points, ed_radii, ed_u = make_nodes(rng, W, grid)
    for name, (cnt, dz, jit) in GROUP.items():
        u, v = PIX[name]
        z0 = 1.0 if name != "B" else surface(u, v, W)
        z = (z0 + dz * np.arange(cnt))[rng.permutation(cnt)]                   # index order is not depth order
        pts.append(backproject(u + _uni(rng, -jit, jit, cnt), v + _uni(rng, -jit, jit, cnt), z, W))
        groups[name] = np.arange(n, n + cnt)
        n += cnt
    # one surfel on about half of the other valid pixels
    occupied = np.full((H, W), np.nan)
    special = set(PIX.values())
    su, sv = [], []
    for v in range(H - 1):
        for u in range(W - 1):
            if (u, v) not in special and rng.random() < 0.55:
                su.append(u)
                sv.append(v)
    su, sv = np.array(su, np.float64), np.array(sv, np.float64)
    sz = surface(su, sv, W) + _uni(rng, -0.01, 0.01, len(su))
    occupied[sv.astype(int), su.astype(int)] = sz
    for name, (u, v) in PIX.items():
        occupied[v, u] = 1.0 if name != "B" else surface(u, v, W)
    pts.append(backproject(su + _uni(rng, -0.12, 0.12, len(su)), sv + _uni(rng, -0.12, 0.12, len(sv)), sz, W))
    n_single = len(su)
    # the pixel just outside each border and the last one inside (the tests are u < W - 1, v < H - 1, exclusive)
    bu = np.array([-0.7, -0.7, -0.3, W - 1.3, W - 1.3, W - 1.7, 6.2, 11.1, 17.3, 6.3, 11.2, 17.1, 3.1, 8.2])
    bv = np.array([2.1, 7.2, 12.1, 3.3, 9.1, 13.2, -0.7, -0.6, -0.3, H - 1.3, H - 1.4, H - 1.7, 2.2, 6.1])
    pts.append(backproject(bu, bv, surface(bu, bv, W) + 0.02, W))
    # two unstable surfels on pixel A's ray (they take no layer)
    pts.append(backproject(np.array([5.1, 4.9]), np.array([4.1, 3.9]), np.array([0.9, 0.95]), W))
    P = np.concatenate(pts)
    N = len(P)
    stable = np.ones(N, bool)
    first_single = n
    stable[first_single:first_single + n_single] = rng.random(n_single) >= 0.05
    stable[-2:] = False
    confs = _uni(rng, 0.2, 3.0, N).astype(np.float32)
    if ties:
        confs[groups["B"]] = np.float32(1.5)                                   # all equal
        confs[groups["A"][1::2]] = confs[groups["A"][0::2]]                    # equal in pairs
    dist, idx = _knn(P, ed_points, K)
    e = 1.0 / (1.0 + dist / ed_radii[idx])                                     # any positive weights: fusion recomputes them
    b = dict(H=H, W=W, K=np.array([[FX, 0.0, W / 2], [0.0, FX, CY], [0.0, 0.0, 1.0]]), num_neighbors=K,
             sf_points=P, sf_norms=_normals(rng, N), sf_colors=_uni(rng, 0.0, 255.0, (N, 3)).astype(np.float32),
             sf_radii=_uni(rng, 0.002, 0.004, N), sf_confs=confs,
             sf_time_stamp=(TIME - 1.0 - rng.integers(0, 45, N)).astype(np.float32), sf_isStable=stable,
             sf_knn_idx=idx.astype(np.int64), sf_knn_w=e / e.sum(1, keepdims=True), ed_points=ed_points, ed_radii=ed_radii)
    if seg:
        u_sf = P[:, 0] * FX / P[:, 2] + W / 2
        conf, ed_conf = _class_conf(rng, u_sf, W), _class_conf(rng, ed_u, W, noise=0.9)
        b.update(num_classes=NUM_CLASSES, sf_seg=np.argmax(conf, 1).astype(np.int64), sf_seg_conf=conf,
                 sf_dist2edge=_uni(rng, 0.0, 20.0, N), ed_seg=np.argmax(ed_conf, 1).astype(np.int64), ed_seg_conf=ed_conf)
        assert np.bincount(b["ed_seg"], minlength=NUM_CLASSES).min() >= K
    b.update(make_frame(rng, W, occupied, TIME, seg, TIE_COLUMNS if knn_ties else ()))
    if track:
        # overflow surfels of pixel A (its two lowest confidences), every surfel of pixel B (absorbed ones and absorbers), a
        # surfel that starts unstable, a stale one, unassigned
        a_low = groups["A"][np.argsort(confs[groups["A"]], kind="stable")[:2]]
        singles = np.arange(first_single, first_single + n_single)
        unstable = singles[~stable[singles]][:1]
        far = np.isnan(occupied) | ~b["new_valid"].reshape(H, W)             # no new point meets it: the stamp stays
        lonely = far[sv.astype(int), su.astype(int)]
        stale = singles[stable[singles] & lonely & (b["sf_time_stamp"][singles] <= TIME - 30)][:1]
        assert len(unstable) == 1 and len(stale) == 1
        b["track_id"] = np.concatenate([a_low, groups["B"], unstable, stale, [-1, -1]]).astype(np.int64)
        groups["track_unstable"], groups["track_stale"] = unstable, stale
    for name in GROUP:                                                         # distinct confidences per pixel, ties apart
        assert ties or len(np.unique(confs[groups[name]])) == len(groups[name])
    return b, dict(th_dist=TH_DIST), groups


def _spec(name):
    for table in (CASES, ORACLE_ONLY, CARRIED):
        if name in table:
            return dict(table[name])
    raise KeyError(name)


def build(name):
    """(b, okw, groups): the ``b`` dict of test_gpu_fusion._objects / test_fusion_oracle.load, the option overrides, and the
    surfel rows of pixels A-D (with ``track_unstable`` / ``track_stale`` for the ``track`` case)."""
    if name in DEGENERATE:
        return _degenerate(name)
    spec = _spec(name)
    extra = spec.pop("okw", {})
    b, okw, groups = _make(seed=SEEDS.get(name, 3), **spec)
    okw.update(extra)
    return b, okw, groups


def _degenerate(name):
    """``empty_model``: n = 0.  ``empty_frame``: ``valid`` all false, T = 0.  ``none_project``: every surfel outside the
    image (nothing is merged, nothing added).  ``all_dropped``: every surfel stale and no merge refreshes a stamp, so the swap
    keeps nothing (``second_frame`` is then fused into the n = 0 model).  Oracle only: they were not run through the
    reference."""
    b, okw, groups = _make(seed=3)
    if name == "empty_model":
        for k in MODEL_FIELDS:
            b[k] = b[k][:0]
    elif name == "empty_frame":
        for k in ("new_points", "new_norms", "new_colors", "new_radii", "new_confs"):
            b[k] = b[k][:0]
        b["new_valid"] = np.zeros(H * int(b["W"]), bool)
        b["new_index_map"] = -np.ones((H, int(b["W"])), np.int64)
    elif name == "none_project":
        b["sf_points"] = b["sf_points"] + np.array([5.0, 0.0, 0.0])
    elif name == "all_dropped":
        b["sf_time_stamp"] = np.minimum(b["sf_time_stamp"], np.float32(TIME - 30))
        okw.update(disable_merging_new_surfels=True, disable_merging_exist_surfels=True)
    return b, okw, {} if name == "empty_model" else groups


def is_seg(name):
    return name not in DEGENERATE and bool(_spec(name).get("seg"))


def digest(b):
    """sha256 over the arrays of ``b`` (names, dtypes, shapes and bytes, in name order)."""
    h = hashlib.sha256()
    for k in sorted(b):
        a = np.ascontiguousarray(b[k])
        h.update(f"{k}:{a.dtype.str}:{a.shape}".encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


# ------------------------------------------------------------------------------------------------ the golden file's layout
# tests/golden/fu_edges.npz holds the reference's outputs without loss, but not row by row: of a fused field only the rows
# that differ from the scene's input field and the appended rows (``_rows`` / ``_vals``), and of the swap the numbers of the
# fused rows it kept (the generator checks that every swapped field is exactly those rows).
BASE_OF = {"points": "sf_points", "norms": "sf_norms", "colors": "sf_colors", "radii": "sf_radii", "confs": "sf_confs",
           "time_stamp": "sf_time_stamp", "isStable": "sf_isStable", "knn_indices": "sf_knn_idx", "knn_w": "sf_knn_w",
           "seg": "sf_seg", "seg_conf": "sf_seg_conf", "dist2edge": "sf_dist2edge"}
OUT_FIELDS = ("points", "norms", "colors", "radii", "confs", "time_stamp", "isStable", "knn_indices", "knn_w", "projdata")
OUT_SEG_FIELDS = ("seg", "seg_conf", "dist2edge")


class Gold(dict):
    """Expanded arrays of one case under the keys test_fusion_oracle.check / test_gpu_fusion._check read."""

    @property
    def files(self):
        return list(self)


def pack_field(out, base):
    """(rows, vals): the rows of ``out`` that are not bit-equal to the same row of ``base``, and every row past its end."""
    n0 = len(base)
    assert out.dtype == base.dtype and out.shape[1:] == base.shape[1:] and len(out) >= n0
    diff = np.nonzero((out[:n0] != base).reshape(n0, -1).any(1))[0]
    rows = np.concatenate([diff, np.arange(n0, len(out))])
    return rows.astype(np.int32), out[rows]


def unpack_field(base, rows, vals, n):
    full = np.empty((n,) + base.shape[1:], base.dtype)
    full[:len(base)] = base
    full[rows] = vals
    return full


def expand_golden(g, name, b):
    """The recorded ``<name>_fuse_*`` / ``<name>_swap_*`` arrays of case ``name`` whose inputs are ``b``."""
    np.testing.assert_array_equal(g[f"{name}_in_digest"], digest(b), err_msg="the scene is not the recorded one")
    out = Gold()
    n = int(g[f"{name}_fuse_n"])
    fields = OUT_FIELDS + (OUT_SEG_FIELDS if f"{name}_fuse_seg_rows" in g.files else ())
    keep = g[f"{name}_swap_rows"]
    for f in fields:
        if f == "projdata":
            full = g[f"{name}_fuse_projdata"]
        else:
            full = unpack_field(b[BASE_OF[f]], g[f"{name}_fuse_{f}_rows"], g[f"{name}_fuse_{f}_vals"], n)
        out[f"{name}_fuse_{f}"] = full
        out[f"{name}_swap_{f}"] = np.ones(len(keep), bool) if f == "isStable" else full[keep]
    for k in ("fuse_track_id", "swap_track_id"):
        if f"{name}_{k}" in g.files:
            out[f"{name}_{k}"] = g[f"{name}_{k}"]
    return out
