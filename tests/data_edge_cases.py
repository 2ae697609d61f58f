"""TEST INFRASTRUCTURE: one deterministic scene that puts surfels on every edge of the point-to-plane term's MATCH SET.

The data term decides per surfel whether it enters the normal equations: it projects the warped point, rounds the pixel
half-to-even, tests the rounded pixel against ``0 <= v < H-1, 0 <= u < W-1`` and against ``valid``, and drops the surfel if
any of the four bilinear taps is outside the image, unmapped (``index_map < 0``) or NaN (``eval_surfel_coreT``,
csrc/slm_data.h; ``project`` / ``bilinear_taps`` / ``bilinear_lookup`` / ``data_term``, oracle/lm_oracle.py; reference
``utils/utils.py:161-184``, ``super/loss.py:106-157,222-255``: defects D2 and D4 of the oracle).  ``synth.make_scene`` only
makes surfels at generic sub-pixel positions well inside the image; ``edge_scene`` adds hand-placed ones.

Layout.  A 60 x 80 frame, J = 48, every pixel of the target valid and mapped (target border 0) before holes are cut by
hand.  The hand-placed surfels come FIRST (``GROUPS``: name -> index array, the same for every K and every count of generic
surfels), the ``n_base`` generic surfels of ``make_scene`` after them.  Interior groups get one 5 x 5 pixel cell per surfel,
so that no hole of one surfel reaches the taps of another.

Exact ties.  A tie only tests anything if device and oracle compute the same bits for T(p).  Every hand-placed surfel has
the weights (w0, 0, ..., 0) and a first node g with ``(p - g) + g == p`` bitwise in float64, so that at the identity warp
T == p under any summation order, with or without FMA contraction (the quaternion part is d + 0 + 0, the other nodes add
0 * finite).  ``p.x`` of an exact coordinate is found by stepping ``np.nextafter`` from ``(m - cx) * Ze / fx`` until the
oracle's own expression ``x * fx / Ze + cx`` gives ``m`` bit for bit (a division stands between the product and the sum:
nothing can fuse there).  This holds in FLOAT64 STATE only: ``state32`` rounds positions and weights to float32, the
surfels become generic, and the oracle frame must be built from the rounded arrays (``Frame.from_scene(state32(sc))``).
The intrinsics are float32 values (the ABI carries fx, fy, cx, cy as float); the oracle reads the same rounded numbers.

``z_eps`` cannot get T.z = -1e-8 out of ``(p - g) + g`` (no node has z near 0), so it uses the weight: p.z = -1 is exact
against every node and w0 = 1e-8 makes T.z = 1e-8 * -1.0, the exact negative of the epsilon: Z + 1e-8 == 0.

``nonfinite_p``.  Read before adding it: a surfel's position is loaded in ``slm_prep.hip`` only by ``k_fill_sorted`` and
``kb_fill`` (``ld_state3(f.sf_points, i)``), which COPY it into the tuple-sorted stream; the sort keys are the node ids
alone.  ``slm_bind.hip`` only null-checks the pointer and compares it when it recognises a rebound frame.  The evaluation
(csrc/slm_data.h) converts coordinates to int only behind ``pv`` (false for NaN and out of range) and indexes with them only
behind ``inside``.  So a position never forms an address or a key and NaN / inf are safe to bind.  The group has NaN in x,
y, z and +-inf in x and y.  An infinite z is left out: with one neighbour T.z = inf projects to the principal point, the
surfel MATCHES with an infinite residual (in the reference too) and the system holds nothing to compare.
"""
import dataclasses
import hashlib

import numpy as np

from oracle import lm_oracle as orc
from super_amd import synth

H, W, J, N_BASE, SEED = 60, 80, 48, 600, 71
KS = (1, 4, 6)
DELTA = 2.0 ** -20            # "just below / just above" a boundary, in pixels
_CELLS_PER_ROW = 13           # interior cells: origin (5 + 5 r, 5 + 5 c), r < 9, c < 13


def _intr(K):
    return float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])


def _solve_exact(m, c, f, Ze):
    """x with ``x * f / Ze + c == m`` bitwise (the oracle's expression), or None"""
    m, Ze = np.float64(m), np.float64(Ze)
    lo = hi = np.float64((m - c) * Ze / f)
    for _ in range(512):
        for x in (hi, lo):
            if x * f / Ze + c == m:
                return x
        hi, lo = np.nextafter(hi, np.inf), np.nextafter(lo, -np.inf)
    return None


class _Builder:
    def __init__(self, base):
        self.K = base.K
        self.g = base.ed_points.astype(np.float64)
        self.valid = base.valid.reshape(H, W).copy()
        self.index_map = base.index_map.copy()
        self.tp, self.tn = base.tgt_points.copy(), base.tgt_norms.copy()
        self.p, self.first, self.w0, self.group, self.expect, self.exact = [], [], [], [], [], []
        self.cell = 0

    # ---- the target side ----
    def next_cell(self):
        """(n, m): the pixel two in from the origin of a fresh interior cell; taps of a surfel there stay in n..n+1"""
        r, c = divmod(self.cell, _CELLS_PER_ROW)
        assert r < 9
        self.cell += 1
        return 5 + 5 * r + 2, 5 + 5 * c + 2

    def invalidate(self, n, m):
        self.valid[n, m] = False

    def unmap(self, n, m):
        self.index_map[n, m] = -1

    # ---- the surfel side ----
    def place(self, group, u, v, expect, exact_u=False, exact_v=False, z0=1.0, w0=1.0, raw=None):
        """a surfel projecting to (u, v) at the identity warp; ``raw``: the position itself (no projection asked for)"""
        fx, fy, cx, cy = _intr(self.K)
        exact = raw is None
        if raw is not None:
            p, first = np.array(raw, np.float64), self._first(np.array(raw, np.float64), need_exact=False)
        else:
            p = first = None
            for k in range(4096):
                Z = np.float64(z0 + np.sign(z0) * k * 2.0 ** -12)
                Ze = Z + 1e-8
                x = _solve_exact(u, cx, fx, Ze) if exact_u else np.float64((u - cx) * Ze / fx)
                y = _solve_exact(v, cy, fy, Ze) if exact_v else np.float64((v - cy) * Ze / fy)
                if x is None or y is None:
                    continue
                cand = np.array([x, y, Z], np.float64)
                first = self._first(cand, need_exact=True)
                if first is not None:
                    p = cand
                    break
            assert p is not None, (group, u, v)
        self.p.append(p)
        self.first.append(first)
        self.w0.append(w0)
        self.group.append(group)
        self.expect.append(bool(expect))
        self.exact.append(exact)

    def _first(self, p, need_exact):
        q = np.where(np.isfinite(p), p, 0.0)
        order = np.argsort(((self.g - q) ** 2).sum(1), kind="stable")
        if not need_exact:
            return int(order[0])
        for j in order[:12]:
            if np.array_equal((p - self.g[j]) + self.g[j], p):
                return int(j)
        return None


def _place_groups(b):
    # ---- D4: exactly integer coordinates (floor == ceil: the two coinciding taps both carry weight 1) ----
    for i in range(8):
        n, m = b.next_cell()
        b.place("int_u", m, n + 0.13 + 0.1 * i, True, exact_u=True)
    for i in range(8):
        n, m = b.next_cell()
        b.place("int_v", m + 0.17 + 0.1 * i, n, True, exact_v=True)
    for i in range(8):
        n, m = b.next_cell()
        b.place("int_uv", m + (i & 1), n + (i >> 1 & 1), True, exact_u=True, exact_v=True)
    # ---- exactly k + 0.5: half-to-even takes the floor tap for even k, the ceil tap for odd k.  Surfels 0-3 tie in u,
    #      4-7 in v; of each four: clean, the FLOOR-side pixel invalid (still mapped), the CEIL-side pixel invalid, clean.
    for name, odd in (("half_even", 0), ("half_odd", 1)):
        for i in range(8):
            n, m = b.next_cell()
            axis_u, kind = i < 4, i % 4
            if axis_u:
                m += (m & 1) != odd                     # k = m with the parity asked for (cells leave room for +1)
                fl, ce = (n, m), (n, m + 1)
                u, v = m + 0.5, n + 0.3
            else:
                n += (n & 1) != odd
                fl, ce = (n, m), (n + 1, m)
                u, v = m + 0.3, n + 0.5
            if kind == 1:
                b.invalidate(*fl)
            if kind == 2:
                b.invalidate(*ce)
            rounded_is_floor = not odd
            dropped = (kind == 1 and rounded_is_floor) or (kind == 2 and not rounded_is_floor)
            b.place(name, u, v, not dropped, exact_u=axis_u, exact_v=not axis_u)
    # ---- [-0.5, 0): rint gives -0.0, pixel 0 is valid, the floor tap is row / column -1 ----
    for i, f in enumerate((-0.5, -0.25, -DELTA, -0.4375)):
        b.place("neg_zero", 12.3 + 9 * i, f, False, exact_v=True)
        b.place("neg_zero", f, 11.3 + 9 * i, False, exact_u=True)
    # ---- the last admissible row / column (rounded H-2, W-2; H - 1.5 = 58.5 and W - 1.5 = 78.5 round DOWN: even) ----
    for i, f in enumerate((-0.3, 0.3, 0.5 - DELTA, 0.5)):
        b.place("last_ok", 8.3 + 9 * i, H - 2 + f, True, exact_v=True)
        b.place("last_ok", W - 2 + f, 7.3 + 9 * i, True, exact_u=True)
    for i, f in enumerate((0.5 + DELTA, 0.7, 1.0, 1.3)):
        b.place("first_bad", 44.3 + 8 * i, H - 2 + f, False, exact_v=True)
        b.place("first_bad", W - 2 + f, 30.3 + 7 * i, False, exact_u=True)
    # ---- 1e9 pixels outside, beyond 2**31 and beyond 2**40 ----
    for i, (u, v) in enumerate(((1e9, 20.3), (-1e9, 20.3), (30.3, 1e9), (30.3, -1e9), (3e9, 3e9), (-2.0 ** 31 - 0.5, 10.3),
                                (5e12, 30.3), (30.3, -5e12))):
        fx, fy, cx, cy = _intr(b.K)
        b.place("far_out", u, v, False, raw=[(u - cx) / fx, (v - cy) / fy, 1.0])
    # ---- the rounded pixel valid and mapped, exactly ONE of the other three taps a hole (invalid and unmapped) ----
    for fu, fv in ((0.3, 0.3), (0.7, 0.7), (0.7, 0.3)):
        rounded = (int(fv > 0.5), int(fu > 0.5))
        for tap in [(a, c) for a in (0, 1) for c in (0, 1) if (a, c) != rounded]:
            n, m = b.next_cell()
            b.invalidate(n + tap[0], m + tap[1])
            b.unmap(n + tap[0], m + tap[1])
            b.place("hole_tap", m + fu, n + fv, False)
    # ---- valid = 1, index_map = -1 at the rounded pixel: dropped through the taps ----
    for i in range(8):
        n, m = b.next_cell()
        fu, fv = (0.2, 0.8)[i & 1], (0.2, 0.8)[i >> 1 & 1]
        b.unmap(n + int(fv > 0.5), m + int(fu > 0.5))
        b.place("valid_unmapped", m + fu + 0.01 * i, n + fv, False)
    # ---- valid = 0, index_map >= 0 at a tap that is NOT the rounded pixel: still a match ----
    for i in range(8):
        n, m = b.next_cell()
        fu, fv = (0.2, 0.8)[i & 1], (0.2, 0.8)[i >> 1 & 1]
        rounded = (int(fv > 0.5), int(fu > 0.5))
        others = [(a, c) for a in (0, 1) for c in (0, 1) if (a, c) != rounded]
        for tap in (others if i >= 4 else others[i % 3:i % 3 + 1]):
            b.invalidate(n + tap[0], m + tap[1])
        b.place("mapped_invalid", m + fu, n + fv + 0.01 * i, True)
    # ---- a NaN point (0-3) or a NaN normal (4-7) in the target row of one tap ----
    for i in range(8):
        n, m = b.next_cell()
        row = b.index_map[n + (i >> 1 & 1), m + (i & 1)]
        (b.tp if i < 4 else b.tn)[row, i % 3] = np.nan
        b.place("nan_row", m + 0.4, n + 0.6, False)
    # ---- behind the camera, onto valid pixels: the reference matches it (mirrored) ----
    for i in range(8):
        n, m = b.next_cell()
        b.place("behind", m + 0.3 + 0.05 * i, n + 0.45, True, z0=-1.0)
    # ---- T.z = -1e-8 exactly: Z + 1e-8 == 0, the projection is +-inf or NaN ----
    for i, (x, y) in enumerate(((0.3, 0.1), (-0.3, 0.1), (0.3, -0.1), (0.0, 0.1), (0.3, 0.0), (-0.2, -0.2), (1.0, 1.0),
                                (-1.0, 0.5))):
        b.place("z_eps", None, None, False, raw=[x, y, -1.0], w0=1e-8)
    # ---- a non-finite position ----
    nan, inf = np.nan, np.inf
    for raw in ([nan, 0.05, 1.0], [0.05, nan, 1.0], [0.05, 0.05, nan], [nan, nan, nan], [inf, 0.05, 1.0],
                [0.05, inf, 1.0], [-inf, 0.05, 1.0], [0.05, -inf, 1.0]):
        b.place("nonfinite_p", None, None, False, raw=raw)


_CACHE = {}


def edge_scene(K=4, n_base=N_BASE):
    """the scene (a ``synth.Scene`` with float64 ``sf_points`` / ``sf_knn_w``); cached, do not modify"""
    if (K, n_base) in _CACHE:
        return _CACHE[(K, n_base)]
    base = synth.make_scene(N=n_base, J=J, H=H, W=W, seed=SEED, n_neighbors=K, src_border=5, tgt_border=0)
    assert base.T == H * W and (np.asarray(base.K, np.float32) == base.K).all()
    b = _Builder(base)
    _place_groups(b)
    n = len(b.p)
    P = np.stack(b.p)
    idx = np.empty((n, K), np.int64)
    for i in range(n):
        q = np.where(np.isfinite(P[i]), P[i], 0.0)
        order = [j for j in np.argsort(((b.g - q) ** 2).sum(1), kind="stable") if j != b.first[i]]
        idx[i] = [b.first[i]] + order[:K - 1]
    w = np.zeros((n, K))
    w[:, 0] = b.w0
    norms = np.tile([0.0, 0.0, -1.0], (n, 1))
    sc = dataclasses.replace(
        base, sf_points=np.concatenate([P, base.sf_points.astype(np.float64)]),
        sf_norms=np.concatenate([norms, base.sf_norms.astype(np.float64)]),
        sf_knn_idx=np.concatenate([idx, base.sf_knn_idx]), sf_knn_w=np.concatenate([w, base.sf_knn_w.astype(np.float64)]),
        tgt_points=b.tp, tgt_norms=b.tn, index_map=b.index_map, valid=b.valid.reshape(-1).copy(),
        meta=dict(base.meta, groups=np.array(b.group), expect=np.array(b.expect), exact=np.array(b.exact), n_groups=n))
    _CACHE[(K, n_base)] = sc
    return sc


def state32(sc):
    """the same scene in float32 state: positions, normals and weights rounded (what ``DeviceFrame.from_scene`` binds with
    ``state_f64=False``); the surfels of the exact groups become generic"""
    r = lambda a: a.astype(np.float32)
    return dataclasses.replace(sc, sf_points=r(sc.sf_points), sf_norms=r(sc.sf_norms), sf_knn_w=r(sc.sf_knn_w))


def subset(sc, keep):
    """the scene with the surfels ``keep`` (an index array) only"""
    keep = np.asarray(keep)
    return dataclasses.replace(sc, sf_points=sc.sf_points[keep], sf_norms=sc.sf_norms[keep], sf_knn_idx=sc.sf_knn_idx[keep],
                               sf_knn_w=sc.sf_knn_w[keep])


def without_groups(sc, names):
    """indices of the surfels that are in none of the groups ``names``"""
    drop = np.concatenate([GROUPS[n] for n in names]) if len(names) else np.zeros(0, np.int64)
    return np.setdiff1d(np.arange(sc.N), drop)


def _tables():
    m = edge_scene(4).meta
    names = list(dict.fromkeys(m["groups"].tolist()))
    groups = {n: np.nonzero(m["groups"] == n)[0] for n in names}
    cls = {}
    for n, ix in groups.items():
        e = m["expect"][ix]
        cls[n] = "match" if e.all() else ("dropped" if not e.any() else "mixed")
    return groups, cls, m["expect"].copy(), m["exact"].copy()


# GROUPS: name -> surfel indices; CLASSES: name -> "match" | "dropped" | "mixed" at the identity warp; EXPECT: per hand-placed
# surfel, matched at identity; EXACT: T == p bitwise at identity (all but far_out, z_eps and nonfinite_p, which sit far from
# every boundary or are exact by their own construction)
GROUPS, CLASSES, EXPECT, EXACT = _tables()
N_GROUPS = len(EXPECT)
D4_GROUPS = ("int_u", "int_v", "int_uv")


def identity(J_=J):
    return np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (J_, 1))


def generic_beta(seed=17, rot=0.01, trans=0.002):
    """a small random warp (``lm_corr_model.random_beta``): no hand-placed surfel sits exactly on a boundary any more"""
    rng = np.random.default_rng(seed)
    return identity() + np.concatenate([rng.normal(0, rot, (J, 4)), rng.normal(0, trans, (J, 3))], axis=1)


def tie_distance(fr, beta):
    """per surfel the distance (px) of its projection (u_, v_) from the nearest decision boundary: an integer (floor / ceil
    change), a half-integer (the rounded pixel changes; -0.5, H - 1.5 and W - 1.5 are half-integers).  inf for a surfel
    that no boundary decides: non-finite, or more than a pixel outside the image."""
    T, _ = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, beta)
    with np.errstate(all="ignore"):
        v_, u_, _, _ = orc.project(T, fr.K, fr.H, fr.W)
        d = np.minimum(np.abs(2 * u_ - np.rint(2 * u_)), np.abs(2 * v_ - np.rint(2 * v_))) / 2
        near = np.isfinite(u_) & np.isfinite(v_) & (u_ >= -1.5) & (u_ <= fr.W + 0.5) & (v_ >= -1.5) & (v_ <= fr.H + 0.5)
    return np.where(near, d, np.inf)


def digest(sc):
    """sha256 over the arrays of the scene that the data term reads (names, dtypes, shapes, bytes)"""
    h = hashlib.sha256()
    for k in ("K", "sf_points", "sf_knn_idx", "sf_knn_w", "ed_points", "ed_knn_idx", "tgt_points", "tgt_norms", "index_map",
              "valid"):
        a = np.ascontiguousarray(getattr(sc, k))
        h.update(f"{k}:{a.dtype.str}:{a.shape}".encode())
        h.update(a.tobytes())
    return np.frombuffer(h.digest(), np.uint8).copy()


def flipped_frames(sc):
    """the scene with ``valid`` AND ``index_map`` flipped at one of the four pixels around the clean surfel of ``half_even``
    and of ``half_odd`` (tie in u), one pixel at a time: 8 (label, scene).  The pixels are valid and mapped in ``sc``, so a
    flip cuts a hole: the surfel is dropped whichever tap it is, and its neighbours are not touched (own cell)."""
    fx, fy, cx, cy = _intr(sc.K)
    out = []
    for name in ("half_even", "half_odd"):
        i = GROUPS[name][0]
        p = sc.sf_points[i]
        u_, v_ = p[0] * fx / (p[2] + 1e-8) + cx, p[1] * fy / (p[2] + 1e-8) + cy
        for n in (int(np.floor(v_)), int(np.ceil(v_))):
            for m in (int(np.floor(u_)), int(np.ceil(u_))):
                valid, imap = sc.valid.reshape(H, W).copy(), sc.index_map.copy()
                assert valid[n, m] and imap[n, m] >= 0
                valid[n, m], imap[n, m] = False, -1
                out.append((f"{name}@{n},{m}", dataclasses.replace(sc, valid=valid.reshape(-1), index_map=imap)))
    return out


def invalid_only_frames(sc):
    """like ``flipped_frames`` but ``valid`` alone is cleared (the pixel stays mapped): the surfel is dropped only if the
    pixel is its ROUNDED pixel -- the direct test of which tap the per-pixel form takes the validity from"""
    out = []
    for label, fl in flipped_frames(sc):
        out.append((label, dataclasses.replace(fl, index_map=sc.index_map)))
    return out
