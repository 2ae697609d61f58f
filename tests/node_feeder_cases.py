"""Inputs and expectations of the node-feeder edge tests (find_knn, the skinning weights, Surfels.update): pure NumPy, no GPU,
no torch.  test_gpu_node_feeder.py runs them through super_amd.nodes on the device; the expectations come from the oracles
(oracle/lm_oracle.py: knn, knn_weights, apply_update; oracle/fusion_oracle.py: class_knn, semantic_weights).

Search.  Every coordinate is a multiple of 1/8 inside +-64, so every difference, square and sum of three squares is exact in
float32 and float64 whatever the FMA contraction: equal distances are REAL ties, and the ids are bit-exact against the oracle's
"squared L2 ascending, lowest index first".  The node counts sit around the search kernel's LDS tile (KNN_TILE nodes).

Weights.  Rows whose only in-radius neighbour has dist == radius exactly (stable kept) or radius = nextafter(dist, 0)
(stable cleared), K = 1 and K = 9, both radius modes, class distributions with zero entries.

Update.  J = K nodes with non-unit quaternions; surfel 0 is built from dyadic numbers so that its blended normal is EXACTLY
zero (the 1e-12 floor of F.normalize applies); the (J+1, 7) deformation composes the oracle with the global row as
super/nodes.py:193-223 does."""
import functools

import numpy as np

from oracle import fusion_oracle as fus
from oracle import lm_oracle as orc

KNN_TILE = 1024                      # nodes per LDS tile of the search kernel (csrc/slm_nodes.hip)
KNN_MAXK = 9                         # K + skip_self at most
SEARCH_NN = (1023, 1024, 1025, 2049)   # ... and K + skip_self itself (search_sizes)
SEARCH_NQ = (1, 255, 257)
SHORT_CLASS_TEXT = "slm_knn_f64: a class has fewer nodes than the neighbours asked for"


def lattice(rng, n, span=512):
    """n points with coordinates m/8, |m| <= span <= 512"""
    return rng.integers(-span, span + 1, size=(n, 3)).astype(np.float64) / 8.0


def search_sizes(K, skip):
    return [(nn, nq) for nn in (K + skip,) + SEARCH_NN for nq in SEARCH_NQ]


@functools.lru_cache(maxsize=None)
def search_case(Nn, Nq):
    """(nodes, queries, dist9, idx9): the first min(Nq, Nn) queries ARE the nodes (skip_self drops a real self), the rest free
    lattice points.  A small span (many equal distances) except for Nq = 255.  dist9 / idx9: the oracle's min(9, Nn) nearest,
    shared by every K and skip_self (expected_search)."""
    rng = np.random.default_rng(1000 * Nn + Nq)
    span = 512 if Nq == 255 else 12
    nodes = lattice(rng, Nn, span)
    q = lattice(rng, Nq, span)
    m = min(Nq, Nn)
    q[:m] = nodes[:m]
    d, i = orc.knn(q, nodes, min(KNN_MAXK, Nn))
    for a in (nodes, q, d, i):
        a.setflags(write=False)
    return nodes, q, d, i


def expected_search(d9, i9, K, skip):
    """skip_self drops the nearest (the reference's [:, 1:])"""
    return d9[:, skip:skip + K], i9[:, skip:skip + K]


@functools.lru_cache(maxsize=None)
def tile_edge_case():
    """Query 0 (the origin) is equidistant from node KNN_TILE - 1 and node KNN_TILE, the last of the first tile and the first
    of the second; node 7 lies a 3-4-5 triple away (dist == 5.0 exactly); every other node is at least 16 away.  Query 3 is
    node 3, whose bit-identical duplicate is node KNN_TILE + 1: under skip_self node 3 drops itself and keeps the duplicate at
    distance 0, the duplicate drops node 3 and keeps ITSELF (the reference drops column 0, whatever it holds)."""
    rng = np.random.default_rng(5)
    Nn = KNN_TILE + 2
    nodes = lattice(rng, Nn)
    nodes[:, 0] = rng.integers(128, 513, size=Nn) / 8.0
    nodes[KNN_TILE - 1] = (1.0, 0.0, 0.0)
    nodes[KNN_TILE] = (-1.0, 0.0, 0.0)
    nodes[7] = (3.0, 4.0, 0.0)
    nodes[KNN_TILE + 1] = nodes[3]
    q = nodes.copy()
    q[0] = 0.0
    d, i = orc.knn(q, nodes, 5)
    assert i[0, :3].tolist() == [KNN_TILE - 1, KNN_TILE, 7] and d[0, :3].tolist() == [1.0, 1.0, 5.0] and d[0, 3] >= 16.0
    assert i[3, :2].tolist() == [3, KNN_TILE + 1] and i[KNN_TILE + 1, :2].tolist() == [3, KNN_TILE + 1]
    assert d[3, 1] == 0.0 and d[KNN_TILE + 1, 1] == 0.0
    return nodes, q, d, i


@functools.lru_cache(maxsize=None)
def class_case(K, short=False):
    """(nodes, node_seg, queries, q_seg, dist, idx).  Classes 0 and 1 interleave (index parity).  Around the origin class 1 has
    plenty of nodes in the first tile, class 0 only K - 1 there and its K-th in the SECOND tile, everything else of either
    class at least 14 away: the class-0 queries near the origin end on that node, the unrestricted search would not.  Class 2
    has exactly K nodes, one of them in the second tile.  short: class 3 has K - 1 nodes and one query (dist, idx = None:
    the reference asserts, the library refuses with SHORT_CLASS_TEXT)."""
    rng = np.random.default_rng(40 + K)
    Nn = KNN_TILE + 9
    nodes = lattice(rng, Nn)
    nodes[:, 0] = rng.integers(128, 513, size=Nn) / 8.0
    seg = (np.arange(Nn) % 2).astype(np.int32)
    near1 = np.arange(1, 2 * KNN_MAXK + 2, 2)                                  # class 1, first tile
    near0 = np.concatenate([np.arange(0, 2 * (K - 1), 2), [KNN_TILE + 2]]).astype(np.int64)   # class 0: K - 1 + the K-th
    for ids in (near1, near0):
        nodes[ids] = lattice(rng, len(ids), 8)
    nodes[near0[-1]] = (4.0, 4.0, 4.0)                                         # farther than the others within +-1, nearer than the rest
    c2 = np.concatenate([200 + 3 * np.arange(K - 1), [KNN_TILE + 5]]).astype(np.int64)
    seg[c2] = 2
    nq = 60
    q = lattice(rng, nq)
    q_seg = (np.arange(nq) % 3).astype(np.int32)
    q[:20] = lattice(rng, 20, 8)                                               # near the origin, classes 0, 1, 2 in turn
    if short:
        c3 = 400 + 5 * np.arange(K - 1)
        seg[c3] = 3
        q_seg[-1] = 3
        return nodes, seg, q, q_seg, None, None
    d, i = fus.class_knn(q, q_seg, nodes, seg, K, 3)
    own0 = np.arange(20)[q_seg[:20] == 0]
    assert (i[own0, K - 1] == KNN_TILE + 2).all(), "the K-th class-0 neighbour must lie in the second tile"
    assert (seg[i] == q_seg[:, None]).all() and (np.bincount(seg, minlength=3)[2] == K)
    assert (i[q_seg == 2] >= KNN_TILE).any()
    if K > 1:      # the unrestricted search answers differently: the class test decides
        assert (orc.knn(q[own0], nodes, K)[1] != i[own0]).any()
    return nodes, seg, q, q_seg, d, i


def weights_case(K, radius_mode, C, f32):
    """dict(idx, dist, radii, stable, q_conf, node_conf, w, stable_out) for Nq = 257 queries over J = 64 nodes; dist and radii
    are float32 values when f32.  Row 0: the only in-radius neighbour has dist == radius == 5.0 (a 3-4-5 triple's distance):
    stable kept.  Row 1: the same with radius = nextafter(5, 0): cleared.  Row 2: inside, but unstable before: stays cleared."""
    rng = np.random.default_rng(100 * K + 10 * radius_mode + C)
    Nq, J = 257, 64
    ft = np.float32 if f32 else np.float64
    idx = np.stack([rng.permutation(J)[:K] for _ in range(Nq)]).astype(np.int64)
    idx[0], idx[1] = np.arange(K), K + np.arange(K)
    dist = rng.uniform(0.05, 2.0, size=(Nq, K)).astype(ft)
    radii = rng.uniform(0.5, 1.5, size=J if radius_mode == 0 else Nq).astype(ft)
    dist[0] = dist[1] = 5.0 + np.arange(K)
    below = np.nextafter(ft(5.0), ft(0.0))
    if radius_mode == 0:
        radii[idx[0]] = radii[idx[1]] = dist[0] - ft(0.5)
        radii[idx[0, 0]], radii[idx[1, 0]] = 5.0, below
    else:
        radii[0], radii[1] = 5.0, below
    dist[2, 0] = 0.25                                     # (radii >= 0.5: inside)
    stable = rng.random(Nq) < 0.8
    stable[:3] = (True, True, False)
    dist64, radii64 = dist.astype(np.float64), radii.astype(np.float64)
    rad = radii64[idx] if radius_mode == 0 else radii64[:, None]
    inside = (dist64 <= rad).any(1)
    assert inside[0] and not inside[1] and inside[2] and (dist64[0] <= rad[0]).sum() == 1
    q_conf = node_conf = None
    if C > 0:
        q_conf, node_conf = rng.random((Nq, C)) + 0.05, rng.random((J, C)) + 0.05
        if C >= 4:      # zero probabilities: the eps inside the log keeps P log(P / (M + eps) + eps) finite
            q_conf[0, 2:] = 0.0
            node_conf[idx[0, 0], 0] = node_conf[idx[0, 0], 3] = 0.0
        q_conf /= q_conf.sum(1, keepdims=True)
        node_conf /= node_conf.sum(1, keepdims=True)
        w = fus.semantic_weights(dist64, rad, node_conf[idx], q_conf[:, None, :])
    else:
        w = orc.knn_weights(dist64, rad)
    assert np.isfinite(w).all()
    return dict(idx=idx, dist=dist, radii=radii, stable=stable, q_conf=q_conf, node_conf=node_conf, w=w, stable_out=stable & inside)


def update_case(K, N, with_global, f32):
    """dict(points, norms, knn_idx, knn_w, ed_points, ed_norms, deform, want = (points, norms, ed_points, ed_norms)): J = K
    nodes, every surfel skinned by all of them in its own order, non-unit quaternions; the state holds float32 values when
    f32.  Surfel 0 (N > 0) has weight 1 on node 0, whose q = (1/2, 0, 0, 1/2) maps its normal (1/4, 0, 1/8) to (1/8, 1/8, 1/8)
    in dyadic arithmetic, and b_0 = -(1/8, 1/8, 1/8): the blended normal is exactly zero."""
    rng = np.random.default_rng(1000 * K + 10 * N + with_global)
    J = K
    ft = np.float32 if f32 else np.float64
    st = lambda a: a.astype(ft).astype(np.float64)      # the state as the device holds it
    points = st(rng.uniform(-0.5, 0.5, size=(N, 3)))
    norms = rng.normal(size=(N, 3))
    norms = st(norms / np.linalg.norm(norms, axis=1, keepdims=True))
    knn_idx = np.stack([rng.permutation(J) for _ in range(N)]).astype(np.int64) if N else np.zeros((0, K), np.int64)
    knn_w = rng.random((N, K)) + 0.1
    knn_w = st(knn_w / knn_w.sum(1, keepdims=True))
    ed_points = st(rng.uniform(-0.5, 0.5, size=(J, 3)))
    ed_norms = rng.normal(size=(J, 3))
    ed_norms = st(ed_norms / np.linalg.norm(ed_norms, axis=1, keepdims=True))
    deform = np.zeros((J + int(with_global), 7))
    deform[:, 0] = 1.0
    deform[:, :4] += rng.normal(scale=0.3, size=(len(deform), 4))
    deform[:, :4] *= rng.uniform(0.7, 1.3, size=(len(deform), 1))       # non-unit: the reference never normalises
    deform[:, 4:] = rng.normal(scale=0.05, size=(len(deform), 3))
    deform[0] = (0.5, 0.0, 0.0, 0.5, -0.125, -0.125, -0.125)
    if N:
        norms[0] = (0.25, 0.0, 0.125)
        knn_idx[0] = np.arange(K)
        knn_w[0] = np.eye(K)[0]
    beta = deform[:J]
    p, n, g, gn = orc.apply_update(points, norms, knn_idx, knn_w, ed_points, ed_norms, beta)
    if N:
        assert (n[0] == 0.0).all(), "surfel 0: the blended normal must be exactly zero"
    if with_global:      # super/nodes.py:204-205, 211-212, 219-222: T_g moves points and nodes, R_g turns the blended normals
        qg, tg = deform[-1:, :4], deform[-1, 4:]
        p, g = p + tg, g + tg
        # (R_g is linear, so R_g of the normalised blend has the direction of R_g of the blend; zero stays zero)
        n, gn = orc._normalize(orc.quat_apply(qg, n)), orc._normalize(orc.quat_apply(qg, gn))
    return dict(points=points, norms=norms, knn_idx=knn_idx, knn_w=knn_w, ed_points=ed_points, ed_norms=ed_norms, deform=deform,
                want=(p, n, g, gn))
