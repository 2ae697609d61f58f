"""TEST INFRASTRUCTURE: the rigid pre-alignment stage (``slm_rigid_*``, ``super_amd/rigid.py``) as the LM oracle sees it.

The stage is, by definition, the reference's LM loop on ONE node at the origin: every surfel attached to it with weight 1,
K = 1, the data term plus the Rot term.  So ``oracle/lm_oracle.py`` already is its checker, on a ``Frame`` built here:

    fr1 = one_node_frame(points, target fields of the real frame)
    opt = rigid_opt()                                   # default_opt(mesh_arap=False, mesh_rot=True)
    orc.lm(fr1, opt, trace=...)                         # the loop: (1,7) beta_g, one dict per iteration
    orc.normal_equations(fr1, beta, opt)                # the 7 x 7 system
    orc.total_loss(fr1, beta, opt)                      # the loss and the match count
    moved(points, norms, Tg)                            # the rigid move, through orc.apply_update
"""
import numpy as np

from oracle import lm_oracle as orc

IDENTITY = np.array([1.0, 0, 0, 0, 0, 0, 0])


def rigid_opt(**kw):
    kw = dict(dict(mesh_arap=False, mesh_rot=True), **kw)
    return orc.default_opt(**kw)


def one_node_frame(points, tgt_points, tgt_norms, index_map, valid, K, H, W):
    n = len(points)
    return orc.Frame(sf_points=np.asarray(points, np.float64).reshape(n, 3), sf_knn_idx=np.zeros((n, 1), np.int64),
                     sf_knn_w=np.ones((n, 1)), ed_points=np.zeros((1, 3)), ed_knn_idx=np.zeros((1, 1), np.int64),
                     tgt_points=np.asarray(tgt_points, np.float64), tgt_norms=np.asarray(tgt_norms, np.float64),
                     index_map=index_map, valid=valid, K=K, H=H, W=W)


def frame_of_scene(sc, points=None):
    """the one-node frame of a ``synth.Scene`` (``points``: another model than the scene's own, e.g. a displaced one)"""
    p = sc.sf_points.astype(np.float64) if points is None else points
    return one_node_frame(p, sc.f64("tgt_points"), sc.f64("tgt_norms"), sc.index_map, sc.valid, sc.K, sc.H, sc.W)


def rotation_quat(axis, angle):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(angle / 2)], np.sin(angle / 2) * a])


def displace(points, angle=0.01, axis=(0.3, -0.5, 0.8), trans=(0.002, -0.001, 0.003)):
    """the model moved rigidly: a rotation by ``angle`` rad about ``axis`` through the origin, then ``trans`` (2, -1, 3 mm)"""
    q = rotation_quat(axis, angle)
    return orc.quat_apply(q[None, :], np.asarray(points, np.float64)) + np.asarray(trans, np.float64)


def displaced_beta(angle=0.004, axis=(-0.2, 0.7, 0.4), trans=(-0.0015, 0.001, 0.002), scale=1.003):
    """a point away from identity for the assembly checks (|q| != 1 on purpose: the Rot term is not at its zero)"""
    return np.concatenate([scale * rotation_quat(axis, angle), trans])


def normalised(beta7):
    b = np.asarray(beta7, np.float64).reshape(7).copy()
    b[:4] /= np.linalg.norm(b[:4])
    return b


def moved(points, norms, Tg):
    """``orc.apply_update`` on the one-node frame: points -> R(q) p + t (the skinned surfels), normals -> normalize(R(q) n)
    (the NODE-normal output with the normals in the place of ``ed_norms``: the surfel-normal output adds the translation
    before it normalises, ``super/nodes.py:207-209``, which a rigid move must not)."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    n = np.asarray(norms, np.float64).reshape(-1, 3)
    beta = np.asarray(Tg, np.float64).reshape(1, 7)
    new_p, _, _, new_n = orc.apply_update(p, n, np.zeros((len(p), 1), np.int64), np.ones((len(p), 1)), np.zeros((1, 3)), n,
                                          beta)
    return new_p, new_n


def run(fr1, opt):
    """(raw beta_g (7,), trace) of the oracle loop"""
    trace = []
    beta = orc.lm(fr1, opt, trace=trace)
    return beta.reshape(7), trace
