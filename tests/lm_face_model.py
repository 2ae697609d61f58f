"""TEST INFRASTRUCTURE: a float64 restatement of the LM path's triangle-area face term (``slm_enable_face``,
include/super_lm.h), built on the public functions of ``oracle/lm_oracle.py``.

The reference has only the first-order form of the term (``super/deform_mesh.py:51-60``); the Gauss-Newton form is this
project's.  For triangle t with node ids (i0, i1, i2): v_a = g_a + beta[i_a, 4:7], e1 = v1 - v0, e2 = v2 - v0, c = e1 x e2,
A = sqrt(|c|^2 + 1e-13) / 2, r_t = lambda (A - A0_t) with A0 the caller's areas; one row with nine non-zeros on the columns
7 i_a + 4..6: dA/dv1 = (e2 x c) / 4A, dA/dv2 = (c x e1) / 4A, dA/dv0 = -(their sum).  The weight multiplies the residual
(GraphFit multiplies the squared sum: ``mesh_face_weight`` = lambda^2 there gives the same loss).

A *mesh* is a pair ``(tri, areas)``: ``tri`` (3, F) integer node ids, ``areas`` (F,); ``None`` stands for "no mesh".  The
other terms come from a *base*: ``(normal_equations(beta) -> (JtJ, jtl, M), total_loss(beta) -> (loss, M))`` --
``base_plain`` for ICP + ARAP + Rot of ``lm_oracle``, ``base_corr`` / ``base_weighted`` for the combinations.
"""
from types import SimpleNamespace

import numpy as np

from oracle import lm_oracle as orc

EPS = 1e-13


def face_term(fr: orc.Frame, tri, areas, beta, lam, grad=False):
    """residuals ``r`` (F,), the areas ``A`` and, with ``grad``, ``Jrow`` (F, 3, 3): row t, vertex a, d r_t / d v_a"""
    tri = np.asarray(tri, dtype=np.int64)
    beta = np.asarray(beta, dtype=np.float64).reshape(-1, 7)
    v = np.asarray(fr.ed_points, dtype=np.float64) + beta[:, 4:7]
    v0, v1, v2 = v[tri[0]], v[tri[1]], v[tri[2]]
    e1, e2 = v1 - v0, v2 - v0
    c = np.cross(e1, e2)
    A = 0.5 * np.sqrt((c ** 2).sum(1) + EPS)
    out = SimpleNamespace(tri=tri, A=A, r=lam * (A - np.asarray(areas, dtype=np.float64)))
    if grad:
        g1 = np.cross(e2, c) / (4.0 * A)[:, None]
        g2 = np.cross(c, e1) / (4.0 * A)[:, None]
        out.Jrow = lam * np.stack([-(g1 + g2), g1, g2], axis=1)
    return out


def face_loss(fr, mesh, beta, lam):
    """(sum r^2, triangle count); (0, 0) without a mesh"""
    if mesh is None or np.asarray(mesh[0]).shape[1] == 0:
        return 0.0, 0
    t = face_term(fr, mesh[0], mesh[1], beta, lam)
    return float((t.r ** 2).sum()), len(t.r)


def face_jacobian(fr, mesh, beta, lam):
    """dense (F, P) Jacobian of the term and its residuals"""
    t = face_term(fr, mesh[0], mesh[1], beta, lam, grad=True)
    F = len(t.r)
    Jd = np.zeros((F, 7 * fr.J))
    rows = np.arange(F)
    for a in range(3):
        for i in range(3):
            np.add.at(Jd, (rows, 7 * t.tri[a] + 4 + i), t.Jrow[:, a, i])
    return Jd, t.r


def face_system(fr, mesh, beta, lam):
    """the term's own (JtJ, jtl = -Jt r)"""
    P = 7 * fr.J
    if mesh is None or np.asarray(mesh[0]).shape[1] == 0:
        return np.zeros((P, P)), np.zeros(P)
    Jd, r = face_jacobian(fr, mesh, beta, lam)
    return Jd.T @ Jd, -Jd.T @ r


# ---- the other terms ---------------------------------------------------------------------------------------------------
def base_plain(fr, opt):
    return (lambda beta: orc.normal_equations(fr, beta, opt)), (lambda beta: orc.total_loss(fr, beta, opt))


def base_corr(fr, opt, targets, mode, lam_corr):
    import lm_corr_model as lcm
    return ((lambda beta: lcm.normal_equations_with_corr(fr, beta, opt, targets, mode, lam_corr)),
            (lambda beta: lcm.total_loss_with_corr(fr, beta, opt, targets, mode, lam_corr)))


def base_weighted(fr, opt, sem, seg_mode, pp_max=0.0):
    import lm_weight_model as lwm
    return ((lambda beta: lwm.normal_equations(fr, sem, beta, opt, seg_mode, pp_max)),
            (lambda beta: lwm.total_loss(fr, sem, beta, opt, seg_mode, pp_max)))


def normal_equations_with_face(fr, beta, opt, mesh, lam, base=None):
    """dense JtJ, jtl = -Jt r and the ICP match count of the base terms plus the face term"""
    ne, _ = base if base is not None else base_plain(fr, opt)
    JtJ, jtl, M = ne(beta)
    A, b = face_system(fr, mesh, beta, lam)
    return JtJ + A, np.asarray(jtl).reshape(-1) + b, M


def total_loss_with_face(fr, beta, opt, mesh, lam, base=None):
    _, tl = base if base is not None else base_plain(fr, opt)
    s, M = tl(beta)
    return s + face_loss(fr, mesh, beta, lam)[0], M


def lm_with_face(fr, opt, mesh, lam, u=10.0, v=7.5, minimal_loss=1e10, trace=None, base=None):
    """the loop of ``lm_oracle.lm`` with the face term in the normal equations and in the loss"""
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (fr.J, 1))
    best = beta.copy()
    for it in range(opt.num_optimize_iterations):
        JtJ, jtl, M = normal_equations_with_face(fr, beta, opt, mesh, lam, base)
        try:
            delta = orc.solve_damped(JtJ, jtl, u).reshape(-1, 7)
        except np.linalg.LinAlgError:
            if trace is not None:
                trace.append(dict(it=it, status="solver_failed", u=u))
            break
        beta = beta + delta
        loss, Mn = total_loss_with_face(fr, beta, opt, mesh, lam, base)
        u_used, accepted, best_before = u, True, minimal_loss
        if opt.phase == "test":
            if loss < minimal_loss:
                minimal_loss = loss
                u /= v
                best = beta.copy()
            else:
                accepted = False
                u *= v
                beta = best.copy()
        if trace is not None:
            trace.append(dict(it=it, loss=loss, u=u_used, accepted=accepted, M_grad=M, M_loss=Mn, beta=beta.copy(),
                              delta=delta.copy(), minimal_loss=best_before))
    return beta


def decision_margins(trace):
    """|loss - minimal_loss| / |minimal_loss| of every iteration: how far its accept decision is from a tie"""
    return np.array([abs(t["loss"] - t["minimal_loss"]) / abs(t["minimal_loss"]) for t in trace])


def visible_weight(fr, mesh, beta, opt, ratio=1.0):
    """lambda at which the largest face entry of J^T J is ``ratio`` times the largest entry of the data term's: the term is
    lost beside the data term at weight 1 (areas 2e-2 m^2 on the 0.2 m node grids of the test scenes, ~1e-5 m^2 at tissue scale),
    so the GPU tests weigh it from the model"""
    only_data = SimpleNamespace(**vars(opt))
    only_data.mesh_arap = only_data.mesh_rot = False
    Ad = orc.normal_equations(fr, beta, only_data)[0]
    Af = face_system(fr, mesh, beta, 1.0)[0]
    return float(np.sqrt(ratio * np.abs(Ad).max() / np.abs(Af).max()))


def scene_mesh(sc):
    """(tri (3, F) int64, areas (F,) float64) of a synth Scene"""
    return np.asarray(sc.ed_triangles, dtype=np.int64), np.asarray(sc.ed_triangle_areas, dtype=np.float64)


def random_beta(J, seed, rot=0.01, trans=0.003):
    rng = np.random.default_rng(seed)
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (J, 1))
    return beta + np.concatenate([rng.normal(0, rot, (J, 4)), rng.normal(0, trans, (J, 3))], axis=1)
