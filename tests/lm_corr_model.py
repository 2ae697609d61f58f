"""TEST INFRASTRUCTURE: a float64 restatement of the LM path's flow-correspondence term (``slm_enable_corr``,
include/super_lm.h), built on the public functions of ``oracle/lm_oracle.py`` and ``oracle/graphfit_oracle.py``.

The reference has no LM form of the term (``super/LM.py:27-29`` is commented out), so the form is this project's:
per surfel a target point o_i, normal n_i and flag valid_i frozen at the bind; with T_i(beta) the skinned surfel and
lambda the weight, mode 1 'point-point' has r_i = lambda (T_i - o_i) (three rows), mode 2 'point-plane'
r_i = lambda n_i.(T_i - o_i) (one row); no dependence through the projection.  The targets are what
``graphfit_oracle.corr_term`` reads at zero deformation (``sf`` = the undeformed surfels).
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import lm_oracle as orc

MODES = {"point-point": 1, "point-plane": 2}


def shifted_coords(fr: orc.Frame, flow):
    """(u', v') of every surfel: the UNROUNDED projection of ``sf_points`` (Z + 1e-8) moved by the flow sampled there
    like ``graphfit_oracle.corr_term`` does (float32 grid, bilinear, zero padding, align_corners=False)."""
    fx, fy, cx, cy = float(fr.K[0, 0]), float(fr.K[1, 1]), float(fr.K[0, 2]), float(fr.K[1, 2])
    P = torch.from_numpy(np.ascontiguousarray(fr.sf_points, dtype=np.float64))
    Z = P[:, 2] + 1e-8
    u_ = P[:, 0] * fx / Z + cx
    v_ = P[:, 1] * fy / Z + cy
    fl = torch.from_numpy(np.ascontiguousarray(flow, dtype=np.float32)).reshape(1, 2, fr.H, fr.W)
    grid = torch.stack([u_ * 2 / fr.W - 1, v_ * 2 / fr.H - 1], dim=1).view(1, -1, 1, 2).float()
    loc = F.grid_sample(fl, grid, mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, :, 0]
    return (u_ + loc[0]).numpy(), (v_ + loc[1]).numpy()


def targets_from_flow(fr: orc.Frame, flow):
    """(o (N,3), n (N,3), valid (N,) bool): margin 1 on the shifted float coordinates, all four taps mapped (and finite);
    zeros where invalid."""
    u, v = shifted_coords(fr, flow)
    with np.errstate(invalid="ignore"):
        ok = (v >= 1) & (v < fr.H - 2) & (u >= 1) & (u < fr.W - 2)
    cand = np.nonzero(ok)[0]
    o, _, _ = orc.bilinear_lookup(v[cand], u[cand], fr.tgt_points, fr.index_map)
    n, _, _ = orc.bilinear_lookup(v[cand], u[cand], fr.tgt_norms, fr.index_map)
    good = ~(np.isnan(o).any(1) | np.isnan(n).any(1))
    N = len(fr.sf_points)
    O, Nn, valid = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N, bool)
    O[cand[good]], Nn[cand[good]], valid[cand[good]] = o[good], n[good], True
    return O, Nn, valid


def tie_distance(fr: orc.Frame, flow):
    """per surfel the distance (px) of its shifted coordinates from the nearest integer or margin: where it is tiny the
    float32 flow sample may put a device and this model on different sides"""
    u, v = shifted_coords(fr, flow)
    return np.minimum(np.abs(u - np.rint(u)), np.abs(v - np.rint(v)))


def corr_term(fr: orc.Frame, beta, targets, mode, lam, grad=False):
    """residuals r (rows in surfel order, mode 1: x, y, z of a surfel consecutive) and, with ``grad``, the Jacobian
    entries ``Jrow`` (M, R, K, 7) of the R rows of each kept surfel on the columns 7 * nodes[:, k] + 0..6."""
    o, n, valid = targets
    sel = np.nonzero(valid)[0]
    T, Jq = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, beta, grad)
    e = T[sel] - o[sel]
    out = SimpleNamespace(sel=sel, nodes=fr.sf_knn_idx[sel])
    if mode == 1:
        C = np.broadcast_to(np.eye(3), (len(sel), 3, 3))           # (M, R=3, 3): the rows' c vectors
    elif mode == 2:
        C = n[sel][:, None, :]                                       # (M, R=1, 3)
    else:
        raise ValueError(mode)
    out.r = lam * np.einsum("mri,mi->mr", C, e).reshape(-1)
    if grad:
        w = fr.sf_knn_w[sel]                                         # (M, K)
        jq = np.einsum("mri,mkij->mrkj", C, Jq[sel])                 # Jq carries w_k already
        jb = w[:, None, :, None] * C[:, :, None, :]
        out.Jrow = lam * np.concatenate([jq, jb], axis=3)            # (M, R, K, 7)
    return out


def corr_loss(fr, beta, targets, mode, lam):
    t = corr_term(fr, beta, targets, mode, lam)
    return float((t.r ** 2).sum()), len(t.sel)


def corr_jacobian(fr, beta, targets, mode, lam):
    """sparse (rows, P) Jacobian of the term and its residuals"""
    import scipy.sparse as sp
    t = corr_term(fr, beta, targets, mode, lam, grad=True)
    M, R, K, _ = t.Jrow.shape
    rows = np.repeat(np.arange(M * R), 7 * K)
    cols = np.broadcast_to((7 * t.nodes[:, None, :, None] + np.arange(7)[None, None, None, :]), (M, R, K, 7)).reshape(-1)
    return sp.coo_matrix((t.Jrow.reshape(-1), (rows, cols)), shape=(M * R, 7 * fr.J)).tocsr(), t.r


def normal_equations_with_corr(fr, beta, opt, targets, mode, lam):
    """dense JtJ, jtl = -Jt r and the ICP match count of ``lm_oracle.normal_equations`` plus the term"""
    JtJ, jtl, M = orc.normal_equations(fr, beta, opt)
    if targets is not None:
        Jc, r = corr_jacobian(fr, beta, targets, mode, lam)
        JtJ = JtJ + (Jc.T @ Jc).toarray()
        jtl = jtl - Jc.T @ r
    return JtJ, jtl, M


def total_loss_with_corr(fr, beta, opt, targets, mode, lam):
    s, M = orc.total_loss(fr, beta, opt)
    if targets is not None:
        s += corr_loss(fr, beta, targets, mode, lam)[0]
    return s, M


def lm_with_corr(fr, opt, targets, mode, lam, u=10.0, v=7.5, minimal_loss=1e10, trace=None):
    """the loop of ``lm_oracle.lm`` with the extra term in the normal equations and in the loss"""
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (fr.J, 1))
    best = beta.copy()
    for it in range(opt.num_optimize_iterations):
        JtJ, jtl, M = normal_equations_with_corr(fr, beta, opt, targets, mode, lam)
        try:
            delta = orc.solve_damped(JtJ, jtl, u).reshape(-1, 7)
        except np.linalg.LinAlgError:
            if trace is not None:
                trace.append(dict(it=it, status="solver_failed", u=u))
            break
        beta = beta + delta
        loss, Mn = total_loss_with_corr(fr, beta, opt, targets, mode, lam)
        u_used, accepted = u, True
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
                              delta=delta.copy()))
    return beta


def random_beta(J, seed, rot=0.01, trans=0.003):
    rng = np.random.default_rng(seed)
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (J, 1))
    return beta + np.concatenate([rng.normal(0, rot, (J, 4)), rng.normal(0, trans, (J, 3))], axis=1)
