"""TEST INFRASTRUCTURE: a float64 restatement of the per-residual weights of the LM path's point-to-plane term
(``slm_enable_data_weights``, include/super_lm.h), built on ``oracle.lm_oracle.data_term`` and ``oracle.graphfit_oracle.jsd``.

For every surfel i of the match set of ``data_term`` (unchanged), e = T_i(beta) - o, s_i = (n.e)^2 without lambda:
  seg_mode 1 / 2: conf = sum over the residual's four taps of wv_t tgt_seg_conf[row_t, :], q = softmax(conf); hard
                  w_i = [sf_seg[i] == argmax q] (first maximum), soft w_i = exp(-0.1 JSD(sf_seg_conf[i], q)); pp_max ignored
  seg_mode 0, pp_max > 0: w_i = [s_i < pp_max]
The weights are constants of the linearisation: rows and residuals are scaled by sqrt(w_i) with w_i at beta; the loss is
sum w_i r_i^2 with w_i fresh where it is evaluated.  Counts stay the match set's.
"""
from types import SimpleNamespace

import numpy as np
import torch

import lm_corr_model as lcm
from oracle import graphfit_oracle as gfo
from oracle import lm_oracle as orc

SEG = {None: 0, "hard": 1, "soft": 2}


def sem_of(sc):
    """the semantic inputs of a Scene as the library is given them"""
    return SimpleNamespace(sf_seg=np.asarray(sc.sf_seg).astype(np.int64), sf_seg_conf=np.asarray(sc.sf_seg_conf, dtype=np.float32),
                           tgt_seg_conf=np.asarray(sc.tgt_seg_conf, dtype=np.float32))


def weights(fr: orc.Frame, sem, beta, seg_mode=0, pp_max=0.0):
    """``w`` (M,) of the matched surfels ``t.match`` at beta, with what the conditions of the GPU tests need: ``gap`` the
    top-two gap of conf (inf with one class or seg_mode 0), ``s`` the squared residuals without lambda; ``t`` is
    ``data_term(fr, beta, 1.0)``"""
    t = orc.data_term(fr, beta, 1.0)
    sel, rows = t.match, t.taps
    s = t.r ** 2
    out = SimpleNamespace(t=t, s=s, gap=np.full(len(sel), np.inf), conf=None)
    if seg_mode == 0:
        out.w = (s < pp_max).astype(np.float64) if pp_max > 0.0 else np.ones(len(sel))
        return out
    v, u = t.v[sel], t.u[sel]
    fv, cv, fu, cu = np.floor(v), np.ceil(v), np.floor(u), np.ceil(u)
    nb, mb = np.stack([fv, fv, cv, cv], -1), np.stack([fu, cu, fu, cu], -1)
    an = np.maximum(1.0 - np.abs(nb - v[:, None]), 0.0)
    am = np.maximum(1.0 - np.abs(mb - u[:, None]), 0.0)
    wv = an * am
    tc = sem.tgt_seg_conf.astype(np.float64)
    conf = np.zeros((len(sel), tc.shape[1]))
    for k in range(4):                                          # tap order, as the residual's own sum
        conf += tc[rows[:, k]] * wv[:, k:k + 1]
    out.conf = conf
    if conf.shape[1] > 1:
        srt = np.sort(conf, 1)
        out.gap = srt[:, -1] - srt[:, -2]
    q = torch.from_numpy(conf).softmax(1)
    if seg_mode == 1:
        out.w = (sem.sf_seg[sel] == q.argmax(1).numpy()).astype(np.float64)
    elif seg_mode == 2:
        p = torch.from_numpy(sem.sf_seg_conf.astype(np.float64)[sel])
        out.w = torch.exp(-0.1 * gfo.jsd(p, q)).numpy()
    else:
        raise ValueError(seg_mode)
    return out


def weights_all(fr, sem, beta, seg_mode=0, pp_max=0.0):
    """(N,) weights in surfel order, 0 for unmatched surfels: what ``slm_data_weights`` writes"""
    ww = weights(fr, sem, beta, seg_mode, pp_max)
    w = np.zeros(len(fr.sf_points))
    w[ww.t.match] = ww.w
    return w, ww


def check_conditions(ww, seg_mode, pp_max):
    """the conditions under which a device and this model must take the same side: no matched surfel with a top-two gap of
    conf below 1e-9 (hard), none with |s / pp_max - 1| below 1e-9 (truncation).  No surfel is excluded: a scene that
    violates one is not used."""
    if seg_mode == 1 and len(ww.gap):
        assert ww.gap.min() >= 1e-9, ww.gap.min()
    if seg_mode == 0 and pp_max > 0.0 and len(ww.s):
        assert np.abs(ww.s / pp_max - 1.0).min() >= 1e-9


def weighted_term(fr, sem, beta, lam, seg_mode=0, pp_max=0.0, grad=False, w_fixed=None):
    """``data_term`` with r and Jrow scaled by sqrt(w); ``w_fixed``: weights held at these values (finite differences)"""
    t = orc.data_term(fr, beta, lam, grad=grad)
    w = weights(fr, sem, beta, seg_mode, pp_max).w if w_fixed is None else w_fixed
    sw = np.sqrt(w)
    t.w = w
    t.r = t.r * sw
    if grad:
        t.Jrow = t.Jrow * sw[:, None, None]
    return t


def data_loss(fr, sem, beta, lam, seg_mode=0, pp_max=0.0):
    """(sum w_i r_i^2, match count)"""
    t = orc.data_term(fr, beta, lam)
    w = weights(fr, sem, beta, seg_mode, pp_max).w
    return float((w * t.r ** 2).sum()), len(t.r)


def data_jacobian(fr, sem, beta, lam, seg_mode=0, pp_max=0.0, w_fixed=None):
    import scipy.sparse as sp
    t = weighted_term(fr, sem, beta, lam, seg_mode, pp_max, grad=True, w_fixed=w_fixed)
    M, K = t.nodes.shape
    rows = np.repeat(np.arange(M), 7 * K)
    cols = (7 * t.nodes[:, :, None] + np.arange(7)[None, None, :]).reshape(-1)
    return sp.coo_matrix((t.Jrow.reshape(-1), (rows, cols)), shape=(M, 7 * fr.J)).tocsr(), t.r


def _no_data(opt):
    o = SimpleNamespace(**vars(opt))
    o.sf_point_plane = False
    return o


def normal_equations(fr, sem, beta, opt, seg_mode=0, pp_max=0.0, corr=None):
    """dense JtJ, jtl = -Jt r and the match count: the weighted data term, ARAP and Rot of ``lm_oracle`` and, with
    ``corr = (targets, mode, lam)``, the flow-correspondence term of ``lm_corr_model``"""
    JtJ, jtl, _ = orc.normal_equations(fr, beta, _no_data(opt))
    Jd, r = data_jacobian(fr, sem, beta, opt.sf_point_plane_weight, seg_mode, pp_max)
    JtJ = JtJ + (Jd.T @ Jd).toarray()
    jtl = jtl - Jd.T @ r
    if corr is not None:
        Jc, rc = lcm.corr_jacobian(fr, beta, *corr)
        JtJ = JtJ + (Jc.T @ Jc).toarray()
        jtl = jtl - Jc.T @ rc
    return JtJ, jtl, Jd.shape[0]


def total_loss(fr, sem, beta, opt, seg_mode=0, pp_max=0.0, corr=None):
    s, _ = orc.total_loss(fr, beta, _no_data(opt))
    d, M = data_loss(fr, sem, beta, opt.sf_point_plane_weight, seg_mode, pp_max)
    s += d
    if corr is not None:
        s += lcm.corr_loss(fr, beta, *corr)[0]
    return s, M


def lm(fr, sem, opt, seg_mode=0, pp_max=0.0, corr=None, u=10.0, v=7.5, minimal_loss=1e10, trace=None, on_beta=None):
    """the loop of ``lm_oracle.lm`` with the weighted term; ``on_beta(beta)`` is called at every point the term is
    evaluated at (the tests assert their conditions there)"""
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (fr.J, 1))
    best = beta.copy()
    for it in range(opt.num_optimize_iterations):
        if on_beta:
            on_beta(beta)
        JtJ, jtl, M = normal_equations(fr, sem, beta, opt, seg_mode, pp_max, corr)
        try:
            delta = orc.solve_damped(JtJ, jtl, u).reshape(-1, 7)
        except np.linalg.LinAlgError:
            if trace is not None:
                trace.append(dict(it=it, status="solver_failed", u=u))
            break
        beta = beta + delta
        if on_beta:
            on_beta(beta)
        loss, Mn = total_loss(fr, sem, beta, opt, seg_mode, pp_max, corr)
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
