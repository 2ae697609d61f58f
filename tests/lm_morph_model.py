"""TEST INFRASTRUCTURE: a float64 restatement of the LM path's semantic boundary-morph term (``slm_enable_morph``,
include/super_lm.h), built on the public functions of ``oracle/lm_oracle.py`` (skinning, Jacobian rows, the loop) and on
``graphfit_oracle.edge_points`` (the boundary lists).

The reference has only the first-order form of the term (``super/deform_mesh.py:126-194``, ``graphfit_oracle.bn_morph``); the
Gauss-Newton form is this project's.  With T = T_i(beta) the skinned surfel i:

1. projection: Ze = T.z + 1e-8, x = T.x fx / Ze + cx, y = T.y fy / Ze + cy (fx .. cy the frame's float32 values widened);
2. surfel i is a *candidate* when argmax_c grid_sample(img_seg_conf)(x, y) != sf_seg[i] (bilinear, zero padding,
   align_corners=False, first maximum), the normalised coordinates are strictly inside (-1, 1) and its class has at least two
   boundary pixels;
3. e1, e2 = the two nearest boundary pixels of its own class in (distance, list position) order, d1 <= d2 the squared
   distances; *kept* when not (sqrt(d1) > dte or sqrt(d2) > dte), dte = min(x, y, W - x, H - y), and l_i = (d1 + d2) / 2 > 15;
4. n = kept surfels; loss = lambda^2 / n sum_kept l_i, nothing when n = 0 (the one departure: the reference's mean over an
   empty selection is NaN);
5. the selection, m_i = (e1 + e2) / 2 and n are constants of the linearisation: two rows per kept surfel,
   r_i = lambda / sqrt(n) ((x, y) - m_i), c = (fx / Ze, 0, -fx T.x / Ze^2) and (0, fy / Ze, -fy T.y / Ze^2), per neighbour k
   lambda / sqrt(n) w_k [c^T dR(q_k)(p - g_k)/dq_k | c].

``sem`` is a namespace ``(C, img_seg (H,W), img_seg_conf (C,H,W) float32, sf_seg (N,))``; ``None`` stands for "no inputs".
The other terms come from a *base*: ``(normal_equations(beta) -> (JtJ, jtl, M), total_loss(beta) -> (loss, M))`` --
``base_plain`` for ICP + ARAP + Rot of ``lm_oracle``, ``base_corr`` / ``base_weighted`` / ``base_face`` for the combinations.
"""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from oracle import graphfit_oracle as gfo
from oracle import lm_oracle as orc

LI_MIN = 15.0
REL = 1e-9


def sem_of(sc, img_seg=None, img_seg_conf=None, sf_seg=None):
    """the term's inputs of a synth Scene (optionally with replaced arrays), with the boundary lists of ``img_seg``"""
    s = SimpleNamespace(C=int(sc.num_classes),
                        img_seg=np.asarray(sc.img_seg if img_seg is None else img_seg, dtype=np.int64),
                        img_seg_conf=np.ascontiguousarray(sc.img_seg_conf if img_seg_conf is None else img_seg_conf, dtype=np.float32),
                        sf_seg=np.asarray(sc.sf_seg if sf_seg is None else sf_seg, dtype=np.int64))
    s.edges = [e.numpy().reshape(-1, 2) for e in gfo.edge_points(s.img_seg, s.C)]
    return s


def intrinsics(fr):
    return tuple(float(np.float32(fr.K[a, b])) for a, b in ((0, 0), (1, 1), (0, 2), (1, 2)))


def project(fr, T):
    fx, fy, cx, cy = intrinsics(fr)
    Ze = T[:, 2] + 1e-8
    return T[:, 0] * fx / Ze + cx, T[:, 1] * fy / Ze + cy, Ze


def sampled_conf(fr, sem, x, y):
    """(N, C) float64 class confidences at the projections, as ``graphfit_oracle.bn_morph`` samples them"""
    sg = torch.from_numpy(np.stack([x / fr.W * 2 - 1, y / fr.H * 2 - 1], 1))
    img = torch.from_numpy(sem.img_seg_conf.astype(np.float64))[None]
    out = F.grid_sample(img, sg[None, :, None, :], mode="bilinear", padding_mode="zeros", align_corners=False)[0, :, :, 0]
    return out.numpy().T, sg.numpy()


def select(fr, sem, beta):
    """the selection at beta: per surfel ``x, y, T, Ze``, ``cand``, ``kept``, ``target`` (N,2), ``li`` (N,) (zeros where not
    kept), and for the candidates the three smallest squared distances ``d`` (N,3; inf where the list is shorter) and ``dte``"""
    beta = np.asarray(beta, dtype=np.float64).reshape(-1, 7)
    T, _ = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, beta)
    x, y, Ze = project(fr, T)
    conf, sg = sampled_conf(fr, sem, x, y)
    new_seg = np.argmax(conf, axis=1)                                  # (first maximum)
    inside = (sg[:, 0] > -1) & (sg[:, 0] < 1) & (sg[:, 1] > -1) & (sg[:, 1] < 1)
    N = len(x)
    cls = sem.sf_seg
    has_list = np.array([0 <= c < sem.C and len(sem.edges[c]) >= 2 for c in cls])
    cand = (new_seg != cls) & inside & has_list
    d = np.full((N, 3), np.inf)
    target, li, kept = np.zeros((N, 2)), np.zeros(N), np.zeros(N, bool)
    dte = np.minimum(np.minimum(np.minimum(x, y), fr.W - x), fr.H - y)
    for c in range(sem.C):
        idx = np.nonzero(cand & (cls == c))[0]
        if not len(idx):
            continue
        E = sem.edges[c]
        dx, dy = x[idx, None] - E[None, :, 0], y[idx, None] - E[None, :, 1]
        d2 = dx * dx + dy * dy
        order = np.argsort(d2, axis=1, kind="stable")[:, :3]
        ds = np.take_along_axis(d2, order, axis=1)
        d[idx, :ds.shape[1]] = ds
        ok = ~((np.sqrt(ds[:, 0]) > dte[idx]) | (np.sqrt(ds[:, 1]) > dte[idx]))
        l = (ds[:, 0] + ds[:, 1]) / 2.0
        k = ok & (l > LI_MIN)
        kept[idx] = k
        li[idx] = np.where(k, l, 0.0)
        target[idx] = np.where(k[:, None], (E[order[:, 0]] + E[order[:, 1]]) / 2.0, 0.0)
    return SimpleNamespace(T=T, x=x, y=y, Ze=Ze, conf=conf, sg=sg, inside=inside, cand=cand, kept=kept, target=target, li=li, d=d,
                           dte=dte, n=int(kept.sum()))


def check_conditions(fr, sem, beta):
    """asserts that a device and this model must take the same side of every decision at beta: all relative margins
    >= 1e-9 -- the top-two gap of the sampled confidences (and the distance of the normalised coordinates from +-1), l_i
    against 15, sqrt(d) against dte, the 2nd against the 3rd nearest squared distance.  An exact tie is decided the same way on
    either side -- of distances by list position, of confidences by the first maximum where the two classes have the same
    four taps -- and only a near-tie is excluded.  No surfel is excluded: a scene or beta that violates one is not used."""
    s = select(fr, sem, beta)
    edge = np.abs(np.abs(s.sg) - 1.0).min()
    assert edge >= REL, ("a projection on the image's edge", edge)
    ins = s.inside
    if sem.C > 1 and ins.any():
        order = np.argsort(s.conf[ins], axis=1, kind="stable")
        top = np.take_along_axis(s.conf[ins], order, axis=1)
        gap = (top[:, -1] - top[:, -2]) / np.maximum(np.abs(top[:, -1]), np.abs(top[:, -2]))
        # an exact tie is resolved by the first maximum on either side when the two classes have the SAME four taps (flat
        # regions of an image: the same products in the same order); only a near-tie, or a tie of unlike taps, is excluded
        tie = np.nonzero(gap == 0.0)[0]
        if len(tie):
            ix = ((s.sg[ins][tie, 0] + 1.0) * fr.W - 1.0) / 2.0
            iy = ((s.sg[ins][tie, 1] + 1.0) * fr.H - 1.0) / 2.0
            x0, y0 = np.floor(ix).astype(np.int64), np.floor(iy).astype(np.int64)
            a, b = order[tie, -1], order[tie, -2]
            for dx in (0, 1):
                for dy in (0, 1):
                    xx, yy = x0 + dx, y0 + dy
                    inb = (xx >= 0) & (xx < fr.W) & (yy >= 0) & (yy < fr.H)
                    xc, yc = np.clip(xx, 0, fr.W - 1), np.clip(yy, 0, fr.H - 1)
                    same = sem.img_seg_conf[a, yc, xc] == sem.img_seg_conf[b, yc, xc]
                    assert (same | ~inb).all(), "class confidences tie on unlike taps"
        assert gap[gap != 0.0].min(initial=1.0) >= REL, ("class confidences nearly tie", gap.min())
    c = s.cand
    if c.any():
        l = (s.d[c, 0] + s.d[c, 1]) / 2.0
        assert np.abs(l / LI_MIN - 1.0).min() >= REL, "l_i on the threshold"
        r = np.abs(np.sqrt(s.d[c, :2]) / s.dte[c, None] - 1.0)
        assert r.min() >= REL, "a boundary pixel as far as the image border"
        d2, d3 = s.d[c, 1], s.d[c, 2]
        fin = np.isfinite(d3) & (d3 != d2)
        if fin.any():
            assert ((d3[fin] - d2[fin]) / d3[fin]).min() >= REL, "2nd and 3rd nearest boundary pixel nearly tie"
    return s


def morph_loss(fr, sem, beta, lam):
    """(lambda^2 / n sum l_i, kept n, candidates); (0, 0, 0) without inputs"""
    if sem is None:
        return 0.0, 0, 0
    s = select(fr, sem, beta)
    return (float(lam * lam / s.n * s.li[s.kept].sum()) if s.n else 0.0), s.n, int(s.cand.sum())


def morph_jacobian(fr, sem, beta, lam, sel=None):
    """dense (2 n, P) Jacobian of the term and its residuals (rows: x then y of a kept surfel), at the selection ``sel``
    (default: the one at beta -- pass a frozen one to differentiate)"""
    beta = np.asarray(beta, dtype=np.float64).reshape(-1, 7)
    if sel is None:
        sel = select(fr, sem, beta)
    idx = np.nonzero(sel.kept)[0]
    n = len(idx)
    P = 7 * fr.J
    if n == 0:
        return np.zeros((0, P)), np.zeros(0)
    T, Jq = orc.skin_points(fr.sf_points, fr.ed_points, fr.sf_knn_idx, fr.sf_knn_w, beta, grad=True)
    x, y, Ze = project(fr, T)
    fx, fy, _, _ = intrinsics(fr)
    Cv = np.zeros((n, 2, 3))
    Cv[:, 0, 0] = fx / Ze[idx]
    Cv[:, 0, 2] = -fx * T[idx, 0] / Ze[idx] ** 2
    Cv[:, 1, 1] = fy / Ze[idx]
    Cv[:, 1, 2] = -fy * T[idx, 1] / Ze[idx] ** 2
    sc = lam / np.sqrt(n)
    r = sc * (np.stack([x[idx], y[idx]], 1) - sel.target[idx]).reshape(-1)
    w = fr.sf_knn_w[idx]
    jq = np.einsum("mri,mkij->mrkj", Cv, Jq[idx])                    # Jq carries w_k already
    jb = w[:, None, :, None] * Cv[:, :, None, :]
    Jrow = sc * np.concatenate([jq, jb], axis=3)                     # (n, 2, K, 7)
    K = w.shape[1]
    Jd = np.zeros((2 * n, P))
    rows = np.repeat(np.arange(2 * n), 7 * K)
    cols = np.broadcast_to(7 * fr.sf_knn_idx[idx][:, None, :, None] + np.arange(7)[None, None, None, :], (n, 2, K, 7)).reshape(-1)
    np.add.at(Jd, (rows, cols), Jrow.reshape(-1))
    return Jd, r


def morph_system(fr, sem, beta, lam):
    """the term's own (JtJ, jtl = -Jt r)"""
    P = 7 * fr.J
    if sem is None:
        return np.zeros((P, P)), np.zeros(P)
    Jd, r = morph_jacobian(fr, sem, beta, lam)
    return Jd.T @ Jd, -Jd.T @ r


# ---- the other terms ---------------------------------------------------------------------------------------------------
def base_plain(fr, opt):
    return (lambda beta: orc.normal_equations(fr, beta, opt)), (lambda beta: orc.total_loss(fr, beta, opt))


def base_corr(fr, opt, targets, mode, lam_corr):
    import lm_corr_model as lcm
    return ((lambda beta: lcm.normal_equations_with_corr(fr, beta, opt, targets, mode, lam_corr)),
            (lambda beta: lcm.total_loss_with_corr(fr, beta, opt, targets, mode, lam_corr)))


def base_weighted(fr, opt, wsem, seg_mode, pp_max=0.0):
    import lm_weight_model as lwm
    return ((lambda beta: lwm.normal_equations(fr, wsem, beta, opt, seg_mode, pp_max)),
            (lambda beta: lwm.total_loss(fr, wsem, beta, opt, seg_mode, pp_max)))


def base_face(fr, opt, mesh, lam_face, base=None):
    import lm_face_model as lfm
    return ((lambda beta: lfm.normal_equations_with_face(fr, beta, opt, mesh, lam_face, base)),
            (lambda beta: lfm.total_loss_with_face(fr, beta, opt, mesh, lam_face, base)))


def normal_equations_with_morph(fr, beta, opt, sem, lam, base=None):
    """dense JtJ, jtl = -Jt r and the ICP match count of the base terms plus the morph term"""
    ne, _ = base if base is not None else base_plain(fr, opt)
    JtJ, jtl, M = ne(beta)
    A, b = morph_system(fr, sem, beta, lam)
    return JtJ + A, np.asarray(jtl).reshape(-1) + b, M


def total_loss_with_morph(fr, beta, opt, sem, lam, base=None):
    _, tl = base if base is not None else base_plain(fr, opt)
    s, M = tl(beta)
    return s + morph_loss(fr, sem, beta, lam)[0], M


def lm_with_morph(fr, opt, sem, lam, u=10.0, v=7.5, minimal_loss=1e10, trace=None, base=None):
    """the loop of ``lm_oracle.lm`` with the term in the normal equations and in the loss.  A trace entry also holds the
    point of its Jacobian pass (``beta_at``), its kept count there (``kept``), the trial point (``beta_trial``) and the kept
    count there (``kept_trial``)."""
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (fr.J, 1))
    best = beta.copy()
    for it in range(opt.num_optimize_iterations):
        at = beta.copy()
        JtJ, jtl, M = normal_equations_with_morph(fr, beta, opt, sem, lam, base)
        try:
            delta = orc.solve_damped(JtJ, jtl, u).reshape(-1, 7)
        except np.linalg.LinAlgError:
            if trace is not None:
                trace.append(dict(it=it, status="solver_failed", u=u))
            break
        beta = beta + delta
        trial = beta.copy()
        loss, Mn = total_loss_with_morph(fr, beta, opt, sem, lam, base)
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
                              delta=delta.copy(), minimal_loss=best_before, beta_at=at, beta_trial=trial,
                              kept=morph_loss(fr, sem, at, lam)[1], kept_trial=morph_loss(fr, sem, trial, lam)[1]))
    return beta


def decision_margins(trace):
    """|loss - minimal_loss| / |minimal_loss| of every iteration: how far its accept decision is from a tie"""
    return np.array([abs(t["loss"] - t["minimal_loss"]) / abs(t["minimal_loss"]) for t in trace])


def visible_weight(fr, sem, beta, opt, ratio=1.0):
    """lambda at which the largest entry of the term's J^T J is ``ratio`` times the largest entry of the data term's: in
    pixel units the term swamps the data term at weight 1, so the GPU tests weigh it from the model"""
    only_data = SimpleNamespace(**vars(opt))
    only_data.mesh_arap = only_data.mesh_rot = False
    Ad = orc.normal_equations(fr, beta, only_data)[0]
    Am = morph_system(fr, sem, beta, 1.0)[0]
    return float(np.sqrt(ratio * np.abs(Ad).max() / np.abs(Am).max()))


def random_beta(J, seed, rot=0.01, trans=0.003):
    rng = np.random.default_rng(seed)
    beta = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (J, 1))
    return beta + np.concatenate([rng.normal(0, rot, (J, 4)), rng.normal(0, trans, (J, 3))], axis=1)
