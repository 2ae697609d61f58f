"""TEST INFRASTRUCTURE: scenes, term inputs and model results for the opt-in terms of the rigid stage (slm_rigid_set_terms:
flow-correspondence rows and per-residual data weights).  No GPU at import; shared by tests/test_rigid_terms_model.py (CPU: the
facts about these fixtures) and tests/test_gpu_rigid_terms.py (GPU: the library against the model).

No new physics: the model is ``lm_weight_model.normal_equations / total_loss / lm(..., corr=(targets, mode, lam))`` on the
one-node frame of ``rigid_model.frame_of_scene`` with ``rigid_model.rigid_opt()``.
"""
import dataclasses
import functools

import numpy as np

import lm_corr_model as lcm
import lm_weight_model as lwm
import rigid_model as rm
from super_amd import synth

WEIGHTS = {"none": (0, 0.0), "hard": (1, 0.0), "soft": (2, 0.0), "trunc": (0, 2e-5)}
FLOW_SEED, FLOW_AMP = 11, (2.0, 1.5)
ISSUE_MOTION = dict(angle=0.004, axis=(0, 0, 1), trans=(0.004, -0.003, 0.0005))


def issue_scene(tgt_holes=0.01):
    return synth.make_scene(N=1200, J=40, H=60, W=80, seed=64, n_neighbors=4, src_border=6, tgt_border=3, tgt_holes=tgt_holes,
                            semantic=True, num_classes=3)


def subset(sc, keep):
    """the scene with the surfels ``keep`` only, their semantic fields included"""
    keep = np.asarray(keep)
    return dataclasses.replace(sc, sf_points=sc.sf_points[keep], sf_norms=sc.sf_norms[keep], sf_knn_idx=sc.sf_knn_idx[keep],
                               sf_knn_w=sc.sf_knn_w[keep], sf_seg=np.asarray(sc.sf_seg)[keep],
                               sf_seg_conf=np.asarray(sc.sf_seg_conf)[keep])


@functools.lru_cache(maxsize=None)
def scene(name):
    """(synth.Scene with semantic fields, model points (N,3) float64: the scene's surfels rigidly displaced)"""
    if name == "issue":                                   # the pan along the surface of the issue's table
        sc = issue_scene()
        return sc, rm.displace(sc.sf_points.astype(np.float64), **ISSUE_MOTION)
    if name == "holes":
        sc = issue_scene(tgt_holes=0.1)
        return sc, rm.displace(sc.sf_points.astype(np.float64), **ISSUE_MOTION)
    if name == "n3000":
        sc = synth.make_scene(N=3000, J=64, H=96, W=128, seed=3, semantic=True, num_classes=3)
    elif name == "big":                                   # a second chunk of the grid-stride walk of k_rg_pass
        sc = synth.make_scene(N=512 * 256 + 300, J=64, H=480, W=640, seed=2, semantic=True, num_classes=3)
    elif name in ("n1", "n65", "n257"):
        sc, p = scene("n3000")
        n = int(name[1:])
        pick = np.linspace(0, sc.N - 1, n).astype(np.int64) if n > 1 else np.array([1234])
        return subset(sc, pick), p[pick]
    else:
        raise KeyError(name)
    return sc, rm.displace(sc.sf_points.astype(np.float64))


def points(name, f64=True):
    p = scene(name)[1]
    return p if f64 else p.astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def frame(name, f64=True):
    return rm.frame_of_scene(scene(name)[0], points(name, f64))


def off_labels(name):
    """a label per surfel that no target ever wins (the class count itself): the hard weight is 0 wherever it is evaluated"""
    sc = scene(name)[0]
    return np.full(sc.N, np.asarray(sc.tgt_seg_conf).shape[1], np.int64)


@functools.lru_cache(maxsize=None)
def sem(name, labels="own"):
    s = lwm.sem_of(scene(name)[0])
    if labels == "off":
        s.sf_seg = off_labels(name)
    return s


@functools.lru_cache(maxsize=None)
def flow(name):
    sc = scene(name)[0]
    return synth.smooth_flow(sc.H, sc.W, FLOW_SEED, amp=FLOW_AMP)


@functools.lru_cache(maxsize=None)
def targets(name, f64=True, kind="flow"):
    """(o (N,3), n (N,3), valid (N,) bool).  kind: "flow" -- ``lcm.targets_from_flow`` of the model as it stands; "exact" --
    every third surfel, its true place (the undisplaced surfel and its normal); "none" -- all invalid; ("one", i) -- the
    exact target of surfel i alone (i < 0 counts from the end)"""
    sc = scene(name)[0]
    if kind == "flow":
        return lcm.targets_from_flow(frame(name, f64), flow(name))
    o = sc.sf_points.astype(np.float64).copy()
    n = sc.sf_norms.astype(np.float64).copy()
    valid = np.zeros(sc.N, bool)
    if kind == "exact":
        valid[::3] = True
    elif kind != "none":
        valid[kind[1]] = True
    o[~valid], n[~valid] = 0.0, 0.0
    return o, n, valid


def opt(n_iter=10, phase="test"):
    return rm.rigid_opt(num_optimize_iterations=n_iter, phase=phase)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    f64: bool = True
    mode: int = 1
    weights: str = "none"
    lam: float = 1.0
    kind: object = "flow"
    u: float = 10.0        # LM(..., u=, v=): the damping schedule of the loop
    v: float = 7.5
    labels: str = "own"    # "off": off_labels

    @property
    def id(self):
        k = self.kind if isinstance(self.kind, str) else "one%d" % self.kind[1]
        return f"{self.name}-{'f64' if self.f64 else 'f32'}-m{self.mode}-{self.weights}-{k}-l{self.lam:g}-u{self.u:g}"

    @property
    def seg(self):
        return WEIGHTS[self.weights]

    @property
    def corr(self):
        return None if self.mode == 0 else (targets(self.name, self.f64, self.kind), self.mode, self.lam)


# The loop cases of the GPU tests: every weight, both modes, both state dtypes, one partial / two / twelve.  The rigid problem
# converges within a few iterations at the default damping (u = 10, v = 7.5), after which accept / reject compares losses that
# agree to 1e-13: no decision a device and the model must share.  So the smooth cases run at u = 1e4, v = 2 (damped all the
# way: every step lowers the loss by more than 1e-5 of it) and the truncated ones, whose weights keep switching, at the
# default, where they bring the rejects.  tests/test_rigid_terms_model.py asserts the margins.
SLOW = dict(u=1e4, v=2.0)
LOOP_CASES = [Case("n3000", True, 1, "hard", 1.0, **SLOW), Case("n3000", False, 2, "soft", 1.0, **SLOW),
              Case("n65", True, 2, "none", 1.0, **SLOW), Case("issue", True, 1, "none", 3.0, "exact", **SLOW),
              Case("n257", True, 1, "trunc", 1.0), Case("n3000", True, 1, "trunc", 0.3)]
TRAIN_CASE = Case("n3000", True, 1, "soft", 1.0, **SLOW)
# selection edges run as loops: no valid correspondence at all (equals the plain stage: PLAIN_CASE), every matched surfel at
# hard weight 0 beside valid correspondences, one surfel
NONE_CASE = Case("n3000", True, 1, "none", 1.0, "none", **SLOW)
PLAIN_CASE = Case("n3000", True, 0, "none", 0.0, "none", **SLOW)
OFF_CASE = Case("n257", True, 1, "hard", 1.0, labels="off", **SLOW)
ONE_SURFEL_CASE = Case("n1", True, 1, "none", 1.0, ("one", 0), **SLOW)
EDGE_LOOP_CASES = [NONE_CASE, PLAIN_CASE, OFF_CASE, ONE_SURFEL_CASE]
# the known-warp figures of the CPU test: the moved model's RMS distance (mm) from its true place after ten iterations
KNOWN_WARP = {"before": 5.30, "plain": 18.60, "pp_w1": 3.75, "pp_w3": 0.75, "pp_w10": 0.08, "plane_w1": 13.7}


def system(c: Case, beta):
    """(JtJ, jtl, M, loss, (data sum, M, corr sum, kept)) of the model at ``beta`` (7,)"""
    fr, s, o = frame(c.name, c.f64), sem(c.name, c.labels), opt()
    b = np.asarray(beta, np.float64).reshape(1, 7)
    A, g, M = lwm.normal_equations(fr, s, b, o, *c.seg, corr=c.corr)
    loss, Ml = lwm.total_loss(fr, s, b, o, *c.seg, corr=c.corr)
    assert M == Ml
    d = lwm.data_loss(fr, s, b, o.sf_point_plane_weight, *c.seg)
    cl = lcm.corr_loss(fr, b, *c.corr) if c.corr is not None else (0.0, 0)
    return A, g, M, loss, (d[0], d[1], cl[0], cl[1])


@functools.lru_cache(maxsize=None)
def loop(c: Case, n_iter, phase="test"):
    """(raw beta (7,), trace, visited) of the model loop; ``visited`` holds, per point the loop evaluated, the weights record
    of ``lwm.weights`` there (the conditions of ``lwm.check_conditions`` are asserted by the callers)"""
    fr, s = frame(c.name, c.f64), sem(c.name, c.labels)
    trace, visited = [], []
    beta = lwm.lm(fr, s, opt(n_iter, phase), *c.seg, corr=c.corr, u=c.u, v=c.v, trace=trace,
                  on_beta=lambda b: visited.append(lwm.weights(fr, s, b, *c.seg)))
    return beta.reshape(7), trace, visited


def rms_mm(name, beta, f64=True):
    """RMS distance (mm) of the model moved by ``beta`` (quaternion normalised) from its true place"""
    sc = scene(name)[0]
    moved, _ = rm.moved(points(name, f64), sc.sf_norms.astype(np.float64), rm.normalised(beta))
    return 1e3 * float(np.sqrt(((moved - sc.sf_points.astype(np.float64)) ** 2).sum(1).mean()))
