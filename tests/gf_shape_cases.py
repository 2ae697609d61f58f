"""Scenes, case tables and CPU references of the GraphFit shape tests (test_gf_shape_cases.py pins the fixtures on the CPU,
test_gpu_graphfit_shapes.py runs them on the device).  No GPU is touched at import; only ``frames_of`` puts tensors on one.

Why these shapes.  k_gf_data's row pass sums gradient rows in a direct-mapped LDS table of 128 slots keyed by ``node & 127``;
a node that finds its slot taken goes to a global atomic instead.  A 60 x 80 scene with J = 48 can never collide, and a
row-major J = 300 grid does not either: the 256 surfels of a workgroup are neighbours on the image, so the ids they touch lie in
a few short runs.  ``relabel_nodes`` renames the nodes with a random permutation -- the same problem, so the oracle's gradient
is the permuted gradient -- after which every workgroup has ids that share a slot (``fallback_nodes`` counts how many must
lose).  The batches give every slot another N, J and triangle count, with the launch maxima coming from different slots; the
edge sizes sit at the staging round (16), the wave (64) and the workgroup (256) of the kernels.

Tolerances are the project's own: terms rtol 1e-9, gradient atol 1e-9 max(1, max|g_ref|) (test_gpu_graphfit.py), deform_verts
after ten steps atol min(1e-9, 1e-6 step) with step = max|dv_oracle - identity| (1e-9: test_gpu_graphfit.py; 1e-6 step:
test_gpu_graphfit_render_in_run.py, which binds for the small steps of the tiny cases)."""
import dataclasses
import functools

import numpy as np

from helpers import GF_CORR_VARIANTS, GF_SEMANTIC_VARIANTS, torch_frame
from oracle import graphfit_oracle as gfo
from super_amd import synth

SCENE_KW = dict(H=60, W=80, src_border=5, tgt_border=3, tgt_holes=0.01)
GF_TAB = 128            # slots of k_gf_data's LDS gradient table (slm_gf.hip)
BLOCK = 256             # surfels per workgroup


# ---------------------------------------------------------------------------------------------------------------- scene helpers
def relabel_nodes(sc, perm):
    """The same scene with node j renamed perm[j]: a pure renaming (gradient row perm[j] of the result is row j of ``sc``'s)."""
    perm = np.asarray(perm, np.int64)
    assert sorted(perm.tolist()) == list(range(sc.J))

    def rows(a):
        out = np.empty_like(a)
        out[perm] = a
        return out

    return dataclasses.replace(
        sc, ed_points=rows(sc.ed_points), ed_norms=rows(sc.ed_norms), ed_radii=rows(sc.ed_radii), ed_knn_w=rows(sc.ed_knn_w),
        ed_knn_idx=rows(perm[sc.ed_knn_idx]), sf_knn_idx=np.ascontiguousarray(perm[sc.sf_knn_idx]),
        ed_triangles=np.ascontiguousarray(perm[sc.ed_triangles]))


def unpermute_rows(a, perm):
    """(J+1,7) rows of a relabelled scene -> the rows of the original (the global row stays last)."""
    return a[np.concatenate([np.asarray(perm, np.int64), [len(perm)]])]


def fallback_nodes(sf_knn_idx, keep=None):
    """(nodes that must take the global-atomic path whatever the race order, workgroups with at least one): per 256-surfel
    block the distinct ids less the distinct table slots.  ``keep`` (N,) bool: only these surfels add rows (the stable ones)."""
    total = blocks = 0
    for b in range(0, len(sf_knn_idx), BLOCK):
        rows = sf_knn_idx[b:b + BLOCK]
        ids = np.unique(rows if keep is None else rows[keep[b:b + BLOCK]])
        lose = len(ids) - len(np.unique(ids & (GF_TAB - 1)))
        total += lose
        blocks += lose > 0
    return total, blocks


def surfel_perm(N, seed):
    return np.random.default_rng(seed).permutation(N)


def reorder_surfels(sc, p):
    """The same scene with surfel row i taken from row p[i]."""
    kw = {k: np.ascontiguousarray(getattr(sc, k)[p]) for k in ("sf_points", "sf_norms", "sf_knn_idx", "sf_knn_w")}
    if sc.num_classes:
        kw.update(sf_seg=sc.sf_seg[p].copy(), sf_seg_conf=np.ascontiguousarray(sc.sf_seg_conf[p]))
    return dataclasses.replace(sc, **kw)


def shuffle_surfels(sc, seed):
    """The same scene with its surfel rows permuted by ``surfel_perm(N, seed)``: another summation order for the oracle."""
    return reorder_surfels(sc, surfel_perm(sc.N, seed))


@functools.lru_cache(maxsize=None)
def short_list_scene():
    """The semantic 60 x 80 scene with class 2 confined to a 4 x 4 patch of the image: its boundary list is shorter than a wave
    (12 pixels), while its 922 surfels are all candidates of the morphing term.  make_scene orders the surfels by image row,
    which spreads a class (a vertical band) over every workgroup, about 100 candidates in each; the surfels are therefore
    sorted by class here (stably: a reordering, to which the terms are indifferent), so that class 2 is contiguous and two
    whole workgroups hold 256 candidates each."""
    sc = synth.make_scene(N=3000, J=48, seed=23, semantic=True, **SCENE_KW)
    conf = sc.img_seg_conf.copy()
    lo, hi = conf.min() - 5.0, conf.max() + 5.0
    conf[2] = lo
    conf[2, 28:32, 38:42] = hi
    conf = np.ascontiguousarray(conf, dtype=np.float32)
    valid_map = sc.valid.reshape(sc.H, sc.W)
    tconf = synth._softmax(conf.astype(np.float64), 0).transpose(1, 2, 0)[valid_map]
    sc = dataclasses.replace(sc, img_seg_conf=conf, img_seg=np.argmax(conf, axis=0).astype(np.int64),
                             tgt_seg_conf=np.ascontiguousarray(tconf.astype(np.float32)))
    return reorder_surfels(sc, np.argsort(sc.sf_seg, kind="stable"))


# ------------------------------------------------------------------------------------------------------------------- the cases
@dataclasses.dataclass(frozen=True)
class Case:
    """One frame and its options: a ``make_scene`` on 60 x 80 (or the short-list scene), the node relabelling, a flow, the
    stability mask and the option tag of ``opt_of``."""
    tag: str
    N: int
    J: int
    K: int
    seed: int
    relabel: bool = False
    semantic: bool = False
    flow: bool = False
    mask: str = "all"          # "all" stable, "random" (10 % unstable) or "groups" (a workgroup, a wave and 16-groups unstable)
    short_list: bool = False

    @property
    def id(self):
        extra = "".join(s for s, on in (("-relabel", self.relabel), ("-sem", self.semantic), ("-flow", self.flow),
                                        ("-short", self.short_list)) if on)
        return f"{self.tag}-N{self.N}-J{self.J}-K{self.K}{extra}" + ("" if self.mask == "all" else "-" + self.mask)


RELABEL_SEED = 1


def relabel_perm(J):
    return np.random.default_rng(RELABEL_SEED).permutation(J)


@functools.lru_cache(maxsize=None)
def _scene(N, J, K, seed, relabel, semantic, flow, short_list):
    if short_list:
        return short_list_scene()
    sc = synth.make_scene(N=N, J=J, seed=seed, n_neighbors=K, n_ed_neighbors=min(4, J - 1), semantic=semantic, **SCENE_KW)
    if relabel:
        sc = relabel_nodes(sc, relabel_perm(J))
    if flow:
        sc = dataclasses.replace(sc, flow=synth.smooth_flow(sc.H, sc.W, seed, amp=(2.5, 1.8)))
    return sc


def scene_of(case, relabel=None):
    """The case's scene (shared, do not modify); ``relabel=False``: its row-major original."""
    return _scene(case.N, case.J, case.K, case.seed, case.relabel if relabel is None else relabel, case.semantic, case.flow,
                  case.short_list)


def stable_of(case):
    """The case's stability mask (N,) bool, or None: every surfel stable."""
    if case.mask == "all":
        return None
    if case.mask == "random":
        return np.random.default_rng(100 + case.seed).uniform(size=case.N) > 0.1
    i = np.arange(case.N)
    return ~(((i >= 256) & (i < 512)) | ((i >= 576) & (i < 640)) | ((i // 16) % 3 == 0))


def perturbed_dv(case):
    """deform_verts away from identity: the perturbation of test_gradient_at_random_point_vs_autograd_oracle."""
    rng = np.random.default_rng(200 + case.seed)
    dv = np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (case.J + 1, 1))
    return dv + np.concatenate([rng.normal(0, 0.01, (case.J + 1, 4)), rng.normal(0, 0.003, (case.J + 1, 3))], axis=1)


def opt_of(tag, **kw):
    """Options by tag: "sgd", "adam", "adamface" (Adam + the face term), the Semantic-SuPer variants of helpers
    ("soft", "morph", "clip", ...) and the flow-correspondence variants ("corr", ...)."""
    if tag in GF_SEMANTIC_VARIANTS:
        o = gfo.default_opt(**GF_SEMANTIC_VARIANTS[tag], **kw)
        o.num_classes = 3
    elif tag in GF_CORR_VARIANTS:
        o = gfo.default_opt(**GF_CORR_VARIANTS[tag], **kw)
    else:
        o = gfo.default_opt(**dict(sgd=dict(optimizer="SGD"), adam=dict(optimizer="Adam"),
                                   adamface=dict(optimizer="Adam", mesh_face=True))[tag], **kw)
    o.deform_udpate_method = "super_edg"
    return o


def problem_of(case, sc=None):
    return gfo.Problem(scene_of(case) if sc is None else sc, stable=stable_of(case))


@functools.lru_cache(maxsize=None)
def oracle_final(case):
    """deform_verts (J+1,7) after the ten steps of gfo.graphfit (shared, do not modify)."""
    out = gfo.graphfit(problem_of(case), opt_of(case.tag))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def oracle_grad(case):
    """(terms dict of floats with "_matched" etc., loss, gradient (J+1,7) with the global row / J) of gfo.total_loss at
    ``perturbed_dv`` by torch autograd, and the morphing term's per-class (class, list length, candidates, kept)."""
    return oracle_grad_at(case, perturbed_dv(case))


def oracle_grad_at(case, dv0, sc=None):
    import torch
    pb = problem_of(case, sc)
    dvt = torch.from_numpy(np.array(dv0)).requires_grad_(True)
    loss, terms = gfo.total_loss(pb, dvt, opt_of(case.tag))
    g, = torch.autograd.grad(loss, dvt)
    g = g.clone()
    g[-1] /= case.J
    t = {k: (float(v.detach()) if torch.is_tensor(v) else v) for k, v in terms.items()}
    return t, float(loss.detach()), g.numpy(), getattr(pb, "morph_stats", None)


def step_of(dv):
    """max|dv - identity|: the size of the update the ten steps made."""
    return float(np.abs(dv - np.eye(1, 7)).max())


def dv_atol(case):
    """The bound on deform_verts after ten steps: min(1e-9, 1e-6 step)."""
    return min(1e-9, 1e-6 * step_of(oracle_final(case)))


# A. table collisions: the relabelled J = 300 scene at a num_neighbors of every entry-lane layout of the row pass
COLLISION_KS = (2, 4, 8)
COLLISION = [Case(tag, 3000, 300, K, 21, relabel=True, mask="random") for K in COLLISION_KS for tag in ("adamface", "clip")]
COLLISION.append(Case("soft", 3000, 300, 4, 21, relabel=True, semantic=True, mask="random"))

# B. ragged batches: (N, J) per slot; the largest N is in slot 0, the largest J and triangle count in slot 1
BATCH_SLOTS = ((3000, 12, False), (16, 300, True), (2100, 140, False), (257, 12, False))
BATCH_VARIANTS = (("sgd", 4), ("adamface", 4), ("soft", 4), ("corr", 4), ("adam", 6))


def batch_cases(tag, K):
    return [Case(tag, N, J, K, 50 + 10 * s + K, relabel=rl, semantic=tag in GF_SEMANTIC_VARIANTS, flow=tag in GF_CORR_VARIANTS)
            for s, (N, J, rl) in enumerate(BATCH_SLOTS)]


# C. edge sizes
EDGE = [Case("adamface", N, J, K, 70 + n) for n, (N, J, K) in
        enumerate(((1, 8, 8), (15, 6, 4), (17, 12, 1), (255, 12, 3), (257, 12, 5), (16, 130, 4)))]
EDGE.append(Case("adamface", 3000, 48, 4, 21, mask="groups"))

# E. a boundary list shorter than a wave, workgroups of 256 candidates
SHORT_LIST = [Case(tag, 3000, 48, 4, 23, semantic=True, short_list=True) for tag in ("soft", "morph")]

# D. float32 state
F32_SINGLE = [c for c in COLLISION if c.K == 4 and c.tag != "soft"]
F32_BATCH = ("soft", 4)

TEN_STEP_CASES = COLLISION + [c for v in BATCH_VARIANTS for c in batch_cases(*v)] + EDGE + SHORT_LIST


# --------------------------------------------------------------------------------------------------------------- device frames
class FlowModels:
    """``models`` of GraphFit for frames with a recorded flow: ``optical_flow(src.rgb, color)`` returns the flow of the frame
    whose ``src.rgb`` it is handed."""

    def __init__(self):
        self.by_rgb = {}
        self.calls = 0

    def add(self, rgb, flow):
        self.by_rgb[id(rgb)] = (rgb, flow)

    def optical_flow(self, a, b):
        self.calls += 1
        return self.by_rgb[id(a)][1]


def frames_of(sc, models=None, stable=None):
    """``(inputs, sf, new_data)`` of a scene on the device as GraphFit reads them: helpers.torch_frame plus the node triangles,
    the Semantic-SuPer inputs when the scene has them, the stability mask and -- ``models``: a FlowModels -- the scene's flow."""
    import torch
    sf, inputs, new_data = torch_frame(sc)
    sf.ED_nodes.triangles = torch.from_numpy(sc.ed_triangles).cuda()
    sf.ED_nodes.triangles_areas = torch.from_numpy(sc.ed_triangle_areas).cuda().double()
    if sc.num_classes:
        sf.seg = torch.from_numpy(sc.sf_seg).cuda()
        sf.seg_conf = torch.from_numpy(sc.sf_seg_conf).cuda().double()
        new_data.seg_conf = torch.from_numpy(sc.tgt_seg_conf).cuda().double()
        inputs[("seg_conf", 0)] = torch.from_numpy(sc.img_seg_conf).cuda().double()[None]
        inputs[("seg", 0)] = torch.from_numpy(sc.img_seg).cuda()[None, None]
    if stable is not None:
        sf.isStable = torch.from_numpy(np.asarray(stable, bool)).cuda()
    if models is not None and sc.flow is not None:
        sf.rgb = torch.zeros(1, 3, sc.H, sc.W, device="cuda")
        models.add(sf.rgb, torch.from_numpy(sc.flow).cuda())
    return inputs, sf, new_data


def case_frame(case, models=None, sc=None):
    return frames_of(scene_of(case) if sc is None else sc, models, stable_of(case))
