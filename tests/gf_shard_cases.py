"""Case table and CPU references of the surfel-sharded GraphFit tests (test_gf_shard_cases.py pins the fixtures on the CPU,
test_gpu_graphfit_sharded.py runs them on the device as emulated ranks).  No GPU is touched at import.

A sharded rank evaluates the surfels [N r // W, N (r + 1) // W) of the frame (slm_gf_set_shard); rank 0 also evaluates the
node terms.  Per iteration the ranks sum their partial state [(J+1) 7 gradient | SLM_GF_NTERMS terms] twice: behind the
morphing term's first pass (its mean needs the GLOBAL kept count) and behind the losses.  The cases below sit where that can
go wrong: every option family at world 2, 3 and 4; shards that keep no surfel of the morphing term while the frame keeps some
(the short-list scene, whose surfels are sorted by class, and the N = 257 frame with its five kept surfels in one shard); a shard
without one candidate; shard edges inside a 16-surfel staging group, a wave and a workgroup of k_gf_data, also where a stability
mask takes surfels out on the in-shard side of the edge; edges at exact multiples of 256; empty shards (N = 3 at world 4) and a
frame without surfels.  The scenes, options and tolerances are gf_shape_cases.py's; the per-shard reference is the same oracle
on ``gfo.Problem(sc, stable=shard_mask)``."""
import dataclasses
import functools

import numpy as np

import gf_shape_cases as cases
from gf_shape_cases import Case
from helpers import GF_CORR_VARIANTS, GF_SEMANTIC_VARIANTS
from oracle import graphfit_oracle as gfo

NTERMS = 10             # SLM_GF_NTERMS (include/super_lm.h)
T_FACE, T_ARAP, T_ROT, T_PP, T_PP_KEPT, T_MORPH, T_MORPH_KEPT, T_MORPH_FLAG, T_CORR, T_CORR_KEPT = range(NTERMS)
SURFEL_TERMS = (T_PP, T_PP_KEPT, T_MORPH, T_MORPH_KEPT, T_MORPH_FLAG, T_CORR, T_CORR_KEPT)
NODE_TERMS = (T_FACE, T_ARAP, T_ROT)
COUNTS = (T_PP_KEPT, T_MORPH_KEPT, T_MORPH_FLAG, T_CORR_KEPT)

# the option tags with the morphing term: the only term that takes a mean, so the only one a rank cannot evaluate alone
MORPH_TAGS = tuple(t for t, kw in GF_SEMANTIC_VARIANTS.items() if kw.get("sf_bn_morph"))
FAMILY_TAGS = ("sgd", "adam", "adamface", "soft", "softadam", "hard", "morph", "clip", "corr", "corrpp")
WORLDS = (2, 3, 4)


@dataclasses.dataclass(frozen=True)
class ShardCase:
    """A frame with its options (gf_shape_cases.Case), the number of ranks and the state dtype ("f32" or None: float64)."""
    case: Case
    world: int
    state: str = None

    @property
    def id(self):
        return f"{self.case.id}-W{self.world}" + ("" if self.state is None else "-" + self.state)

    @property
    def morph(self):
        return self.case.tag in MORPH_TAGS


def family_case(tag, **kw):
    """The 3000-surfel, 48-node frame of an option family (semantic scene / recorded flow where the family reads one)."""
    return Case(tag, 3000, 48, 4, 21, semantic=tag in GF_SEMANTIC_VARIANTS, flow=tag in GF_CORR_VARIANTS, **kw)


FAMILIES = [ShardCase(family_case(tag), W) for tag in FAMILY_TAGS for W in WORLDS]
# sorted by class: shard 0 keeps nothing at world 3 (nine candidates) and has no candidate at all at world 4
SHORT_LIST = [ShardCase(c, W) for c in cases.SHORT_LIST for W in (3, 4)]
# the frame test_gpu_dist_procgroup.py runs under a two-rank process group (GraphFit._iterate with its exchange buffer)
PROCGROUP = ShardCase(Case("softadam", 3000, 48, 4, 23, semantic=True, short_list=True), 2)
SHORT_LIST.append(PROCGROUP)
# five kept surfels, all in shard 0
FEW_KEPT = [ShardCase(Case("soft", 257, 12, 4, 84, semantic=True), W) for W in (2, 3)]
K6 = [ShardCase(Case("morph", 3000, 48, 6, 21, semantic=True), 3)]      # k_gf_morph skins with gf_skin_pos
MASKED = [ShardCase(family_case("softadam", mask="random"), 3), ShardCase(family_case("adamface", mask="groups"), 3),
          ShardCase(family_case("soft", mask="groups"), 4)]
F32 = [ShardCase(family_case("soft"), 3, "f32"), ShardCase(family_case("adamface"), 2, "f32")]
ALIGNED = [ShardCase(Case("soft", 1024, 48, 4, 21, semantic=True), 4)]  # bounds 256, 512, 768
DEGENERATE = [ShardCase(Case("adamface", 3, 12, 4, 90), 4), ShardCase(Case("soft", 3, 12, 4, 90, semantic=True), 4),
              ShardCase(Case("adamface", 0, 12, 4, 91), 2)]
SHARDED = FAMILIES + SHORT_LIST + FEW_KEPT + K6 + MASKED + F32 + ALIGNED + DEGENERATE
# the cases of the one-evaluation check against oracle_grad and oracle_partial: those without the morphing term (with it on
# a sharded handle slm_gf_loss_grad refuses to evaluate, and a rank's share of a mean is no sum; the ten steps and the
# reported terms cover those families)
GRAD_CASES = [sc for sc in SHARDED if not sc.morph]

# re-sharding: a handle used as (1, 2) becomes (2, 3).  The tiny frame's new shard [10, 15) lies in one wave, so every sum
# of its evaluation has one order and the bits are determined; the large one's local rows add with float64 atomics
RESHARD_TINY = Case("adamface", 15, 6, 4, 71)
RESHARD_LARGE = family_case("soft")

# kept surfels of the morphing term per shard at ``perturbed_dv`` (counted on the CPU oracle)
KEPT_TABLE = {("soft-N3000-J48-K4-sem-short", 3): (0, 169, 177), ("soft-N3000-J48-K4-sem-short", 4): (0, 88, 93, 165),
              ("soft-N257-J12-K4-sem", 2): (5, 0), ("soft-N257-J12-K4-sem", 3): (5, 0, 0)}


# ------------------------------------------------------------------------------------------------------------------ shards
def bounds(N, W):
    """[lo, hi) of every rank's shard: slm_gf_bind_frame's N r / W in integers."""
    return [(N * r // W, N * (r + 1) // W) for r in range(W)]


def shard_mask(case, r, W):
    """(N,) bool: the surfels rank r of W evaluates -- in its shard and stable."""
    lo, hi = bounds(case.N, W)[r]
    m = np.zeros(case.N, bool)
    m[lo:hi] = True
    st = cases.stable_of(case)
    return m if st is None else m & st


def identity(case):
    return np.tile(np.eye(1, 7), (case.J + 1, 1))


def morph_counts(case, dv, mask=None):
    """(candidates, kept) of the morphing term at ``dv`` over the stable surfels, or over ``mask`` (N,) bool."""
    import torch
    pb = gfo.Problem(cases.scene_of(case), stable=cases.stable_of(case) if mask is None else mask)
    _, sf = gfo.deform(pb, torch.from_numpy(np.array(dv)))
    gfo.bn_morph(pb, sf)
    return sum(s[2] for s in pb.morph_stats), sum(s[3] for s in pb.morph_stats)


def terms_vector(case, dv):
    """The SLM_GF_NTERMS entries the library reports for the whole frame at ``dv``, from the oracle: weighted losses, the
    kept counts, the morphing term as the weighted mean with its flag (0, 0, 0 where no class contributes)."""
    return _terms_vector(case, np.ascontiguousarray(dv).tobytes())


@functools.lru_cache(maxsize=64)
def _terms_vector(case, dv_bytes):
    dv = np.frombuffer(dv_bytes, np.float64).reshape(case.J + 1, 7)
    t, _, _, stats = cases.oracle_grad_at(case, dv)
    v = np.zeros(NTERMS)
    for k, name in ((T_FACE, "face_losses"), (T_ARAP, "arap_loss"), (T_ROT, "rot_loss"), (T_PP, "point_plane_loss"),
                    (T_PP_KEPT, "_matched"), (T_CORR, "corr_loss"), (T_CORR_KEPT, "_corr_matched")):
        v[k] = t.get(name, 0.0)
    if "sf_bn_morph_loss" in t:
        v[T_MORPH], v[T_MORPH_KEPT], v[T_MORPH_FLAG] = t["sf_bn_morph_loss"], sum(s[3] for s in stats), 1.0
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def oracle_partial(case, r, W):
    """(terms vector, gradient (J+1,7) with the global row NOT divided) of what rank r of W adds to the exchange at
    ``perturbed_dv``: the surfel terms over its shard, and on rank 0 the node terms.  Without the morphing term only (its
    mean is no sum of shares)."""
    import torch
    assert case.tag not in MORPH_TAGS
    opt = cases.opt_of(case.tag)
    if r != 0:
        opt.mesh_face = opt.mesh_arap = opt.mesh_rot = False
    pb = gfo.Problem(cases.scene_of(case), stable=shard_mask(case, r, W))
    dvt = torch.from_numpy(cases.perturbed_dv(case)).requires_grad_(True)
    loss, t = gfo.total_loss(pb, dvt, opt)
    g = torch.autograd.grad(loss, dvt)[0].numpy() if torch.is_tensor(loss) and loss.requires_grad else np.zeros((case.J + 1, 7))
    v = np.zeros(NTERMS)
    for k, name in ((T_FACE, "face_losses"), (T_ARAP, "arap_loss"), (T_ROT, "rot_loss"), (T_PP, "point_plane_loss"),
                    (T_PP_KEPT, "_matched"), (T_CORR, "corr_loss"), (T_CORR_KEPT, "_corr_matched")):
        x = t.get(name, 0.0)
        v[k] = float(x.detach()) if torch.is_tensor(x) else x
    return v, g


def touched_rows(case, r, W):
    """(J+1,) bool: the gradient rows the surfels of rank r can add to -- their nodes and the global row."""
    rows = np.zeros(case.J + 1, bool)
    m = shard_mask(case, r, W)
    rows[np.unique(cases.scene_of(case).sf_knn_idx[m])] = True
    rows[case.J] = bool(m.any())
    return rows
