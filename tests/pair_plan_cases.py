"""Frames that aim at the wave-level, segmented code of the pair-record Jacobian pass (python-super_amd/csrc/slm_pairs.h:
``pair_gram``; slm_prep.hip: ``prep_pairs``; slm_front.hip: ``k_pair_scatter``), which the raster-ordered, spatially coherent
``synth.make_scene`` frames reach only with long runs: a frame of ONE neighbour set, waves of 64 different sets, runs of every
length 1..9 with their boundaries at every remainder mod 4 and across a wave boundary, unmatched lanes at the first lane of a
wave and at the start, the end and the middle of a run, a wave without a matched lane and one with a single matched lane that
is not lane 0, sets that agree in their four smallest ids (the second sort key of the K > 4 order), shuffled rows, and sets
that couple the nodes 0 and J - 1 while one node belongs to no surfel.

Every case is a ``synth.Scene``: geometry, targets and semantic inputs of the 60 x 80 ``tiny`` base of prep_plan_cases.py at the
case's J (rows from the image interior, so that every surfel is matched unless the case moves it off the target), with
``sf_knn_idx`` / ``sf_knn_w`` replaced -- weights positive, normalised and distinct inside a row, columns never in ascending
id order (K >= 2), fixed seeds.  What a case's name claims is asserted from tests/pair_plan_model.py (and, for the match
pattern, from ``oracle.lm_oracle.data_term``) when the case is built.  Plain NumPy, importable without a GPU: consumed by
tests/test_pair_plan_cases.py (CPU) and tests/test_gpu_pair_plan.py (MI355X)."""
import dataclasses
import functools

import numpy as np

import lm_corr_model as lcm
import pair_plan_model as ppm
from oracle import lm_oracle as orc
from prep_plan_cases import TINY
from super_amd import synth

PER_SURFEL = ("sf_points", "sf_norms", "sf_knn_idx", "sf_knn_w", "sf_seg", "sf_seg_conf")
ALL_K = (1, 2, 3, 4, 5, 6, 7, 8)
COUNTS = (1, 2, 3, 4, 5, 7, 8, 9)          # run_lengths: surfels per set, cycled in sf_perm order
MARGIN = 12                                 # px between an "interior" surfel and the image border


def identity(J):
    return np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (J, 1))


def perturbed(J):
    return lcm.random_beta(J, 17, rot=0.01, trans=0.002)


def betas(J):
    return {"perturbed": perturbed(J), "identity": identity(J)}


def data_opt():
    """the data-side terms alone: ARAP and Rot off"""
    return orc.default_opt(mesh_arap=False, mesh_rot=False)


@functools.lru_cache(maxsize=None)
def base(J=48, K=4):
    """the `tiny` frame with J nodes and K surfel neighbours (K_ED = min(4, J - 1)), with semantic inputs (three classes)"""
    return synth.make_scene(**{**TINY, "J": J}, n_neighbors=min(K, J), n_ed_neighbors=min(4, J - 1), semantic=True, num_classes=3)


@functools.lru_cache(maxsize=None)
def interior(J=48, K=4):
    """rows of base(J, K) that project at least MARGIN px inside the image"""
    sc = base(J, K)
    t = orc.data_term(orc.Frame.from_scene(sc), identity(J), 1.0)
    ok = (t.u >= MARGIN) & (t.u < sc.W - MARGIN) & (t.v >= MARGIN) & (t.v < sc.H - MARGIN)
    rows = np.intersect1d(np.nonzero(ok)[0], t.match)
    assert len(rows) >= 1500
    return rows


def rows_of(sc, sel):
    """the scene with surfel rows ``sel`` (an index array)"""
    return dataclasses.replace(sc, **{k: np.ascontiguousarray(getattr(sc, k)[sel]) for k in PER_SURFEL if getattr(sc, k) is not None})


def _weights(rng, N, K):
    w = rng.uniform(0.05, 1.0, (N, K))
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    assert (w > 0).all() and all(len(set(r)) == K for r in w.tolist())
    return w


def frame(J, sets, seed):
    """a frame whose surfel i has the node SET sets[i] (N x K), columns permuted per row and never ascending"""
    rng = np.random.default_rng(seed)
    sets = np.sort(np.asarray(sets, np.int64), axis=1)
    N, K = sets.shape
    assert sets.min() >= 0 and sets.max() < J and (K == 1 or (np.diff(sets, axis=1) > 0).all()) and N <= 1500 and J <= 64
    idx = np.take_along_axis(sets, rng.permuted(np.tile(np.arange(K), (N, 1)), axis=1), axis=1)
    if K > 1:
        asc = (np.diff(idx, axis=1) > 0).all(1)
        idx[asc] = idx[asc, ::-1]
        assert not (np.diff(idx, axis=1) > 0).all(1).any()
    sc = rows_of(base(J), interior(J)[rng.permutation(len(interior(J)))[:N]])
    sc.sf_knn_idx = np.ascontiguousarray(idx)
    sc.sf_knn_w = _weights(rng, N, K)
    return sc


def random_sets(rng, n, K, lo, hi):
    """n distinct ascending K-sets of ids in [lo, hi), in lexicographic order"""
    out = set()
    while len(out) < n:
        out.add(tuple(sorted(rng.choice(np.arange(lo, hi), K, replace=False).tolist())))
    return sorted(out)


def spread(sets, counts, rng):
    """surfel rows: set t repeated counts[t] times, in random surfel order"""
    rows = np.repeat(np.asarray(sets, np.int64).reshape(len(sets), -1), counts, axis=0)
    return rows[rng.permutation(len(rows))]


@dataclasses.dataclass(eq=False)
class Case:
    name: str
    scene: synth.Scene
    state_f64: bool = True
    off: np.ndarray = None            # holes_in_runs: the surfels moved off the target (bool per surfel)

    @property
    def K(self):
        return self.scene.sf_knn_idx.shape[1]

    @functools.cached_property
    def plan(self):
        return ppm.build_plan(self.scene.sf_knn_idx, self.scene.J)

    @functools.cached_property
    def fr(self):
        return orc.Frame.from_scene(self.scene)       # (the scene's state is float32: the float32-state case has the SAME numbers)

    def match(self, beta):
        """bool per surfel: matched by the data term at beta"""
        on = np.zeros(self.scene.N, bool)
        on[orc.data_term(self.fr, beta, 1.0).match] = True
        return on

    @functools.lru_cache(maxsize=None)
    def system(self, which, lo=0, hi=None):
        """(A, jtl, M) of the plain data term at betas()[which], over the surfels at positions [lo, hi) of sf_perm"""
        beta = betas(self.scene.J)[which]
        if (lo, hi) == (0, None):
            return orc.normal_equations(self.fr, beta, data_opt())
        sub = rows_of(self.scene, self.plan.sf_perm[lo:hi].astype(np.int64))
        if sub.N == 0:
            P = 7 * self.scene.J
            return np.zeros((P, P)), np.zeros(P), 0
        return orc.normal_equations(orc.Frame.from_scene(sub), beta, data_opt())


def _all_matched(case):
    for b in betas(case.scene.J).values():
        assert case.match(b).all(), case.name


# ------------------------------------------------------------------------------------------------------------- the cases
def one_set(N, K, J=48):
    rng = np.random.default_rng(2000 + 10 * N + K + 100 * J)
    s = np.arange(K) if J == K else np.sort(rng.choice(J, K, replace=False))
    case = Case(f"one_set_n{N}_k{K}" + ("_jk" if J == K else ""), frame(J, np.tile(s, (N, 1)), 2001 + 10 * N + K + 100 * J))
    runs = ppm.runs_in_perm(case.plan)
    assert len(np.unique(ppm.set_ids(case.plan))) == 1 and len(runs) == -(-N // 64) and (runs[:, 3] == np.minimum(64, N - 64 * runs[:, 0])).all()
    assert case.plan.pairs == K * (K + 1) // 2 and (J != K or case.plan.pairs == J * (J + 1) // 2)
    _all_matched(case)
    return case


def all_distinct(K):
    """every surfel of a wave has another set: 64 runs of one row (K = 1: the 64 sets of 64 nodes, one wave)"""
    rng = np.random.default_rng(2100 + K)
    J, N = (64, 64) if K == 1 else (48, 130)
    sets = np.asarray(random_sets(rng, N, K, 0, J))
    case = Case(f"all_distinct_k{K}", frame(J, sets[rng.permutation(N)], 2101 + K))
    runs = ppm.runs_in_perm(case.plan)
    assert len(np.unique(ppm.set_ids(case.plan))) == N and (runs[:, 3] == 1).all() and (np.bincount(runs[:, 0]) == 64).any()
    _all_matched(case)
    return case


def run_lengths(K, state_f64=True):
    """sets repeated 1, 2, 3, 4, 5, 7, 8, 9 times (cycled) in sf_perm order"""
    rng = np.random.default_rng(2200 + K)
    sets = random_sets(rng, 40, K, 0, 48)
    counts = [COUNTS[t % len(COUNTS)] for t in range(len(sets))]
    case = Case(f"run_lengths_k{K}" + ("" if state_f64 else "_f32"), frame(48, spread(sets, counts, rng), 2201 + K), state_f64=state_f64)
    sid = ppm.set_ids(case.plan)[case.plan.sf_perm]
    cut = np.concatenate([[0], np.nonzero(np.diff(sid))[0] + 1, [case.plan.N]])       # the sets' position spans
    assert np.diff(cut).tolist() == counts                                          # ... have the lengths, in sf_perm order
    assert set(cut[:-1] % 4) == set(cut[1:] % 4) == {0, 1, 2, 3}                     # boundaries at every remainder mod 4
    assert ((cut[:-1] // 64) != ((cut[1:] - 1) // 64)).any()                         # a set's span crosses a wave boundary
    assert set(ppm.runs_in_perm(case.plan)[:, 3]) >= set(COUNTS)
    _all_matched(case)
    return case


def holes_in_runs(K):
    """five waves of runs of 5, 7 and 6 surfels; unmatched: the first lane of wave 0, the first / the last / a middle position
    of every other run of the waves 0, 3 and 4, all of wave 1, and all of wave 2 but its lane 37"""
    rng = np.random.default_rng(2300 + K)
    sets = random_sets(rng, 47, K, 0, 48)              # (47: no share boundary of world 2 or 3 on a set's boundary)
    counts = [(5, 7, 6)[t % 3] for t in range(len(sets))]
    sc = frame(48, spread(sets, counts, rng), 2301 + K)
    plan = ppm.build_plan(sc.sf_knn_idx, 48)
    assert plan.N >= 5 * 64 - 60
    sid = ppm.set_ids(plan)[plan.sf_perm]
    cut = np.concatenate([[0], np.nonzero(np.diff(sid))[0] + 1, [plan.N]])
    off_pos = np.zeros(plan.N, bool)
    off_pos[0] = True
    for r, (a, b) in enumerate(zip(cut[:-1], cut[1:])):
        where = {0: a, 1: b - 1, 2: (a + b) // 2}.get(r % 4)
        if where is not None:
            off_pos[where] = True
    off_pos[64:128] = True
    off_pos[128:192] = True
    off_pos[128 + 37] = False
    off = np.zeros(plan.N, bool)
    off[plan.sf_perm[off_pos]] = True
    sc.sf_points = sc.sf_points.copy()
    sc.sf_points[off, 0] += np.float32(10.0)                 # projects far outside the image
    case = Case(f"holes_in_runs_k{K}", sc, off=off)
    for beta in betas(48).values():                          # the pattern, from the oracle's match set
        on = case.match(beta)
        assert (on == ~off).all()
        onp = on[plan.sf_perm]
        assert not onp[0] and not onp[64:128].any() and np.nonzero(onp[128:192])[0].tolist() == [37]
        first, last = onp[cut[:-1]], onp[cut[1:] - 1]
        mid = np.array([not onp[a + 1:b - 1].all() for a, b in zip(cut[:-1], cut[1:])])
        whole = np.array([onp[a:b].any() for a, b in zip(cut[:-1], cut[1:])])
        assert (~first & whole).any() and (~last & whole).any() and (mid & first & last).any()
        runs = ppm.runs_in_perm(plan, on)
        assert set(runs[:, 0]) == {0, 2, 3, 4} and (runs[runs[:, 0] == 2, 1:] == [128 + 37, 128 + 38, 1]).all()
    return case


def shared_prefix(K):
    """groups of sets that share their four smallest ids and differ in the others, interleaved in surfel order"""
    assert K > 4
    rng = np.random.default_rng(2400 + K)
    sets, counts = [], []
    for p in random_sets(rng, 6, 4, 0, 20):
        for t in random_sets(rng, 5, K - 4, 20, 48):
            sets.append(p + t)
            counts.append(int(rng.integers(1, 4)))
    case = Case(f"shared_prefix_k{K}", frame(48, spread(sets, counts, rng), 2401 + K))
    c, perm = case.plan.c, case.plan.sf_perm
    by_prefix = np.lexsort((np.arange(case.plan.N),) + tuple(c[:, k] for k in (3, 2, 1, 0)))     # the first four ids alone
    assert not np.array_equal(by_prefix, perm)                # the ids 4..K-1 decide the order
    same_prefix = (c[perm[1:], :4] == c[perm[:-1], :4]).all(1)
    differ = (c[perm[1:]] != c[perm[:-1]]).any(1)
    assert (same_prefix & differ).sum() >= 6 * 4              # neighbours in sf_perm that differ ONLY behind the prefix
    srf = ppm.set_ids(case.plan)
    assert (np.diff(srf) != 0).mean() > 0.9                   # interleaved: neighbours in surfel order rarely share a set
    _all_matched(case)
    return case


def shuffled(K):
    """a make_scene frame at K neighbours (its own KNN ids and weights), surfel rows permuted"""
    sc = base(48, K)
    rng = np.random.default_rng(2500 + K)
    case = Case(f"shuffled_k{K}", rows_of(sc, interior(48, K)[rng.permutation(len(interior(48, K)))[:1500]]))
    runs = ppm.runs_in_perm(case.plan)
    assert (np.diff(ppm.set_ids(case.plan)) != 0).mean() > 0.9 and runs[:, 3].max() > 4
    return case


def far_pairs(K):
    """sets that couple node 0 with node J - 1; node 31 belongs to no surfel"""
    J = 64
    rng = np.random.default_rng(2600 + K)
    ids = np.setdiff1d(np.arange(1, J - 1), [31])
    sets = [(0,) + tuple(sorted(rng.choice(ids, K - 2, replace=False).tolist())) + (J - 1,) for _ in range(12)]
    sets += [tuple(sorted(rng.choice(np.setdiff1d(np.arange(J), [31]), K, replace=False).tolist())) for _ in range(20)]
    sets = sorted(set(sets))
    case = Case(f"far_pairs_k{K}", frame(J, spread(sets, [int(rng.integers(1, 8)) for _ in sets], rng), 2601 + K))
    key = case.plan.blk_key
    assert (J - 1) * J + 0 in key and 31 * J + 31 not in key and 31 not in case.plan.c
    assert (case.plan.key_a - case.plan.key_b).max() == J - 1
    diag = case.plan.key_a[case.plan.key_a == case.plan.key_b]
    assert len(diag) < J and set(diag) == set(np.unique(case.plan.c))
    _all_matched(case)
    return case


ONE_SET_N = (1, 63, 64, 65, 129)
BUILDERS = {}
for _K in ALL_K:
    for _N in ONE_SET_N:
        BUILDERS[f"one_set_n{_N}_k{_K}"] = functools.partial(one_set, _N, _K)
    if _K >= 2:
        BUILDERS[f"one_set_n65_k{_K}_jk"] = functools.partial(one_set, 65, _K, _K)          # J == K
    BUILDERS[f"all_distinct_k{_K}"] = functools.partial(all_distinct, _K)
    BUILDERS[f"run_lengths_k{_K}"] = functools.partial(run_lengths, _K)
    BUILDERS[f"holes_in_runs_k{_K}"] = functools.partial(holes_in_runs, _K)
for _K in (5, 6, 8):
    BUILDERS[f"shared_prefix_k{_K}"] = functools.partial(shared_prefix, _K)
for _K in (4, 6):
    BUILDERS[f"shuffled_k{_K}"] = functools.partial(shuffled, _K)
for _K in (3, 5):
    BUILDERS[f"far_pairs_k{_K}"] = functools.partial(far_pairs, _K)
BUILDERS["run_lengths_k6_f32"] = functools.partial(run_lengths, 6, False)                  # the float32-state case
NAMES = tuple(BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name):
    """the case of a name (shared, do not modify)"""
    c = BUILDERS[name]()
    assert c.name == name, (c.name, name)
    return c


def names_of(K):
    return tuple(n for n in NAMES if case_k(n) == K)


def case_k(name):
    return int(name.split("_k")[1].split("_")[0])


# the frames of the shares test (world 2 and 3) and of the tests of the other users of pair_gram
SHARED = tuple(f"{fam}_k{K}" for fam in ("run_lengths", "holes_in_runs") for K in (3, 4, 6))
OTHER_USERS = tuple(f"{fam}_k{K}" for fam in ("all_distinct", "holes_in_runs") for K in (4, 6))
BATCHES = {6: ("run_lengths_k6", "one_set_n65_k6", "holes_in_runs_k6"), 4: ("holes_in_runs_k4", "all_distinct_k4", "one_set_n1_k4")}


def bounds(N, W):
    """[lo, hi) of every rank's share of the sf_perm positions (bind_shard_share: N r / W in integers)"""
    return [(N * r // W, N * (r + 1) // W) for r in range(W)]


def boundary_inside_a_run(c, W):
    """a share boundary of world W falls strictly inside a span of equal sets of sf_perm"""
    sid = ppm.set_ids(c.plan)[c.plan.sf_perm]
    return any(0 < lo < c.plan.N and sid[lo - 1] == sid[lo] for lo, _ in bounds(c.plan.N, W)[1:])


# --------------------------------------------------------------------------------------- inputs of the other users of pair_gram
def edge_pattern(c):
    """bool per surfel, laid over the runs of sf_perm: False at the start of every run r = 0 mod 3 and at the end of every
    run r = 1 mod 3 (of the matched surfels' runs, cut at the waves), True elsewhere"""
    on = c.match(perturbed(c.scene.J)) & c.match(identity(c.scene.J))
    runs = ppm.runs_in_perm(c.plan, on)
    onp = on[c.plan.sf_perm]
    pat = np.ones(c.plan.N, bool)
    for r, (_, a, b, _) in enumerate(runs):
        pos = np.nonzero(onp[a:b])[0] + a
        if r % 3 == 0:
            pat[pos[0]] = False
        elif r % 3 == 1:
            pat[pos[-1]] = False
    out = np.zeros(c.plan.N, bool)
    out[c.plan.sf_perm] = pat
    assert (~out).sum() >= 10 and out.sum() >= 10
    return out


def corr_targets(c):
    """point-point correspondences: o = the surfel moved a few mm, valid by ``edge_pattern`` (normals: the surfel's own)"""
    rng = np.random.default_rng(2700 + c.K)
    o = c.scene.f64("sf_points") + rng.normal(0, 0.003, (c.scene.N, 3))
    return o, c.scene.f64("sf_norms"), edge_pattern(c)


def hard_sem(c):
    """semantic inputs under which the HARD weight of a matched surfel is 1 or 0 by ``edge_pattern`` -- weight 0 at run
    starts and ends: two classes, the target table says class 0 everywhere (confidence gap 1), sf_seg = 0 where the pattern
    holds and 1 elsewhere"""
    from types import SimpleNamespace
    pat = edge_pattern(c)
    T = c.scene.T
    return SimpleNamespace(sf_seg=np.where(pat, 0, 1).astype(np.int64), sf_seg_conf=np.tile(np.float32([0.5, 0.5]), (c.scene.N, 1)),
                           tgt_seg_conf=np.tile(np.float32([1.0, 0.0]), (T, 1))), pat


def face_mesh(c):
    """a mesh of 24 triangles over nodes far apart in id (pairs no surfel has) with areas off by a few percent"""
    rng = np.random.default_rng(2800 + c.K)
    J = c.scene.J
    tri = np.stack([rng.choice(J, 3, replace=False) for _ in range(24)], 1).astype(np.int64)
    g = c.scene.f64("ed_points")
    area = 0.5 * np.linalg.norm(np.cross(g[tri[1]] - g[tri[0]], g[tri[2]] - g[tri[0]]), axis=1)
    mesh = (tri, area * rng.uniform(0.9, 1.1, 24))
    plan = ppm.build_plan(c.scene.sf_knn_idx, J, tri)
    assert plan.pairs > c.plan.pairs                          # the mesh brings pairs of its own
    return mesh, plan
