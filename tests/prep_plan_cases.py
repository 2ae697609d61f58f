"""Frames that aim at the branches of the K = 4 preparation (python-super_amd/csrc/slm_prep.hip) which the raster-ordered,
spatially coherent ``synth.make_scene`` frames never reach: partly active waves, padding at every remainder, bins at and next
to BIN_CAP in both sorting phases, more bins than threads of the one-block scans, workgroups at and beyond SLM_LB_MAX records,
the hinted bound at its edge, a plan that shrinks, and rows the bind must refuse.

Every case is a ``synth.Scene``: geometry and targets of the 60 x 80 ``tiny`` base (at the case's J), tiled or truncated to N
surfels, with ``sf_knn_idx`` / ``sf_knn_w`` replaced -- weights positive, normalised and distinct inside a row, columns NOT in
ascending id order (so that "original column order" differs from the canonical tuple), fixed seeds.  What a case's name
claims is asserted from ``prep_plan_model.plan_stats`` when the case is built.  Plain NumPy, importable without a GPU: consumed
by tests/test_prep_plan_cases.py (CPU) and tests/test_gpu_prep_plan.py (MI355X)."""
import dataclasses
import functools

import numpy as np

from prep_plan_model import BIN_CAP, LB_MAX, plan_stats
from super_amd import synth

TINY = dict(N=3000, J=48, H=60, W=80, seed=7, src_border=5, tgt_border=3)       # `tiny` of test_gpu_prepare_binned.py
SMALL = dict(N=12000, J=108, H=120, W=160, seed=3, src_border=6, tgt_border=4)  # `small` of the same file
PER_SURFEL = ("sf_points", "sf_norms", "sf_knn_idx", "sf_knn_w")


@functools.lru_cache(maxsize=None)
def base(J=48):
    """the `tiny` frame with J nodes (K_ED = min(4, J - 1))"""
    return synth.make_scene(**{**TINY, "J": J}, n_ed_neighbors=min(4, J - 1))


def tiny():
    return dataclasses.replace(base(48))


def _rows(sc, sel):
    """the scene with surfel rows ``sel`` (an index array: truncation, tiling or a permutation)"""
    return dataclasses.replace(sc, **{k: np.ascontiguousarray(getattr(sc, k)[sel]) for k in PER_SURFEL})


def _weights(rng, N, K=4):
    """positive, normalised float32 weights, distinct inside every row"""
    w = rng.uniform(0.05, 1.0, (N, K))
    w = (w / w.sum(1, keepdims=True)).astype(np.float32)
    assert (w > 0).all() and all(len(set(r)) == K for r in w[:64])
    return w


def _frame(J, tuples, seed):
    """a frame whose surfel i has the node SET tuples[i] (N x 4), columns permuted per row and never ascending"""
    rng = np.random.default_rng(seed)
    tuples = np.asarray(tuples, np.int64)
    N = len(tuples)
    assert tuples.shape == (N, 4) and (np.diff(np.sort(tuples, 1), axis=1) > 0).all() and tuples.min() >= 0 and tuples.max() < J
    idx = np.take_along_axis(np.sort(tuples, 1), rng.permuted(np.tile(np.arange(4), (N, 1)), axis=1), axis=1)
    asc = (np.diff(idx, axis=1) > 0).all(1)
    idx[asc] = idx[asc, ::-1]
    sc = _rows(base(J), np.arange(N) % base(J).N)
    sc.sf_knn_idx = np.ascontiguousarray(idx)
    sc.sf_knn_w = _weights(rng, N)
    return sc


def _random_tuples(rng, n, lo, hi, k=4):
    """n ascending k-tuples of ids in [lo, hi), distinct from each other, in random order"""
    out = set()
    while len(out) < n:
        out.add(tuple(sorted(rng.choice(np.arange(lo, hi), k, replace=False).tolist())))
    out = sorted(out)
    return [out[i] for i in rng.permutation(n)]


def _spread(tuples, counts, rng):
    """surfel rows: tuple t repeated counts[t] times, in random surfel order"""
    rows = np.repeat(np.asarray(tuples, np.int64), counts, axis=0)
    return rows[rng.permutation(len(rows))]


# ------------------------------------------------------------------------------------------------------------- the cases
def n_surfels(N, J):
    """N surfels of one tuple: a single, partly active wave in kb_keys / kb_scatter"""
    sc = _frame(J, np.tile([0, 1, 2, 3] if J == 4 else [5, 17, 30, 47], (N, 1)), 1000 + 10 * N + J)
    st = plan_stats(sc.sf_knn_idx, J)
    assert st.tuples == 1 and st.positions == ((N + 3) // 4 * 4 + 63) // 64 * 64 and (N > 61 or st.positions == 64)
    return sc


PAD_SIZES = (300, 1, 2, 3, 4, 5, 63, 64, 65)       # in tuple order


def pad_edges():
    rng = np.random.default_rng(1101)
    tuples = [(t, t + 9, t + 20, t + 38) for t in range(len(PAD_SIZES))]      # ascending in t: the order of PAD_SIZES
    sc = _frame(48, _spread(tuples, PAD_SIZES, rng), 1102)
    st = plan_stats(sc.sf_knn_idx, 48)
    assert st.tuple_surfels.tolist() == list(PAD_SIZES) and sorted(PAD_SIZES) == [1, 2, 3, 4, 5, 63, 64, 65, 300]
    five = PAD_SIZES.index(5)
    assert st.tuple_start[five] % 64 == 60 and st.tuple_runs[five] == 2            # 8 positions, two runs
    end = st.tuple_start + (st.tuple_surfels + 3) // 4 * 4 - 1
    assert ((st.tuple_start >> 8) != (end >> 8)).any()                              # a tuple spans two workgroups
    return sc


def shuffled_surfels():
    """`tiny` with its surfel rows permuted (its own KNN ids and weights): neighbouring lanes never share a bin for long"""
    sc = _rows(base(48), np.random.default_rng(1201).permutation(base(48).N))
    a = np.sort(sc.sf_knn_idx, 1)[:, 0]
    runs = np.diff(np.flatnonzero(np.concatenate([[True], a[1:] != a[:-1], [True]])))
    assert np.median(runs) == 1 and ((a[:-2] == a[2:]) & (a[:-2] != a[1:-1])).any()     # lane runs of 1; a, b, a alternation
    return sc


def bin_a(count):
    """node 0 is the smallest id of exactly `count` surfels (three tuples); no other phase-A bin above 200"""
    rng = np.random.default_rng(1300 + count)
    hot = [(0, 1, 2, 3), (0, 5, 9, 11), (0, 7, 20, 33)]
    rest = _random_tuples(rng, 30, 1, 48)
    rows = _spread(hot + rest, [400, 400, count - 800] + [50] * 30, rng)
    sc = _frame(48, rows, 1301 + count)
    st = plan_stats(sc.sf_knn_idx, 48)
    assert st.bin_a[0] == count and (st.tuple_ids[:, 0] == 0).sum() >= 3 and st.bin_a[1:].max() <= 200
    assert st.max_bin_b < BIN_CAP          # phase B stays out of the way: what happens is decided by node 0's bin alone
    assert st.wg_records.max() <= LB_MAX   # ... and the record arrays can be read back
    return sc


def bin_b(entries):
    """node J - 1 is the largest id of exactly entries / 4 single-surfel tuples (4 entries per run); phase-A bins small.
    (The other three ids of 64 tuples in a row come from nine ids, so that no workgroup has more than LB_MAX records and the
    record arrays can be read back.)"""
    rng = np.random.default_rng(1400 + entries)
    assert entries % 4 == 0
    top = []
    for g in range(-(-entries // 256)):
        top += [t + (47,) for t in _random_tuples(rng, min(64, entries // 4 - 64 * g), 9 * g, 9 * g + 9, k=3)]
    rest = _random_tuples(rng, 6, 37, 47)
    sc = _frame(48, _spread(top + rest, [1] * len(top) + [30] * 6, rng), 1401 + entries)
    st = plan_stats(sc.sf_knn_idx, 48)
    assert st.bin_b[47] == entries == st.max_bin_b and st.max_bin_a < 200 and st.wg_records.max() <= LB_MAX
    assert (st.tuple_surfels[st.tuple_ids[:, 3] == 47] == 1).all() and (st.tuple_ids[:, 3] == 47).sum() == entries // 4
    return sc


def many_nodes(J):
    """J above the 1024 threads of the one-block scans; 3 000 surfels on 75 tuples of nearby ids: most bins empty"""
    rng = np.random.default_rng(1500 + J)
    starts = np.concatenate([rng.choice(J - 8, 74, replace=False), [J - 8]])
    tuples = [tuple(int(s) + np.sort(rng.choice(8, 4, replace=False))) for s in starts[:-1]] + [(J - 4, J - 3, J - 2, J - 1)]
    sc = _frame(J, _spread(tuples, [40] * 75, rng), 1501 + J)
    st = plan_stats(sc.sf_knn_idx, J)
    assert -(-J // 1024) == {1025: 2, 2050: 3}[J] and st.ids_used.max() == J - 1      # bins per thread of a 1024-thread scan
    assert (st.bin_a == 0).sum() > J // 2 and (st.bin_b == 0).sum() > J // 2 and sc.N == 3000 and st.wg_records.max() <= LB_MAX
    return sc


def wg_records(count):
    """exactly `count` (96 or 97) distinct pairs in workgroup 0 (256 positions); the other workgroups have fewer"""
    rng = np.random.default_rng(1600 + count)
    nine = [(4 * t, 4 * t + 1, 4 * t + 2, 4 * t + 3) for t in range(9)]                  # node-disjoint: 90 pairs
    extra = [(0, 1, 2, 4), (8, 9, 10, 12)]                                               # three ids of one, one of another: + 3 each
    if count == 97:
        extra.append((0, 1, 3, 4))                                                       # only (4, 3) is new: + 1
    first = nine + extra
    sizes = [20] * len(first)
    sizes[-1] += 256 - sum(sizes)                                                        # workgroup 0 exactly full
    assert sum((s + 3) // 4 * 4 for s in sizes) == 256
    later = [(36, 37, 38, 39), (40, 41, 42, 43), (44, 45, 46, 47), (36, 40, 44, 47)]
    sc = _frame(48, _spread(first + later, sizes + [70, 70, 70, 30], rng), 1601 + count)
    st = plan_stats(sc.sf_knn_idx, 48)
    assert st.wg_records[0] == count and st.wg_records[1:].max() <= LB_MAX and len(st.wg_records) >= 2
    assert (count <= LB_MAX) == (st.wg_records.max() <= LB_MAX)
    return sc


def wg_dense():
    """64 single-surfel tuples of uniformly random ids: one workgroup with several hundred records (run_lidx clamps at 255)"""
    rng = np.random.default_rng(1701)
    sc = _frame(48, _random_tuples(rng, 64, 0, 48), 1702)
    st = plan_stats(sc.sf_knn_idx, 48)
    assert len(st.wg_records) == 1 and st.wg_records[0] > 300 and (st.tuple_surfels == 1).all() and st.tuples == 64
    return sc


def hint_pair(miss):
    """(A, B): B has t0 + t0 // 8 + 64 tuples (the hinted bound after A holds exactly) or one more (it misses by one)"""
    rng = np.random.default_rng(1800 + int(miss))
    a = _frame(48, _spread(_random_tuples(rng, 100, 0, 48), [5] * 100, rng), 1801 + int(miss))
    t0 = plan_stats(a.sf_knn_idx, 48).tuples
    want = t0 + t0 // 8 + 64 + int(miss)
    b = _frame(48, _spread(_random_tuples(rng, want, 0, 48), [1] * (want - 40) + [6] * 40, rng), 1803 + int(miss))
    assert t0 == 100 and plan_stats(b.sf_knn_idx, 48).tuples == want and b.N > want        # min(bound, N) does not bind
    return a, b


def shrink():
    return tiny(), n_surfels(65, 48)


def bad_row(kind):
    """`tiny` with ONE bad row, the last: a repeated id, an id = J, an id = -1"""
    sc = tiny()
    idx = sc.sf_knn_idx.copy()
    if kind == "dup_row":
        idx[-1, 2] = idx[-1, 0]
    elif kind == "oob_row":
        idx[-1, 1] = sc.J
    else:
        assert kind == "neg_row"
        idx[-1, 3] = -1
    sc.sf_knn_idx = idx
    good = sc.sf_knn_idx[:-1]
    assert (good >= 0).all() and (good < sc.J).all() and (np.diff(np.sort(good, 1), axis=1) > 0).all()
    return sc


SINGLE = {f"n{n}_j{J}": functools.partial(n_surfels, n, J) for J in (4, 48) for n in (1, 3, 63, 64, 65)}
SINGLE.update({
    "pad_edges": pad_edges, "shuffled_surfels": shuffled_surfels,
    "binA_1023": functools.partial(bin_a, 1023), "binA_1024": functools.partial(bin_a, 1024), "binA_1025": functools.partial(bin_a, 1025),
    "binB_1024": functools.partial(bin_b, 1024), "binB_1028": functools.partial(bin_b, 1028),
    "j1025": functools.partial(many_nodes, 1025), "j2050": functools.partial(many_nodes, 2050),
    "wg_96": functools.partial(wg_records, 96), "wg_97": functools.partial(wg_records, 97), "wg_dense": wg_dense,
})
PAIRS = {"hint_hold": functools.partial(hint_pair, False), "hint_miss": functools.partial(hint_pair, True), "shrink": shrink}
REFUSED = ("dup_row", "oob_row", "neg_row")
OVER_CAP = ("binA_1025", "binB_1028")          # a bin above BIN_CAP: the slot goes to the rocPRIM pipeline
NOT_MERGED = ("wg_97", "wg_dense")             # a workgroup above LB_MAX records: the per-run form of the data term
WIDENED = ("shuffled_surfels", "binA_1025", "wg_dense")
WIDEN_K = (1, 6, 8)


@functools.lru_cache(maxsize=None)
def single(name):
    return SINGLE[name]()


@functools.lru_cache(maxsize=None)
def pair(name):
    return PAIRS[name]()


def widened(name, K):
    """the case at K neighbours (the pair-record form): the first min(K, 4) columns kept, the others drawn without repetition;
    fresh weights, distinct inside a row"""
    sc = dataclasses.replace(single(name))
    rng = np.random.default_rng(1900 + 10 * WIDENED.index(name) + K)
    idx = sc.sf_knn_idx[:, :min(K, 4)].copy()
    if K > 4:
        noise = rng.random((sc.N, sc.J))
        noise[np.arange(sc.N)[:, None], idx] = 2.0                   # never an id the row has already
        idx = np.concatenate([idx, np.argsort(noise, axis=1)[:, :K - 4]], axis=1)
    assert all(len(set(r)) == K for r in idx.tolist())
    sc.sf_knn_idx = np.ascontiguousarray(idx, dtype=np.int64)
    sc.sf_knn_w = _weights(rng, sc.N, K)
    return sc
