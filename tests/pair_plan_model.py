"""TEST INFRASTRUCTURE: a NumPy construction of the pair plan (``PairPlan``, python-super_amd/csrc/slm_prep.h) and of the pair
records the Jacobian pass of the pair-record form must leave behind (python-super_amd/csrc/slm_pairs.h), written from those
two specifications -- whole-array NumPy (``unique``, ``searchsorted``, ``lexsort``) on the plan side and a DENSE normal matrix
cut into blocks on the record side: no wave, no run, no ballot is simulated here.

The plan of a frame with N surfels of K neighbours among J nodes (and, with the face term, a mesh ``tri`` (3, F)):
  blk_key   the ascending distinct keys max(a, b) * J + min(a, b) over all node pairs of all surfels, diagonal pairs included,
            and over the six pairs of every triangle; unsigned 32-bit
  sf_pidx   (N, K(K+1)/2): slot ra(ra+1)/2 + rb (rb <= ra) holds the position in blk_key of the pair (c[ra], c[rb]), c the
            surfel's ids in ascending order
  sf_perm   the surfels in lexicographic order of the full tuple c, ties by surfel id.  (The tie rule holds because the
            library sorts with rocprim::radix_sort_pairs over the surfel ids 0..N-1 in order -- once for K <= 4, least
            significant key first for K > 4 -- and a radix sort is stable; slm_prep.hip, prep_pairs.)
  tri_pidx  (F, 6): the positions of a triangle's pairs -- the diagonals of vertex 0, 1, 2, then (0,1), (0,2), (1,2)
            (FaceDev::tri_pidx, slm_face.h)

The records of a system (A = J^T J, jtl = -J^T r) whose every non-zero block is a pair of blk_key -- the data-side terms with
ARAP and Rot switched off: record k of key a * J + b, 56 doubles,
  a > b    entries 0..48 = A[7a:7a+7, 7b:7b+7] row-major (the larger id's rows first: never transposed); 49..55 unused
  a == b   entries 0..48 = the block of node a, of which only the LOWER triangle (row >= column) is defined; 49..55 = the
           node's seven entries of +J^T r.  SIGN: k_pair_scatter (slm_front.hip) stores rhs = -record, "jtl = -J^T r": the
           record carries J^T r itself, i.e. MINUS the references' jtl.
Behind the records ride SLM_VK_TAIL = 64 doubles whose SUM is the matched count of the data term.
"""
from types import SimpleNamespace

import numpy as np

WREC = 56            # SLM_WREC: doubles per record
VK_TAIL = 64         # SLM_VK_TAIL
WHAT = dict(blk_key=13, sf_pidx=14, sf_perm=15, tri_pidx=16)        # slm_debug_read_plan (include/super_lm.h)


def slots(K):
    """(ra, rb) of the canonical slots in slot order ra(ra+1)/2 + rb"""
    ra, rb = np.tril_indices(K)
    assert (ra * (ra + 1) // 2 + rb == np.arange(K * (K + 1) // 2)).all()
    return ra, rb


def canon(knn_idx):
    """(N, K) ids of every surfel ascending"""
    return np.sort(np.asarray(knn_idx, dtype=np.int64), axis=1)


def tri_pairs(tri):
    """(F, 6, 2) node pairs (larger, smaller) of every triangle in tri_pidx order"""
    t = np.asarray(tri, dtype=np.int64)
    va, vb = np.array([0, 1, 2, 0, 0, 1]), np.array([0, 1, 2, 1, 2, 2])
    a, b = t[va].T, t[vb].T
    return np.stack([np.maximum(a, b), np.minimum(a, b)], -1)


def build_plan(knn_idx, J, tri=None):
    c = canon(knn_idx)
    N, K = c.shape
    assert 1 <= K <= 8 and J * J < 2 ** 32 and c.min() >= 0 and c.max() < J and (K == 1 or (np.diff(c, axis=1) > 0).all())
    ra, rb = slots(K)
    keys = (c[:, ra] * J + c[:, rb]).astype(np.uint32)                       # (N, NP); c[ra] >= c[rb]
    allk = keys.reshape(-1)
    tkeys = None
    if tri is not None and np.asarray(tri).shape[1] > 0:
        tp = tri_pairs(tri)
        tkeys = (tp[..., 0] * J + tp[..., 1]).astype(np.uint32)
        allk = np.concatenate([allk, tkeys.reshape(-1)])
    blk_key = np.unique(allk)
    sf_pidx = np.searchsorted(blk_key, keys).astype(np.int32)
    assert (blk_key[sf_pidx] == keys).all()
    order = np.lexsort((np.arange(N),) + tuple(c[:, k] for k in range(K - 1, -1, -1)))      # last key = most significant
    plan = SimpleNamespace(N=N, K=K, J=J, c=c, blk_key=blk_key, sf_pidx=sf_pidx, sf_perm=order.astype(np.int32), pairs=len(blk_key),
                           tri_pidx=None if tkeys is None else np.searchsorted(blk_key, tkeys).astype(np.int32))
    plan.key_a, plan.key_b = (blk_key // np.uint32(J)).astype(np.int64), (blk_key % np.uint32(J)).astype(np.int64)
    return plan


# ------------------------------------------------------------------------------------------------ what the cases assert from
def set_ids(plan):
    """(N,) an id per distinct neighbour set (equal sets <-> equal ids), in surfel order"""
    _, inv = np.unique(plan.c, axis=0, return_inverse=True)
    return inv.reshape(-1)


def runs_in_perm(plan, on=None):
    """the maximal runs of equal sets among the positions of sf_perm that are ``on`` (a bool per SURFEL; default all), cut at
    the 64-position waves as the Jacobian pass cuts them: arrays (wave, first position, last position + 1, "on" surfels)"""
    sid = set_ids(plan)[plan.sf_perm]
    onp = np.ones(plan.N, bool) if on is None else np.asarray(on, bool)[plan.sf_perm]
    out = []
    for w0 in range(0, plan.N, 64):
        pos = np.nonzero(onp[w0:w0 + 64])[0] + w0
        if len(pos) == 0:
            continue
        cut = np.nonzero(np.diff(sid[pos]) != 0)[0] + 1
        for seg in np.split(pos, cut):
            out.append((w0 // 64, seg[0], seg[-1] + 1, len(seg)))
    return np.array(out, dtype=np.int64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------- the records
LOWER = np.tril(np.ones((7, 7), bool)).reshape(-1)


def record_mask(plan):
    """(pairs, 56) bool: the entries of the records that are DEFINED -- every block entry of an off-diagonal pair, the lower
    triangle and the seven J^T r entries of a diagonal one"""
    m = np.zeros((plan.pairs, WREC), bool)
    diag = plan.key_a == plan.key_b
    m[:, :49] = True
    m[diag, :49] = LOWER
    m[diag, 49:] = True
    return m


def records_of(plan, A, jtl):
    """(pairs, 56) the records of the dense system (A, jtl = -J^T r); undefined entries 0"""
    A, g = np.asarray(A, dtype=np.float64), -np.asarray(jtl, dtype=np.float64).reshape(-1)
    rec = np.zeros((plan.pairs, WREC))
    r7 = np.arange(7)
    rows = 7 * plan.key_a[:, None, None] + r7[None, :, None]
    cols = 7 * plan.key_b[:, None, None] + r7[None, None, :]
    rec[:, :49] = A[rows, cols].reshape(plan.pairs, 49)
    rec[:, 49:] = g[7 * plan.key_a[:, None] + r7[None, :]]
    return np.where(record_mask(plan), rec, 0.0)


def dense_of(plan, rec):
    """the records summed back into (lower triangle of A, J^T r): the inverse bookkeeping of ``records_of``"""
    P = 7 * plan.J
    L, g = np.zeros((P, P)), np.zeros(P)
    rec = np.where(record_mask(plan), rec, 0.0)
    for k in range(plan.pairs):
        a, b = plan.key_a[k], plan.key_b[k]
        L[7 * a:7 * a + 7, 7 * b:7 * b + 7] += rec[k, :49].reshape(7, 7)
        if a == b:
            g[7 * a:7 * a + 7] += rec[k, 49:]
    return L, g


def covered(plan, A):
    """every non-zero of A sits in a block of blk_key (or its transpose)"""
    nz = np.abs(np.asarray(A)).reshape(plan.J, 7, plan.J, 7).max(axis=(1, 3)) > 0
    have = np.zeros((plan.J, plan.J), bool)
    have[plan.key_a, plan.key_b] = have[plan.key_b, plan.key_a] = True
    return bool((~nz | have).all())


def split(buf, plan):
    """(records (pairs, 56), matched count) of an SLM_X_PAIR_BLOCKS buffer of the pair-record form"""
    buf = np.asarray(buf, dtype=np.float64).reshape(-1)
    assert buf.size == plan.pairs * WREC + VK_TAIL, (buf.size, plan.pairs)
    return buf[:plan.pairs * WREC].reshape(plan.pairs, WREC), float(buf[plan.pairs * WREC:].sum())


def record_errors(plan, got, want):
    """(largest |difference| over the defined block entries, over the defined J^T r entries)"""
    m = record_mask(plan)
    d = np.where(m, np.abs(got - want), 0.0)
    return float(d[:, :49].max()), float(d[:, 49:].max())
