"""Node graphs for the solver tests: the regular grid of ``synth.make_scene`` at the sizes where the symbolic plan of the
multifrontal solver changes shape, and named irregular topologies (relabelled, disconnected, a hub node, coincident nodes,
a random dense graph, self references and duplicates in the node KNN table), plus frames whose normal matrix has ONE
exactly-zero node block at a chosen place of the elimination order.  Plain NumPy, importable without a GPU: consumed by
``orc.Frame.from_scene`` (tests/test_solver_graph_cases.py) and ``DeviceFrame.from_scene`` (tests/test_gpu_solver_graphs.py).

Every builder returns a ``synth.Scene`` on the 60 x 80 base of the small tests; seeds are fixed; results are cached, and the
tests treat them as read-only."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np

from oracle import lm_oracle as orc
from super_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = dict(H=60, W=80, src_border=5, tgt_border=3)
U_SOLVE = 0.37          # the damping of every single solve of these tests

# grid sizes: 4 = one 28-wide front; 9 / 10 = 63 / 70 scalars, either side of one 64-wide tile; 18 / 19 = the last unsplit leaf
# and the first split at SLM_ND_LEAF; 50 / 51 the same at SLM_ND_LEAF_LATENCY; 64 / 128: P = 7J is a multiple of 64;
# 97: prime, so the grid is a 1 x 97 chain; 100: a 10 x 10 grid, the eighth four-level tree of DEEP_BATCH
GRID_J = (4, 9, 10, 18, 19, 50, 51, 64, 97, 100, 128)


def _scene(J, N, seed, **kw):
    return synth.make_scene(N=N, J=J, seed=seed, **BASE, **kw)


def _grid(J):
    # 1 500 .. 3 000 surfels, more for more nodes
    return _scene(J, 1500 + 1500 * (J - 4) // 124, 200 + J, n_ed_neighbors=min(4, J - 1))


def _grid_k6():
    """num_neighbors 6, num_ED_neighbors 8: the K-generic pair path feeds the fronts"""
    return _scene(64, 2500, 301, n_neighbors=6, n_ed_neighbors=8)


def _shuffled():
    """the J = 128 grid under a random permutation of the node labels: same problem, arbitrary numbering"""
    sc = _scene(128, 3000, 310)
    new_of_old = np.random.default_rng(311).permutation(sc.J)
    old_of_new = np.argsort(new_of_old)
    for name in ("ed_points", "ed_norms", "ed_radii", "ed_knn_idx", "ed_knn_w"):
        setattr(sc, name, np.ascontiguousarray(getattr(sc, name)[old_of_new]))
    sc.ed_knn_idx = np.ascontiguousarray(new_of_old[sc.ed_knn_idx])
    sc.sf_knn_idx = np.ascontiguousarray(new_of_old[sc.sf_knn_idx])
    sc.ed_triangles = np.ascontiguousarray(new_of_old[sc.ed_triangles])
    sc.meta["new_of_old"] = new_of_old
    return sc


def island_sides(sc):
    """(side of every node, side of every surfel) of the cut at the median node x"""
    cut = float(np.median(sc.f64("ed_points")[:, 0]))
    return sc.f64("ed_points")[:, 0] > cut, sc.f64("sf_points")[:, 0] > cut


def _islands():
    """two halves without any coupling: nodes split at the median x, surfel -> node and node -> node neighbours
    recomputed inside each half (weights as the generator computes them)"""
    sc = _scene(128, 3000, 320)
    e64, s64 = sc.f64("ed_points"), sc.f64("sf_points")
    node_side, sf_side = island_sides(sc)
    K, Ke = sc.sf_knn_idx.shape[1], sc.ed_knn_idx.shape[1]
    radii = np.empty(sc.J)
    for side in (False, True):
        nodes = np.nonzero(node_side == side)[0]
        assert len(nodes) > max(K, Ke)
        d2, ii = synth.knn_bruteforce(e64[nodes], e64[nodes], Ke + 1)
        dd = np.sqrt(d2[:, 1:])
        sc.ed_knn_idx[nodes] = nodes[ii[:, 1:]]
        radii[nodes] = dd.mean(axis=1)
        sc.ed_radii[nodes] = radii[nodes].astype(np.float32)
        sc.ed_knn_w[nodes] = synth.softmax_exp_weights(dd, sc.f64("ed_radii")[nodes][:, None]).astype(np.float32)
    for side in (False, True):
        nodes, sfs = np.nonzero(node_side == side)[0], np.nonzero(sf_side == side)[0]
        d2, ii = synth.knn_bruteforce(s64[sfs], e64[nodes], K)
        sc.sf_knn_idx[sfs] = nodes[ii]
        sc.sf_knn_w[sfs] = synth.softmax_exp_weights(np.sqrt(d2), sc.f64("ed_radii")[nodes[ii]]).astype(np.float32)
    assert (node_side[sc.sf_knn_idx] == sf_side[:, None]).all() and (node_side[sc.ed_knn_idx] == node_side[:, None]).all(), \
        "a pair crosses the cut"
    return sc


def _hub():
    """node 0 is a neighbour of every other node: it sits on every separator path"""
    sc = _scene(128, 3000, 330)
    sc.ed_knn_idx[1:, -1] = 0
    return sc


def _coincident():
    """32 nodes at one position: the median split falls back on the node id, their Jacobian blocks coincide"""
    sc = _scene(128, 3000, 340)
    sc.ed_points[:32] = sc.ed_points[0]
    return sc


def _random_dense(n_neighbors=8):
    """node -> node neighbours drawn uniformly from [0, J) at 8 per node (self references and duplicates included), 8 nodes
    per surfel: no geometric separator exists.  Every node of either half of the median split touches the other half, the
    separator is a whole half and the other half is empty: dissect() takes its could-not-split branch at the root, and the
    plan is ONE dense front of 64 nodes (7 pivot tile columns) at either leaf size -- fronts 1, levels 1 (PLANS
    below).  ``n_neighbors=4``: the same graph for batches, whose frames share num_neighbors."""
    sc = _scene(64, 2500, 350, n_neighbors=n_neighbors, n_ed_neighbors=8)
    sc.ed_knn_idx = np.random.default_rng(351).integers(0, sc.J, size=sc.ed_knn_idx.shape).astype(np.int64)
    return sc


def _self_and_dup():
    """a node KNN table that lists the node itself (column 0) and one neighbour twice (columns 1 and 2)"""
    sc = _scene(128, 3000, 360)
    sc.ed_knn_idx[:, 0] = np.arange(sc.J)
    sc.ed_knn_idx[:, 2] = sc.ed_knn_idx[:, 1]
    return sc


_BUILDERS = {f"grid_j{J}": functools.partial(_grid, J) for J in GRID_J}
_BUILDERS.update(grid_j64_k6=_grid_k6, shuffled=_shuffled, islands=_islands, hub=_hub, coincident=_coincident,
                 random_dense=_random_dense,
                 random_dense_k4=functools.partial(_random_dense, 4), self_and_dup=_self_and_dup)
CASES = tuple(_BUILDERS)
TOPOLOGIES = ("shuffled", "islands", "hub", "coincident", "random_dense", "random_dense_k4", "self_and_dup")
# Batches of eight different cases (the frames of one batch share num_neighbors: 4).  DEEP: every tree has four levels when
# dissected to 18-node leaves, so solver_path 4 runs the hybrid form; MIXED: one to four levels, so it falls back to the
# per-level launches, and the slots with fewer levels than the batch maximum idle through the deeper ones.
DEEP_BATCH = ("grid_j97", "grid_j100", "grid_j128", "shuffled", "islands", "hub", "coincident", "self_and_dup")
MIXED_BATCH = ("shuffled", "islands", "hub", "random_dense_k4", "grid_j4", "grid_j19", "grid_j51", "grid_j64")


# (fronts, levels) of every case when a bind dissects to 18-node leaves (SLM_ND_LEAF: solver_path 3 and 4, and 0 for large
# batches) and to 50-node leaves (SLM_ND_LEAF_LATENCY: solver_path 2, and 0 for one or two slots or slots x J <= 8 000)
PLANS = {
    "grid_j4": ((1, 1), (1, 1)), "grid_j9": ((1, 1), (1, 1)), "grid_j10": ((1, 1), (1, 1)), "grid_j18": ((1, 1), (1, 1)),
    "grid_j19": ((3, 2), (1, 1)), "grid_j50": ((5, 3), (1, 1)), "grid_j51": ((5, 3), (3, 2)), "grid_j64": ((7, 3), (3, 2)),
    "grid_j97": ((15, 4), (3, 2)), "grid_j100": ((11, 4), (3, 2)), "grid_j128": ((13, 4), (5, 3)), "grid_j64_k6": ((5, 3), (3, 2)),
    "shuffled": ((13, 4), (5, 3)), "islands": ((15, 4), (7, 3)), "hub": ((13, 4), (5, 3)), "coincident": ((11, 4), (5, 3)),
    "random_dense": ((1, 1), (1, 1)), "random_dense_k4": ((1, 1), (1, 1)), "self_and_dup": ((13, 4), (5, 3)),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return _BUILDERS[name]()


def perturbed_beta(J, seed=9):
    """identity + N(0, 0.01) on the quaternions, N(0, 0.002) on the translations (the perturbation of
    test_c2_assembly_paths_agree_and_match_oracle_terms), the quaternion components then snapped to multiples of 2^-8.

    The Rot term is evaluated in FLOAT32, by the reference, the oracle and the library alike, and two float32 evaluations
    round differently: the oracle widens r = 1 - |q|^2 and J = -2 q to float64 before it forms J^T J and J^T r, the library
    forms them in float32.  At an unsnapped beta the library's JtJ differs from the oracle's by 2e-7 (of 4) and jtl by 3e-9
    in the Rot term alone (data and ARAP terms: 1e-16 relative), which is a backward error of 1 400 - 2 100 P eps and a
    forward error of up to 9e-10 on EVERY solver path, the band included -- nothing a solver test can hold to 64 P eps.
    On the 2^-10 grid |q|^2 and q q^T are exact but the 26-bit products q r still round (jtl 3.7e-9 apart).  With 9-bit
    quaternion components r is a multiple of 2^-16 below 1/8, every product and sum of the term fits float32's 24 bits, the
    Rot parts of the two assemblies are bit-equal (measured: 0 in JtJ and jtl on every case), and the bounds measure the
    solver."""
    rng = np.random.default_rng(seed)
    beta = np.tile([1.0, 0, 0, 0, 0, 0, 0], (J, 1)) + np.concatenate(
        [rng.normal(0, 0.01, (J, 4)), rng.normal(0, 0.002, (J, 3))], axis=1)
    beta[:, :4] = np.round(beta[:, :4] * 256.0) / 256.0
    return beta


def generic_beta(J, seed=9):
    """the same perturbation without the snap: generic low-order bits in the Rot blocks and the right-hand side.  Only for
    comparisons with the library's OWN assembled matrix, which do not depend on how the oracle rounds the Rot term."""
    rng = np.random.default_rng(seed)
    return np.tile([1.0, 0, 0, 0, 0, 0, 0], (J, 1)) + np.concatenate(
        [rng.normal(0, 0.01, (J, 4)), rng.normal(0, 0.002, (J, 3))], axis=1)


def identity_beta(J):
    return np.tile([1.0, 0, 0, 0, 0, 0, 0], (J, 1))


@functools.lru_cache(maxsize=None)
def reference(name, beta="perturbed", opt_kw=()):
    """(A, b, delta, norm(A, 2)): the oracle's JtJ + U_SOLVE I, jtl and Cholesky solution of a case (or failure case, or "split_column") at the
    perturbed (or identity) beta, computed once and read-only"""
    sc = case(name) if name in _BUILDERS else (split_column_case() if name == "split_column" else failure_case(name))
    b0 = perturbed_beta(sc.J) if beta == "perturbed" else identity_beta(sc.J)
    JtJ, jtl, _ = orc.normal_equations(orc.Frame.from_scene(sc), b0, orc.default_opt(**dict(opt_kw)))
    A = JtJ + U_SOLVE * np.eye(len(jtl))
    delta = orc.solve_damped(JtJ, jtl, U_SOLVE)
    for a in (A, jtl, delta):
        a.setflags(write=False)
    return A, jtl, delta, float(np.linalg.norm(A, 2))


def backward_error(A, b, d, norm2):
    """norm(A d - b) / (norm(A, 2) norm(d) + norm(b))"""
    return float(np.linalg.norm(A @ d - b) / (norm2 * np.linalg.norm(d) + np.linalg.norm(b)))


def backward_bound(P):
    """64 P eps: P eps for the solve, 64 for the difference between the library's assembly and the oracle's.
    Largest value measured on the MI355X over the sweep of tests/test_gpu_solver_graphs.py: 0.025 P eps (MEASURED there)."""
    return 64.0 * P * np.finfo(np.float64).eps


# ------------------------------------------------------------------------------------- failure placement
# A frame without the surfels that list ONE chosen node.  The data term then leaves that node's seven rows and columns of JtJ
# exactly zero, and they stay exactly zero under every Schur update (which only subtracts products with those zero columns).
#
# With the data term ALONE (FAIL_OPT_DATA, u0 = 0: the configuration of test_solver_failure_stops_like_the_reference) that
# frame fails -- but so does every frame, and in its first leaf: at the identity the qw column of the data-term Jacobian is
# exactly zero for every node (d R(q) x / d qw = 2 v x x = 0 at v = 0), and away from the identity the quaternion's radial
# direction stays a null direction to rounding (smallest eigenvalue 3e-14 against 60 at the perturbed beta).  No healthy frame
# exists in that configuration, and no zero pivot is confined to the root.  With the Rot term added (FAIL_OPT_ROT, u0 = 0)
# every node block gains 4 q q^T: at the identity that is +4 on qw, the healthy systems are positive definite (condition
# 1e6; all ten iterations of the oracle's loop solve), and the chosen node's block is diag(4, 0, 0, 0, 0, 0, 0) with zero
# off-diagonal rows -- its qx pivot is exactly zero, deterministically, and it is the only one.
FAIL_J = 48                       # the 6 x 8 grid
FAIL_OPT_DATA = (("mesh_arap", False), ("mesh_rot", False))
FAIL_OPT_ROT = (("mesh_arap", False), ("mesh_rot", True))
# (a) fail_corner, a corner of the 6 x 8 grid: eliminated in the first leaf; (b) fail_root, a node of the middle of that grid
# (row 2, column 3): the widest axis is x, the median split cuts between columns 3 and 4, and the separator the analysis keeps
# (a minimum vertex cover of the cut edges) holds this node -- a pivot of the ROOT front, eliminated last when the tree is
# dissected to SLM_ND_LEAF nodes (tests/test_solver_graph_cases.py asserts it on the analysis itself).  At SLM_ND_LEAF_LATENCY
# the 48 nodes are ONE front, whose pivots are in id order: the corner is its first pivot (tile column 0), the middle node
# pivot 19 (tile column 2 of 6) -- so in the task-graph form the flag of (b) never crosses a front boundary.  (c)
# fail_root_j128 closes that: node (3, 7) of the 8 x 16 grid is a pivot of the root front at EITHER leaf size (13 fronts in 4
# levels / 5 fronts in 3 levels), so the zero pivot is the last thing every form meets, two or three levels above the leaves.
FAIL_NODE = {"fail_corner": 0, "fail_root": 2 * 8 + 3, "fail_root_j128": 3 * 16 + 7}
FAIL_GRID = {"fail_corner": (48, (6, 8)), "fail_root": (48, (6, 8)), "fail_root_j128": (128, (8, 16))}
FAILURES = ("fail_corner", "fail_root")          # the J = 48 frames, which also run inside batches of healthy J = 48 frames
FAILURES_ALL = tuple(FAIL_NODE)


@functools.lru_cache(maxsize=None)
def failure_case(name):
    J, grid = FAIL_GRID[name]
    sc = _scene(J, 3000, 401 if J == FAIL_J else 402)
    assert sc.meta["grid"] == grid
    keep = (sc.sf_knn_idx != FAIL_NODE[name]).all(axis=1)
    for k in ("sf_points", "sf_norms", "sf_knn_idx", "sf_knn_w"):
        setattr(sc, k, np.ascontiguousarray(getattr(sc, k)[keep]))
    assert 1500 <= sc.N < 3000
    return sc


@functools.lru_cache(maxsize=None)
def healthy_case(k):
    """the frames that share a batch with a failing one: J = 48 grids, positive definite under FAIL_OPT_ROT at u0 = 0"""
    return _scene(FAIL_J, 3000, 420 + k)


# ------------------------------------------------------------------------------------- the symbolic plan, on the CPU
def coupled_pairs(sc):
    """keys a * J + b (a >= b) of the node pairs that share a surfel, ascending: the pair list of the data term"""
    idx = sc.sf_knn_idx
    a, b = idx[:, :, None], idx[:, None, :]
    keys = (np.maximum(a, b) * sc.J + np.minimum(a, b)).reshape(-1)
    return np.unique(keys).astype(np.uint32)


def nd_harness_command(out, extra=()):
    """The one recipe that builds the host-side symbolic analysis (csrc/slm_nd_host.hip is plain C++) with its harness
    tools/studies/nd/nd_stats.cpp into a shared library (tests/test_nd_host_sanitized.py builds the same two files with
    sanitizer flags).  A missing compiler is an error, not a skip: the placement assertions must not vanish silently."""
    gxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if not gxx:
        raise RuntimeError("the plan tests need a host C++ compiler (g++, c++ or clang++)")
    csrc = os.path.join(ROOT, "python-super_amd", "csrc")
    return [gxx, "-O1", *extra, "-std=c++17", "-shared", "-fPIC", "-I", csrc, "-x", "c++",
            os.path.join(ROOT, "tools", "studies", "nd", "nd_stats.cpp"), os.path.join(csrc, "slm_nd_host.hip"), "-o", out]


def _leaf_sizes():
    """(SLM_ND_LEAF, SLM_ND_LEAF_LATENCY) as csrc/slm_nd.h defines them"""
    text = open(os.path.join(ROOT, "python-super_amd", "csrc", "slm_nd.h")).read()
    return tuple(int(re.search(r"^#define %s (\d+)" % n, text, re.M).group(1)) for n in ("SLM_ND_LEAF", "SLM_ND_LEAF_LATENCY"))


LEAF, LEAF_LATENCY = _leaf_sizes()       # 18: per-level and hybrid forms; 50: the task graph (PLANS is written for these)


@functools.lru_cache(maxsize=None)
def _nd_lib():
    import ctypes as C
    tmp = tempfile.mkdtemp(prefix="nd_plan_")
    atexit.register(shutil.rmtree, tmp, ignore_errors=True)
    so = os.path.join(tmp, "nd_plan.so")
    subprocess.check_call(nd_harness_command(so))
    return C.CDLL(so)


def host_plan(sc, leaf_nodes):
    """The plan that a bind builds for the scene when it dissects down to ``leaf_nodes`` (18: per-level / hybrid forms,
    50: task graph): dict(fronts, levels, node_front (J), node_pos (J), front_depth, front_nv, front_is_leaf); fronts are numbered in
    processing order, deepest level first, so the root is the last one.  Raises without a host compiler."""
    import ctypes as C
    lib = _nd_lib()
    pts = np.ascontiguousarray(sc.ed_points, np.float32)
    knn = np.ascontiguousarray(sc.ed_knn_idx, np.int32)
    pairs = coupled_pairs(sc)
    node_front, node_pos = np.full(sc.J, -1, np.int32), np.full(sc.J, -1, np.int32)
    fronts = np.zeros((sc.J + 1, 3), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib.nd_node_fronts(sc.J, knn.shape[1], p(pts), p(knn), p(pairs), len(pairs), int(leaf_nodes), p(node_front), p(node_pos),
                           p(fronts), len(fronts))
    assert 1 <= n <= len(fronts), n
    return dict(fronts=n, levels=int(fronts[:n, 0].max()) + 1, node_front=node_front, node_pos=node_pos,
                front_depth=fronts[:n, 0].copy(), front_nv=fronts[:n, 1].copy(), front_is_leaf=fronts[:n, 2].astype(bool))


def host_level_schedule(sc):
    """The per-level launch schedule of the scene's plan at SLM_ND_LEAF (the per-level and hybrid forms), deepest level first
    as launch_front_levels walks it: a list of (n_fronts, max_npt, max_nt) -- fronts of the level, the most pivot tile columns
    and the most tile rows (pivot + boundary) of one of them (NDLevelSched, csrc/slm_nd.h)."""
    import ctypes as C
    lib = _nd_lib()
    pts = np.ascontiguousarray(sc.ed_points, np.float32)
    knn = np.ascontiguousarray(sc.ed_knn_idx, np.int32)
    pairs = coupled_pairs(sc)
    stats, fronts = np.zeros(8), np.zeros((sc.J + 1, 4), np.int32)      # per front: depth, pivot nodes, boundary nodes, parent
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    n = lib.nd_stats(sc.J, knn.shape[1], p(pts), p(knn), p(pairs), len(pairs), p(stats), p(fronts), len(fronts), None)
    assert 1 <= n <= len(fronts), n
    depth, npt = fronts[:n, 0], (7 * fronts[:n, 1] + 63) // 64
    nt = npt + (7 * fronts[:n, 2] + 63) // 64
    return [(int((depth == d).sum()), int(npt[depth == d].max()), int(nt[depth == d].max())) for d in range(int(depth.max()), -1, -1)]


@functools.lru_cache(maxsize=None)
def split_column_case():
    """A 16 x 24 grid (J = 384, P = 2 688): at 18-node leaves one level of its tree has 16 fronts of up to six tile rows, so an
    eight-slot batch launches (6 - c) * 16 * 8 = 768 / 640 workgroups for that level's tile columns c = 0 / 1 -- past the 512
    at which launch_front_levels splits the fused panel column into k_fpotrf + k_ftrsm (tests/test_gpu_solver_graphs.py)."""
    return _scene(384, 3000, 884)
