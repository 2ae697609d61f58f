"""Case table, CPU references and the emulated-rank driver of the surfel-sharded LM tests (test_lm_shard_cases.py pins the
fixtures on the CPU, test_gpu_lm_sharded.py runs them on the device).  No GPU is touched at import.

A sharded rank (``slm_set_shard(rank, world)``, include/super_lm.h) evaluates a share of the frame's data term and all the
regularisers.  Its shares, fixed at the bind (``bind_shard_share``, csrc/slm_bind.hip):
  pair form (weighted, or num_neighbors != 4)   Jacobian pass: positions [lo, hi) of the neighbour-set-ordered list sf_perm;
                                                loss pass: surfels [lo, hi) of the caller's order
  tuple form (num_neighbors == 4, unweighted)   both passes: 256-position workgroups of the tuple-sorted list
  slm_loss / slm_assemble (parity entry points) surfels [lo, hi) of the caller's order in the pair form, in slm_loss in the
                                                tuple form too; slm_assemble of the tuple form: the rank's workgroups
with lo = N r // W, hi = N (r + 1) // W.  Per iteration the ranks sum their pair records (with the matched count behind
them), take rank 0's step and sum their data-loss partials.  The cases below sit where that can go wrong: every family
(unweighted K = 1, 3, 4, 6, 8; hard / soft / truncation weights at K = 4 and 6) at world 2, 3 and 4; a rank whose share
matches nothing; a rank whose share matches but weighs nothing; bounds on multiples of 64 and 256 and inside a wave; shares
without a surfel; float32 state; the solver forms; batches of unlike N.

References: oracle/lm_oracle.py (unweighted) and lm_weight_model.py (weighted) -- no new physics here.  A share's reference
is the same model restricted to the matched surfels with index in [lo, hi)."""
import dataclasses
import functools

import numpy as np

import lm_corr_model as lcm
import lm_weight_model as lwm
import test_gpu_lm_weights as tw          # scenes, CONFIGS and `decisive` of the weights tests (no GPU at import)
from gf_shape_cases import reorder_surfels
from helpers import load_golden
from oracle import lm_oracle as orc

CONFIGS = dict(tw.CONFIGS)               # "hard": (1, 0.0), "soft": (2, 0.0), "trunc": (0, 2e-5)
CONFIGS[None] = (0, 0.0)
CLASSES = dict(tw.CLASSES)
CLASSES[3] = 3
WORLDS = (2, 3, 4)
UNWEIGHTED_K = (1, 3, 4, 6, 8)
WEIGHTED_K = (4, 6)
SLM_X_PAIR_BLOCKS, SLM_X_DELTA, SLM_X_DATA_LOSS = 0, 1, 2      # include/super_lm.h (checked against _lib in the driver)
UNSUPPORTED, UNBOUND = 5, 4
GOLDEN_EXTRA = 8                          # the reject fixtures run on past their rejected iteration (test_gpu_parity.py)

BIND_TEXT = b"slm_bind_frame: sharded frames need the multifrontal data paths (data_path 0 or 2, J < 65536)"
STEP_TEXT = b"sharded LM step: every slot needs a multifrontal data path (tuple-sorted or K-generic) and the ND solver"


# ------------------------------------------------------------------------------------------------------------------ scenes
def _make(N, J, K, seed, holes=0.01, classes=None, border=4):
    from super_amd import synth
    return synth.make_scene(N=N, J=J, H=60, W=80, seed=seed, n_neighbors=K, src_border=border, tgt_border=3, tgt_holes=holes,
                            semantic=True, num_classes=classes or CLASSES.get(K, 3))


def identity(J):
    return np.tile(np.array([1.0, 0, 0, 0, 0, 0, 0]), (J, 1))


def _leading(sc, first):
    """``sc`` with the surfels ``first`` (ascending) moved to the front, the others behind them in their order: points,
    normals, KNN rows, weights and semantic rows alike"""
    rest = np.setdiff1d(np.arange(sc.N), first)
    return reorder_surfels(sc, np.concatenate([first, rest]))


ZERO_WEIGHT_SEED = 87                     # the first seed from 60 on with at least N / 4 = 300 hard weights 0 at identity (320)


@functools.lru_cache(maxsize=None)
def scene(name):
    """The scene of a name (shared, do not modify):
      k<K>       the 1200-surfel / 40-node scene of test_gpu_lm_weights.py at num_neighbors K
      n65        its wave-and-one-lane scene (K = 4, 12 nodes)
      hole<K>    k<K> with tgt_holes = 0.1, the surfels unmatched at identity in front (empty_share)
      zw4        k4 with the surfels of hard weight 0 at identity in front (zero_weight_share)
      a<N>       N surfels at K = 4 (aligned: a1024 / 40 nodes, a256 / 12 nodes; inside_a_wave: a257 / 12 nodes)
      t<N>       N = 3, 1, 0 surfels at K = 4, 12 nodes (tiny)
      golden:<name>  the scene of a committed golden"""
    if name.startswith("golden:"):
        return load_golden(name[7:])[1]
    if name in ("n65",) or (name[0] == "k" and int(name[1:]) in tw.CLASSES):
        return tw._scene(name)
    if name[0] == "k":
        K = int(name[1:])
        return _make(1200, 40, K, 60 + K)
    if name.startswith("hole"):
        K = int(name[4:])
        sc = _make(1200, 40, K, 60 + K, holes=0.1)
        t = orc.data_term(orc.Frame.from_scene(sc), identity(sc.J), 1.0)
        return _leading(sc, np.setdiff1d(np.arange(sc.N), t.match))
    if name == "zw4":
        sc = _make(1200, 40, 4, ZERO_WEIGHT_SEED)
        ww = lwm.weights(orc.Frame.from_scene(sc), lwm.sem_of(sc), identity(sc.J), 1)
        return _leading(sc, ww.t.match[ww.w == 0.0])
    if name[0] == "a":
        N = int(name[1:])
        return _make(N, 40 if N > 512 else 12, 4, 70 + N % 7, classes=3)
    if name[0] == "t":
        N = int(name[1:])
        return _make(N, 12, 4, 90 + N, holes=0.0, classes=2, border=6)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def frame(name):
    return orc.Frame.from_scene(scene(name))


@functools.lru_cache(maxsize=None)
def sem(name):
    sc = scene(name)
    return lwm.sem_of(sc) if sc.num_classes else None


def perturbed(name):
    return lcm.random_beta(scene(name).J, 17, rot=0.01, trans=0.002)


def golden_opt(name):
    return load_golden(name[7:])[2] if name.startswith("golden:") else orc.default_opt()


# ------------------------------------------------------------------------------------------------------------------- cases
@dataclasses.dataclass(frozen=True)
class ShardCase:
    """A scene, the weights' configuration (None: unweighted), the number of ranks, the state dtype, the solver form and the
    number of iterations of its loop"""
    scene: str
    cfg: str
    world: int
    state_f64: bool = True
    solver_path: int = 0
    iters: int = 10

    @property
    def id(self):
        return (f"{self.scene.replace('golden:', '')}-{self.cfg or 'plain'}-W{self.world}" + ("" if self.state_f64 else "-f32") +
                (f"-sp{self.solver_path}" if self.solver_path else ""))

    @property
    def seg_pp(self):
        return CONFIGS[self.cfg]

    @property
    def pair_form(self):
        """the K-generic pair records (weighted, or num_neighbors != 4); else the tuple-sorted form"""
        return self.cfg is not None or scene(self.scene).sf_knn_idx.shape[1] != 4

    @property
    def opt(self):
        o = golden_opt(self.scene)
        o.num_optimize_iterations = self.iters
        return o


FAMILIES = ([ShardCase(f"k{K}", None, W) for K in UNWEIGHTED_K for W in WORLDS] +
            [ShardCase(f"k{K}", cfg, W) for cfg in ("hard", "soft", "trunc") for K in WEIGHTED_K for W in WORLDS])
# rank 0 of 4 matches nothing at identity (the frame does)
EMPTY_SHARE = [ShardCase("hole4", "hard", 4), ShardCase("hole6", None, 4), ShardCase("hole4", None, 4), ShardCase("hole6", "soft", 4)]
# rank 0 of 4 matches, every hard weight of its share 0 at identity
ZERO_WEIGHT_SHARE = [ShardCase("zw4", "hard", 4)]
ALIGNED = [ShardCase("a1024", "soft", 4), ShardCase("a1024", None, 4), ShardCase("a256", "hard", 4), ShardCase("a256", None, 4)]
INSIDE_A_WAVE = [ShardCase(n, cfg, W) for n, cfg in (("a257", "trunc"), ("a257", None), ("n65", "hard"), ("n65", None)) for W in (2, 3)]
F32 = [ShardCase("k6", "soft", 3, state_f64=False), ShardCase("k4", None, 2, state_f64=False)]
SOLVER_FORMS = [ShardCase("k4", None, 2, solver_path=2), ShardCase("k4", None, 2, solver_path=3),
                ShardCase("k6", "soft", 3, solver_path=2), ShardCase("k4", "hard", 3, solver_path=3)]
GOLDENS = [ShardCase("golden:s60x80_j48_reject", None, 2, iters=10 + GOLDEN_EXTRA),
           ShardCase("golden:s60x80_j48_k6", None, 3, iters=10 + GOLDEN_EXTRA)]
LOOPS = FAMILIES + EMPTY_SHARE + ZERO_WEIGHT_SHARE + ALIGNED + INSIDE_A_WAVE + F32 + SOLVER_FORMS + GOLDENS
POINTS = FAMILIES                                   # the cases of the one-evaluation checks (A)

# tiny and degenerate frames: what the bind code says must happen (bind_data_plan, bind_shard_share; csrc/slm_bind.hip).
#   N = 3, N = 1: four tuples per surfel, so the tuple-sorted plan exists (n_tuples > 0) and, weighted, the pair plan
#                 (n_blocks > 0); the symbolic plan depends on the node graph only -> they RUN, the ranks without a surfel
#                 (and, in the tuple form, without a workgroup) adding exactly nothing
#   N = 0:        no tuple, the plan is empty, bind_data_plan leaves the slot on the per-entry form, which a sharded
#                 solver refuses at the bind
TINY = [(ShardCase("t3", None, 4), "runs"), (ShardCase("t3", "hard", 4), "runs"), (ShardCase("t1", None, 2), "runs"),
        (ShardCase("t1", "soft", 2), "runs"), (ShardCase("t0", None, 2), ("bind", UNSUPPORTED, BIND_TEXT)),
        (ShardCase("t0", "hard", 2), ("bind", UNSUPPORTED, BIND_TEXT))]

# batches: three slots of unlike N in one set of launches
BATCH_WEIGHTED = (("k4", "n65", "hole4"), "hard", 3)
BATCH_PLAIN = ("k4", "a257", "a1024")               # unweighted, the tuple form; at solver_path 0, 3 and 4
ALL_CASES = LOOPS + [c for c, _ in TINY] + [ShardCase(n, BATCH_WEIGHTED[1], BATCH_WEIGHTED[2]) for n in BATCH_WEIGHTED[0]] + \
    [ShardCase(n, None, 3) for n in BATCH_PLAIN]


# ------------------------------------------------------------------------------------------------------------------ shares
def bounds(N, W):
    """[lo, hi) of every rank's share: bind_shard_share's N r / W in integers"""
    return [(N * r // W, N * (r + 1) // W) for r in range(W)]


def conditions(name, cfg, beta):
    """the weights of the matched surfels at beta, with the model's conditions asserted (no surfel is excluded)"""
    seg_mode, pp_max = CONFIGS[cfg]
    ww = lwm.weights(frame(name), sem(name), beta, seg_mode, pp_max)
    lwm.check_conditions(ww, seg_mode, pp_max)
    return ww


def share_losses(name, cfg, beta, W, lam=1.0):
    """[(sum w r^2, matched count)] per rank of W over the matched surfels of its caller-order window, then the frame's"""
    ww = conditions(name, cfg, beta)
    per = ww.w * (lam * ww.t.r) ** 2
    out = []
    for lo, hi in bounds(len(frame(name).sf_points), W):
        m = (ww.t.match >= lo) & (ww.t.match < hi)
        out.append((float(per[m].sum()), int(m.sum())))
    whole = lwm.data_loss(frame(name), sem(name), beta, lam, *CONFIGS[cfg])
    return out, whole


def _rot32(beta, lam, A, b):
    """adds the Rot term with its products rounded to float32, as the reference (and the library) forms them"""
    t = orc.rot_term(beta, lam, grad=True)
    jv, r = t.Jq.astype(np.float32), t.r.astype(np.float32)
    jtj = (jv[:, :, None] * jv[:, None, :]).astype(np.float64)
    jtr = (jv * r[:, None]).astype(np.float64)
    base = 7 * np.arange(len(jv))
    for c in range(4):
        b[base + c] -= jtr[:, c]
        for d in range(4):
            A[base + c, base + d] += jtj[:, c, d]
    return A, b


def full_system(name, cfg, beta):
    """the model's normal equations (JtJ, jtl, matched count), Rot products in float32 (test_gpu_lm_weights._system_rot32)"""
    opt = orc.default_opt()
    A, b, M = lwm.normal_equations(frame(name), sem(name), beta, orc.default_opt(mesh_rot=False), *CONFIGS[cfg])
    A, b = _rot32(beta, opt.mesh_rot_weight, A, b)
    return A, b, M


def reg_system(name, beta):
    """the same without the data term: what every rank adds whatever its share"""
    opt = orc.default_opt()
    A, b, _ = orc.normal_equations(frame(name), beta, lwm._no_data(orc.default_opt(mesh_rot=False)))
    A, b = _rot32(beta, opt.mesh_rot_weight, np.array(A), np.array(b))
    return A, b


@functools.lru_cache(maxsize=None)
def model_trace(name, cfg, iters=10):
    """(final beta, trace) of the model's loop from identity, its conditions asserted at every beta (shared, do not modify)"""
    fr, trace = frame(name), []
    opt = golden_opt(name)
    opt.num_optimize_iterations = iters
    if cfg is None:
        beta = orc.lm(fr, opt, trace=trace)
    else:
        beta = lwm.lm(fr, sem(name), opt, *CONFIGS[cfg], trace=trace, on_beta=lambda b: conditions(name, cfg, b))
    return beta, trace


# ------------------------------------------------------------------------------------------------------ emulated-rank driver
class Ranks:
    """One batch of frames split over ``world`` emulated ranks: one solver context (``Engine``) per rank on this GPU, each
    with ``slm_enable_data_weights`` (``cfg``), then ``slm_set_shard(rank, world)``, then its slots bound with their semantic
    inputs.  The all-reduce of the pair records and of the data-loss partials and the broadcast of delta are emulated by
    combining the ranks' exchange buffers (``slm_lm_exchange_get`` / ``_set``).  ``scenes``: one ``synth.Scene`` per slot,
    ``sems``: their semantic inputs (``lm_weight_model.sem_of``) where the configuration has a semantic weight.
    ``ranks``: the subset of ranks to build (default all)."""

    def __init__(self, scenes, cfg, world, state_f64=True, solver_path=0, iters=10, sems=None, ranks=None, exchange_data=True,
                 bind=True, **engine_kw):
        import torch
        from super_amd import _lib
        from super_amd.engine import Engine
        assert (_lib.SLM_X_PAIR_BLOCKS, _lib.SLM_X_DELTA, _lib.SLM_X_DATA_LOSS) == (SLM_X_PAIR_BLOCKS, SLM_X_DELTA, SLM_X_DATA_LOSS)
        self.torch, self._lib = torch, _lib
        self.dev = torch.device("cuda", 0)
        self.scenes, self.sems, self.n = list(scenes), sems or [None] * len(scenes), len(scenes)
        self.cfg = CONFIGS[cfg] if (cfg is None or isinstance(cfg, str)) else cfg
        self.world, self.state_f64, self.iters = world, state_f64, iters
        self.exchange_data = exchange_data          # (False: a solver without the data term has nothing to sum)
        self.keep = {}
        self.es = []
        for r in (range(world) if ranks is None else ranks):
            e = Engine(self.dev, max_frames=self.n, num_iterations=iters, solver_path=solver_path, **engine_kw)
            self.es.append(e)
            if self.cfg != (0, 0.0):
                _lib.check(e.lib.slm_enable_data_weights(e.h, self.cfg[0], self.cfg[1]), "slm_enable_data_weights")
            if r is not None:                        # (None: an unsharded handle, see ``unsharded``)
                _lib.check(e.lib.slm_set_shard(e.h, r, world), "slm_set_shard")
        self.lib = self.es[0].lib
        self.st = self.es[0].stream
        if bind:
            self.bind()

    def bind_slot(self, e, slot, semantic=True):
        from super_amd.engine import DeviceFrame
        e.bind(slot, DeviceFrame.from_scene(self.scenes[slot], self.dev, state_f64=self.state_f64))
        if semantic and self.cfg[0]:
            t = lambda a, dt: self.torch.from_numpy(np.ascontiguousarray(a)).to(device=self.dev, dtype=dt)
            s = self.sems[slot]
            seg, sc, tc = t(s.sf_seg, self.torch.int32), t(s.sf_seg_conf, self.torch.float32), t(s.tgt_seg_conf, self.torch.float32)
            self.keep[(id(e), slot)] = (seg, sc, tc)
            self._lib.check(e.lib.slm_bind_data_semantic(e.h, slot, sc.shape[1], seg.data_ptr(), sc.data_ptr(), tc.data_ptr(), e.stream),
                            "slm_bind_data_semantic")

    def bind(self):
        for e in self.es:
            for slot in range(self.n):
                self.bind_slot(e, slot)

    def set_beta(self, beta, slot=0):
        b = self.torch.from_numpy(np.ascontiguousarray(beta)).to(self.dev)
        for e in self.es:
            self._lib.check(e.lib.slm_set_beta(e.h, slot, b.data_ptr(), e.stream), "slm_set_beta")
        self.torch.cuda.synchronize()

    def loss(self, e, slot=0):
        out = self.torch.zeros(4, dtype=self.torch.float64, device=self.dev)
        self._lib.check(e.lib.slm_loss(e.h, slot, out.data_ptr(), e.stream), "slm_loss")
        return out.cpu().numpy()

    def assemble(self, e, slot=0):
        P = 7 * self.scenes[slot].J
        A = self.torch.empty((P, P), dtype=self.torch.float64, device=self.dev)
        b = self.torch.empty(P, dtype=self.torch.float64, device=self.dev)
        self._lib.check(e.lib.slm_assemble(e.h, slot, A.data_ptr(), b.data_ptr(), e.stream), "slm_assemble")
        return A.cpu().numpy(), b.cpu().numpy()

    def exchange_size(self, e, slot, what):
        import ctypes as C
        n = C.c_int64(-1)
        self._lib.check(e.lib.slm_lm_exchange_size(e.h, slot, what, C.byref(n)), "slm_lm_exchange_size")
        return n.value

    def get(self, e, slot, what):
        buf = self.torch.empty(self.exchange_size(e, slot, what), dtype=self.torch.float64, device=self.dev)
        self._lib.check(e.lib.slm_lm_exchange_get(e.h, slot, what, buf.data_ptr(), e.stream), "slm_lm_exchange_get")
        return buf

    def exchange(self, what, combine):
        """every slot's buffer ``what`` of every rank combined and set back into every rank; returns the ranks' own buffers
        of slot 0 as they were"""
        first = None
        for slot in range(self.n):
            bufs = [self.get(e, slot, what) for e in self.es]
            first = first or bufs
            out = combine(bufs)
            for e in self.es:
                self._lib.check(e.lib.slm_lm_exchange_set(e.h, slot, what, out.data_ptr(), e.stream), "slm_lm_exchange_set")
        return first

    def call(self, fn):
        for e in self.es:
            self._lib.check(getattr(e.lib, fn)(e.h, self.n, e.stream), fn)

    def grad_and_exchange(self):
        self.call("slm_lm_grad_local")
        return self.exchange(SLM_X_PAIR_BLOCKS, lambda b: self.torch.stack(b).sum(0)) if self.exchange_data else None

    def step(self):
        """one LM iteration of every rank in lock-step"""
        self.grad_and_exchange()
        self.call("slm_lm_solve")
        self.exchange(SLM_X_DELTA, lambda b: b[0].clone())
        self.call("slm_lm_loss_local")
        if self.exchange_data:
            self.exchange(SLM_X_DATA_LOSS, lambda b: self.torch.stack(b).sum(0))
        self.call("slm_lm_accept")

    def run(self):
        for _ in range(self.iters):
            self.step()
        return self.results()

    def results(self):
        """[[(beta, records) per slot] per rank]"""
        return [[(e.beta(i).cpu().numpy(), e.records(i)) for i in range(self.n)] for e in self.es]

    def close(self):
        for e in self.es:
            e.close()
        self.es = []


def case_ranks(case, **kw):
    return Ranks([scene(case.scene)], case.cfg, case.world, case.state_f64, case.solver_path, case.iters, sems=[sem(case.scene)],
                 **_engine_kw(case.opt), **kw)


def _engine_kw(opt):
    return dict(use_data=bool(opt.sf_point_plane), use_arap=bool(opt.mesh_arap), use_rot=bool(opt.mesh_rot),
                w_data=float(opt.sf_point_plane_weight), w_arap=float(opt.mesh_arap_weight), w_rot=float(opt.mesh_rot_weight),
                phase_test=opt.phase == "test")


def unsharded(scenes, cfg, state_f64=True, solver_path=0, iters=10, sems=None, opt=None):
    """[(beta, records)] per slot of ``slm_run`` on one fresh unsharded handle, and its ``slm_debug_last_solver_form``"""
    R = Ranks(scenes, cfg, 1, state_f64, solver_path, iters, sems=sems, ranks=[None], **_engine_kw(opt or orc.default_opt()))
    e = R.es[0]
    e.run(R.n)
    out = [(e.beta(i).cpu().numpy(), e.records(i)) for i in range(R.n)]
    form = e.lib.slm_debug_last_solver_form(e.h)
    R.close()
    return out, form
