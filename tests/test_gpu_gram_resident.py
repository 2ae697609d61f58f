"""The resident, software-pipelined Jacobian pass (``k_data_gram``): a workgroup walks a contiguous range of its slot's
256-position chunks instead of owning one.  ``SLM_GRAM_WGS`` (read once per solver) sets the workgroups per slot; the
results must not depend on it.  Needs an MI355X (-m gpu).

Frames are of the ``tiny`` size (N <= 3 000, J = 48, 60 x 80: about 13 chunks), so the knob values cover
  1   one workgroup walks every chunk of the slot (and zeroes all of the fronts' pieces);
  2   several chunks per workgroup;
  5   two or three chunks per workgroup, uneven ranges;
  64  one chunk per workgroup at most, and most workgroups with NO chunk (they only share the zeroing).
Checked against the NumPy oracle / the reference's goldens with the tolerances of ``test_gpu_parity.py``
(``test_mid_size_vs_oracle``, ``test_atomic_cross_check_path_agrees``), and against ``data_path = 2`` (one Gram per run,
plain stores), which must come out BITWISE the same at every knob value.

A batch with an unbound slot in the middle cannot reach the kernel: ``slm_run`` refuses it (``check_slots``).  The test
pins that refusal, then binds the slot and solves the batch of three different sizes.
"""
import dataclasses
import functools

import numpy as np
import pytest

from helpers import load_golden, ref_opt, torch_frame
from oracle import lm_oracle as orc

pytestmark = pytest.mark.gpu

KNOBS = [1, 2, 5, 64]
TOL_BETA = 1e-4      # test_gpu_parity.TOL_BETA


@functools.lru_cache(maxsize=None)
def _scene(N, seed, hole=False):
    from super_amd import synth
    sc = synth.make_scene(N=N, J=48, H=60, W=80, seed=seed, src_border=5, tgt_border=3)
    if hole:
        # the targets of the image's left half are invalid: the tuple-sorted order is spatially coherent, so whole chunks
        # of positions have no match (zero rows, records of zeros)
        valid = sc.valid.copy().reshape(sc.H, sc.W)
        imap = sc.index_map.copy()
        valid[:, : sc.W // 2] = False
        imap[:, : sc.W // 2] = -1
        sc = dataclasses.replace(sc, valid=valid.reshape(-1), index_map=imap)
    return sc


@functools.lru_cache(maxsize=None)
def _oracle(N, seed, hole=False):
    trace = []
    beta = orc.lm(orc.Frame.from_scene(_scene(N, seed, hole)), orc.default_opt(), trace=trace)
    return beta, trace


def _lm(sc, data_path=0):
    from super_amd.LM import LM_Solver
    o = ref_opt(orc.default_opt())
    o.slm_data_path = data_path
    lm = LM_Solver(o)
    beta = lm.LM(*torch_frame(sc)).cpu().numpy()
    return beta, lm.last_records[0]


_slab_ref = {}     # data_path = 2 results of the first knob value that ran: every other one must equal them bitwise


def _same_as_first(key, beta, recs):
    got = (beta, [(r["loss"], r["u"], r["accepted"], r["M_grad"], r["M_loss"]) for r in recs])
    want = _slab_ref.setdefault(key, got)
    np.testing.assert_array_equal(got[0], want[0])
    assert got[1] == want[1]


@pytest.mark.parametrize("fuse", ["1", "0"])
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("hole", [False, True])
def test_one_frame_any_workgroup_count(monkeypatch, knob, fuse, hole):
    """LM on one tiny frame (full targets / targets invalid over half the image), zeroing fused or a launch of its own."""
    monkeypatch.setenv("SLM_GRAM_WGS", str(knob))
    monkeypatch.setenv("SLM_FUSE_BEGIN", fuse)
    sc = _scene(3000, 7, hole)
    want, trace = _oracle(3000, 7, hole)
    beta, recs = _lm(sc)
    assert all(r["status"] == 0 for r in recs)
    np.testing.assert_allclose(beta, want, rtol=0, atol=TOL_BETA)
    np.testing.assert_allclose([r["loss"] for r in recs], [t["loss"] for t in trace], rtol=1e-6)
    assert [r["M_loss"] for r in recs] == [t["M_loss"] for t in trace]
    if hole:
        full = _oracle(3000, 7, False)[1]
        assert 0 < trace[0]["M_loss"] < 0.75 * full[0]["M_loss"]      # the hole removes matches, not all of them
    beta2, recs2 = _lm(sc, data_path=2)
    _same_as_first(("one", hole), beta2, recs2)
    np.testing.assert_allclose(beta2, want, rtol=0, atol=TOL_BETA)


@pytest.mark.parametrize("knob", KNOBS)
def test_normal_equations_agree_with_the_per_run_slab(monkeypatch, knob):
    """The merged records against data_path = 2 at the same point, tolerances of test_atomic_cross_check_path_agrees.
    (Nothing bitwise here: prepareCostTerm assembles through the band path, whose entry order per pair changes from bind
    to bind at the rounding level whatever the Jacobian pass does; the bitwise checks are on the LM path.)"""
    import torch
    from super_amd.LM import LM_Solver
    monkeypatch.setenv("SLM_GRAM_WGS", str(knob))
    g, sc, opt = load_golden("s60x80_j48")
    sf, inputs, new_data = torch_frame(sc)
    beta = torch.from_numpy(g["b1_beta"]).cuda()
    outs = {}
    for path in (0, 2):
        o = ref_opt(opt)
        o.slm_data_path = path
        jtj, jtl = LM_Solver(o).prepareCostTerm(sf, inputs, new_data, beta, grad=True)
        outs[path] = (jtj.cpu().numpy(), jtl.cpu().numpy())
    scale = np.abs(outs[0][0]).max()
    np.testing.assert_allclose(outs[0][0], outs[2][0], rtol=0, atol=1e-12 * scale)
    np.testing.assert_allclose(outs[0][1], outs[2][1], rtol=0, atol=1e-11)
    np.testing.assert_allclose(outs[0][1].reshape(-1), g["b1_jtl"], rtol=0, atol=1e-8)


BATCH = ((3000, 11), (2100, 12), (1300, 13))     # three slots of different N: different chunk counts per slot


@functools.lru_cache(maxsize=None)
def _batch_singles():
    return tuple(_lm(_scene(N, s))[0] for N, s in BATCH)


@pytest.mark.parametrize("knob", KNOBS)
def test_batch_of_three_sizes(monkeypatch, knob):
    from super_amd.LM import LM_Solver
    singles = _batch_singles()                    # (at the default workgroup count)
    monkeypatch.setenv("SLM_GRAM_WGS", str(knob))
    lmb = LM_Solver(ref_opt(orc.default_opt()), max_frames=3)
    batch = lmb.LM_batch([torch_frame(_scene(N, s)) for N, s in BATCH])
    for a, b in zip(singles, batch):
        np.testing.assert_allclose(b.cpu().numpy(), a, rtol=0, atol=1e-7)     # test_batch_of_frames_matches_single
    np.testing.assert_allclose(batch[1].cpu().numpy(), _oracle(*BATCH[1])[0], rtol=0, atol=TOL_BETA)


def test_chunk_shapes_of_the_fixtures():
    """What the cases above rely on: about 13 chunks for the largest frame, and among the frames a last chunk with idle
    waves (positions not a multiple of 256; they are padded to a multiple of 64, so its last wave holds padding)."""
    import torch
    from super_amd.engine import DeviceFrame, Engine
    dev = torch.device("cuda", 0)
    pos = []
    for N, s in BATCH + ((3000, 7),):
        eng = Engine(dev)
        eng.bind(0, DeviceFrame.from_scene(_scene(N, s), dev, state_f64=True))
        pos.append(int(eng.plan_info(0)["positions"]))
        eng.close()
    assert all(p % 64 == 0 for p in pos)
    assert 8 <= (max(pos) + 255) // 256 <= 20
    assert len({(p + 255) // 256 for p in pos[:3]}) == 3
    assert any(p % 256 != 0 for p in pos), pos


def test_unbound_middle_slot_is_refused_then_solved(monkeypatch):
    import torch
    from super_amd import _lib
    from super_amd.engine import DeviceFrame, Engine
    monkeypatch.setenv("SLM_GRAM_WGS", "5")
    dev = torch.device("cuda", 0)
    eng = Engine(dev, max_frames=3)
    frames = [DeviceFrame.from_scene(_scene(N, s), dev, state_f64=True) for N, s in BATCH]
    eng.bind(0, frames[0])
    eng.bind(2, frames[2])
    with pytest.raises(_lib.SuperLMError):
        eng.run(3)
    eng.bind(1, frames[1])
    eng.run(3)
    for i, want in enumerate(_batch_singles()):
        np.testing.assert_allclose(eng.beta(i).cpu().numpy(), want, rtol=0, atol=1e-7)
    eng.close()


@pytest.mark.parametrize("knob", KNOBS)
def test_two_share_shard_split(monkeypatch, knob):
    """One frame over two ranks ([wg_lo, wg_hi) in chunk units), the shares summed by the exchange: the checks of
    test_surfel_sharded_lm_reproduces_the_single_gpu_solve."""
    from test_gpu_parity import _run_emulated_ranks
    monkeypatch.setenv("SLM_GRAM_WGS", str(knob))
    g, o, betas, recs = _run_emulated_ranks("s60x80_j48", 2)
    np.testing.assert_array_equal(betas[1], betas[0])
    assert [x["accepted"] for x in recs[1]] == [x["accepted"] for x in recs[0]]
    assert [x["loss"] for x in recs[1]] == [x["loss"] for x in recs[0]]
    np.testing.assert_allclose(betas[0], g["lm_beta"], rtol=0, atol=TOL_BETA)
    np.testing.assert_allclose([x["loss"] for x in recs[0]], g["lm_loss"], rtol=1e-6)
    assert [x["accepted"] for x in recs[0]] == [bool(a) for a in g["lm_accepted"]]
    assert recs[0][0]["M_grad"] == len(g["b0_match"])


@pytest.mark.parametrize("no_reuse", ["0", "1"])
@pytest.mark.parametrize("knob", KNOBS)
def test_rejected_iteration_with_and_without_reuse(monkeypatch, knob, no_reuse):
    """The fixture with a rejected step, run on past it: records kept (the pass is skipped, only the zeroing runs) or
    recomputed.  data_path = 2 bitwise across knob values AND across reuse / recompute; the merged records against the
    reference's golden."""
    import torch
    from super_amd.engine import DeviceFrame, Engine
    monkeypatch.setenv("SLM_GRAM_WGS", str(knob))
    monkeypatch.setenv("SLM_NO_REUSE", no_reuse)
    g, sc, opt = load_golden("s60x80_j48_reject")
    n_gold = len(g["lm_accepted"])
    n_it = int(opt.num_optimize_iterations) + 8
    dev = torch.device("cuda", 0)
    out = {}
    for path in (2, 0):
        eng = Engine(dev, data_path=path, num_iterations=n_it)
        eng.bind(0, DeviceFrame.from_scene(sc, dev, state_f64=True))
        eng.run(1)
        out[path] = (eng.beta(0).cpu().numpy(), eng.records(0))
        eng.close()
    acc = [r["accepted"] for r in out[2][1]]
    assert acc[:n_gold] == [bool(a) for a in g["lm_accepted"]]
    assert False in acc[:-1]                         # a rejected iteration that is followed by another one
    _same_as_first("reject", *out[2])
    assert [r["accepted"] for r in out[0][1]][:n_gold] == [bool(a) for a in g["lm_accepted"]]
    np.testing.assert_allclose([r["loss"] for r in out[0][1]][:n_gold], g["lm_loss"], rtol=1e-6, atol=1e-12)
    np.testing.assert_allclose(out[0][0], out[2][0], rtol=0, atol=1e-7)
