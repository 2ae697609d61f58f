"""What test_gpu_depth_edges.py relies on, pinned on the CPU: every case of depth_edge_cases.py hits the edge it names, its inputs
are the recorded ones, and the NumPy oracle reproduces what the reference itself gave on it (tests/golden/dp_edges.npz) at the
tolerances of test_depth_oracle.py -- discrete fields and points bit for bit -- so that the oracle may stand in where the
reference cannot run (depth_edge_cases.ORACLE_ONLY).  The oracle had only ever been pinned at 60 x 80."""
import functools
import os

import numpy as np
import pytest

import depth_edge_cases as dec
from oracle import depth_oracle as dpo
from test_depth_oracle import check

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dp_edges.npz")


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLD) as g:
        return {k: g[k] for k in g.files}


@functools.lru_cache(maxsize=None)
def case(name):
    """(base, okw) of a case; shared between tests, never written to."""
    base, okw = dec.build(name)
    return base, okw


@functools.lru_cache(maxsize=None)
def oracle(name):
    base, okw = case(name)
    with np.errstate(all="ignore"):
        return dec.run_oracle(base, okw)


def reference(name):
    """The reference's recording of a case, the oracle's outputs where the reference cannot run it."""
    return oracle(name) if name in dec.ORACLE_ONLY else dec.expand_golden(golden(), name, case(name)[0])


def test_the_recording_holds_every_case_the_reference_can_run():
    assert set(dec.ORACLE_ONLY) <= {"sem_delall", "sem_one", "sem_absent", "sem_255", "sem_c4"}
    assert tuple(golden()["cases"]) == dec.RECORDED
    assert len(dec.CASES) == 6 * 8 + 3 + 3 + 8 + 7 and max(H * W for H, W in dec.SIZES) <= 61 * 83
    assert os.path.getsize(GOLD) < 720 * 1024
    # the frames that must come out empty: superv2 on images with H <= int(0.1 * W), every class deleted, a mask dilated away
    assert set(dec.EMPTY) == {f"s{s}_{v}" for s in ("8x131", "17x257") for v in ("v2", "v2range", "v2ssim")} | {"raft_k5", "sem_delall"}


@pytest.mark.parametrize("name", list(dec.CASES))
def test_case_hits_its_edge(name):
    dec.check_predicate(name, oracle(name), case(name)[0])
    if name not in dec.ORACLE_ONLY:
        dec.check_predicate(name, reference(name), case(name)[0])


@pytest.mark.parametrize("name", dec.RECORDED)
def test_oracle_reproduces_the_reference(name):
    ref = reference(name)                      # (checks the input digest)
    out = oracle(name)
    for k in ("points", "norms", "radii", "confs", "disp_conf"):
        if k in ref:                             # non-finite values sit where the reference has them
            np.testing.assert_array_equal(np.isnan(out[k]), np.isnan(ref[k]))
            np.testing.assert_array_equal(np.isinf(out[k]), np.isinf(ref[k]))
    check(out, ref, "")
    T = int(ref["valid"].sum())
    for k, (dt, tail) in dec.REF_LAYOUT.items():
        if k in ref:
            assert out[k].dtype == ref[k].dtype == dt and out[k].shape == ref[k].shape == (T,) + tail, k


def test_nan_is_not_inval_but_never_valid():
    """superv1: ``NaN <= 0`` and ``NaN > 1.5`` are both false, so the invalid map misses a NaN depth; only the NaN test on the
    normal keeps it (and its four neighbours) out of the frame.  superv2 keeps every depth but 0."""
    for name in ("nf_v1", "nf_v1n8", "nf_v2"):
        ref, d = reference(name), case(name)[0]["depth"]
        nan = np.isnan(d)
        assert nan.sum() == 3 and not ref["inval"][nan].any() and not ref["valid_map"][nan].any()
    assert reference("nf_v1")["inval"][dec.NF_INF] and not reference("nf_v2")["inval"][dec.NF_INF]


def test_oracle_ssim_spreads_one_nan_over_rows_and_columns():
    """The divergence DESIGN.md states: with a non-finite depth the reference's SSIM (``scipy.ndimage.uniform_filter``, a running
    sum along each line) loses the rest of the line behind the first NaN, and then the columns that cross those lines; a
    direct sum over each 7 x 7 window, which is what ``k_dp_ssim`` does, loses the windows that hold the NaN and nothing else.
    That is why no SSIM case has a non-finite depth."""
    base, _ = dec.build("nf_v2")
    H, W = base["depth"].shape
    bad = ~np.isfinite(base["depth"])
    bad[dec.NF_NAN_BORDER] = bad[dec.NF_NAN_PAIR[1]] = False
    base["depth"][dec.NF_NAN_BORDER] = base["depth"][dec.NF_NAN_PAIR[1]] = 0.2       # leaves one NaN and one +inf
    assert bad.sum() == 2
    with np.errstate(all="ignore"):
        out = dec.run_oracle(base, dec.VARIANTS["v2ssim"])
        gx, gy = dpo.project3d_grid(base["depth"], base["inv_K"], base["K"], base["stereo_T"])
        warp = dpo.grid_sample_bilinear(base["color01"], gx, gy)
    lost = np.isnan(warp).any(0)
    np.testing.assert_array_equal(lost, bad)                                        # the warp is NaN at exactly those two pixels
    # the windows a direct sum loses: every pixel within 3 of a lost one (reflecting borders are out of reach here)
    yy, xx = np.nonzero(lost)
    window = np.zeros((H, W), bool)
    for y, x in zip(yy, xx):
        assert 3 <= y < H - 3 and 3 <= x < W - 3
        window[y - 3:y + 4, x - 3:x + 4] = True
    nan = np.isnan(out["disp_conf"])
    assert window.sum() == 2 * 49 and nan[window].all()
    assert nan.mean() > 0.4 and nan.sum() > 8 * window.sum(), nan.mean()
