"""Both K = 4 preparations (the binned kernels and the rocPRIM pipeline of python-super_amd/csrc/slm_prep.hip) against the
independent NumPy construction of tests/prep_plan_model.py, on the frames of tests/prep_plan_cases.py that aim at the branches
``synth.make_scene`` frames never reach: all thirteen arrays of ``slm_debug_read_plan`` and the sizes of ``plan_info``, EXACTLY,
for float32 and float64 state, after a first and after a second (hinted) bind; which preparation ran and the largest bin it
saw; the merged form on and off at SLM_LB_MAX records; the hinted bound at its edge; a plan that shrinks; refused rows; and the
numbers that flow through the plan -- ``slm_assemble`` on data_path 0, 1 and 2 against ``oracle.lm_oracle.normal_equations``
at a perturbed beta, also for the same frames widened / narrowed to K = 1, 6, 8 (the pair-record form).

``SLM_PREP_LEGACY`` is read once per process: one child process per setting runs ALL cases, writes the raw arrays to an .npz
and prints one JSON line; the tests below share the two results.  Needs an MI355X (-m gpu).  Run with -s for one MEASURE line
per case; the values of one run are in RECORD at the end of the file."""
import functools
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INFO_KEYS = ("tuples", "positions", "runs", "pairs", "merged_records", "preparation", "largest_bin")
DATA_PATHS = (0, 1, 2)
DENSE_J = 128                     # above it only jtl is compared: a dense JtJ at J = 2 050 is 1.6 GB
BINNED, ROCPRIM = 1, 2            # plan_info()["preparation"]
BAD_KNN = ("status 1: slm_bind_frame: a KNN index (sf_knn_idx or ed_knn_idx) lies outside [0, J) or a surfel's row of sf_knn_idx "
           "repeats an id")       # SLM_ERR_INVALID and the text of include/super_lm.h's slm_bind_frame


def _wide(name, K):
    return f"{name}@K{K}"


# ====================================================================================================== the child process
def _child(refs_path, out_path):
    import ctypes as C
    import torch
    for p in (ROOT, os.path.join(ROOT, "python-super_amd"), os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import prep_plan_cases as ppc
    from super_amd import _lib
    from super_amd.engine import DeviceFrame, Engine
    dev = torch.device("cuda", 0)
    refs = np.load(refs_path)
    arrays, report = {}, {}

    def read_plan(eng):
        out = []
        for what in range(13):
            n = C.c_int64(0)
            _lib.check(eng.lib.slm_debug_read_plan(eng.h, 0, what, None, 0, C.byref(n), eng.stream), "size")
            buf = np.zeros(max(n.value, 1), np.uint8)
            _lib.check(eng.lib.slm_debug_read_plan(eng.h, 0, what, buf.ctypes.data_as(C.c_void_p), n.value, C.byref(n), eng.stream), "read")
            out.append(buf[:n.value].copy())
        return out

    def bind(eng, sc, f64, key, same_as=None):
        """bind, then the slot's sizes and arrays under `key`; an array equal to `same_as`'s, byte for byte, is only named"""
        eng.bind(0, DeviceFrame.from_scene(sc, dev, state_f64=f64))
        info = eng.plan_info(0)
        report[key] = {k: info[k] for k in INFO_KEYS}
        got = read_plan(eng)
        report[key]["same_as"], report[key]["same"] = same_as, []
        for what, a in enumerate(got):
            if same_as is not None and np.array_equal(a, arrays[f"{same_as}|{what}"]):
                report[key]["same"].append(what)
            else:
                arrays[f"{key}|{what}"] = a
        return got

    def assemble(sc, dp, beta, dense):
        eng = Engine(dev, data_path=dp, num_iterations=1)
        try:
            eng.bind(0, DeviceFrame.from_scene(sc, dev, state_f64=True))
            merged = eng.plan_info(0)["merged_records"]
            bt = torch.from_numpy(np.ascontiguousarray(beta)).to(dev)
            _lib.check(eng.lib.slm_set_beta(eng.h, 0, bt.data_ptr(), eng.stream), "slm_set_beta")
            P = 7 * sc.J
            jtl = torch.zeros(P, dtype=torch.float64, device=dev)
            jtj = torch.zeros((P, P), dtype=torch.float64, device=dev) if dense else None
            _lib.check(eng.lib.slm_assemble(eng.h, 0, jtj.data_ptr() if dense else None, jtl.data_ptr(), eng.stream), "slm_assemble")
            torch.cuda.synchronize()
            return (jtj.cpu().numpy() if dense else None), jtl.cpu().numpy(), merged
        finally:
            eng.close()

    def numbers(tag, sc):
        """slm_assemble on the three data paths at the perturbed beta: largest errors against the oracle and between the paths"""
        dense = sc.J <= DENSE_J
        outs = [assemble(sc, dp, refs[f"beta|{sc.J}"], dense) for dp in DATA_PATHS]
        amax = lambda a: float(np.abs(a).max()) if a.size else 0.0
        r = dict(dense=dense, merged_records=[o[2] for o in outs], jtl_err=[amax(o[1] - refs[f"{tag}|jtl"]) for o in outs],
                 jtl_max=[amax(o[1]) for o in outs], jtl_between=[amax(outs[0][1] - o[1]) for o in outs],
                 finite=bool(all(np.isfinite(o[1]).all() and (o[0] is None or np.isfinite(o[0]).all()) for o in outs)))
        if dense:
            r.update(jtj_err=[amax(o[0] - refs[f"{tag}|jtj"]) for o in outs], jtj_max=[amax(o[0]) for o in outs],
                     jtj_between=[amax(outs[0][0] - o[0]) for o in outs], jtj_asym=[amax(o[0] - o[0].T) for o in outs])
        report[f"num/{tag}"] = r

    tiny = ppc.tiny()
    for name in ppc.SINGLE:
        sc = ppc.single(name)
        for f64 in (False, True):
            prec = "f64" if f64 else "f32"
            eng = Engine(dev, data_path=0, num_iterations=1)
            bind(eng, sc, f64, f"{name}/{prec}/1")
            bind(eng, sc, f64, f"{name}/{prec}/2", same_as=f"{name}/{prec}/1")       # the second bind takes the hinted path
            if name in ppc.OVER_CAP:                                                   # the slot stays on the rocPRIM pipeline
                bind(eng, tiny, f64, f"{name}/{prec}/then_tiny")
            eng.close()
        numbers(name, sc)
    for name in ppc.WIDENED:
        for K in ppc.WIDEN_K:
            numbers(_wide(name, K), ppc.widened(name, K))
    for name in ppc.PAIRS:
        a, b = ppc.pair(name)
        for f64 in (False, True):
            prec = "f64" if f64 else "f32"
            fresh = Engine(dev, data_path=0, num_iterations=1)
            bind(fresh, b, f64, f"{name}/{prec}/fresh")
            fresh.close()
            eng = Engine(dev, data_path=0, num_iterations=1)
            bind(eng, a, f64, f"{name}/{prec}/A")
            bind(eng, b, f64, f"{name}/{prec}/B", same_as=f"{name}/{prec}/fresh")
            eng.close()
    for kind in ppc.REFUSED:
        eng = Engine(dev, data_path=0, num_iterations=1)
        try:
            eng.bind(0, DeviceFrame.from_scene(ppc.bad_row(kind), dev))
            report[f"{kind}/error"] = None
        except _lib.SuperLMError as e:
            report[f"{kind}/error"] = str(e)
        bind(eng, tiny, False, f"{kind}/then_tiny")
        eng.close()
    np.savez(out_path, **arrays)
    print("RESULT " + json.dumps(report))


if __name__ == "__main__":
    _child(sys.argv[1], sys.argv[2])
    sys.exit(0)


# ============================================================================================================== the tests
import pytest   # noqa: E402

import prep_plan_cases as ppc   # noqa: E402
import prep_plan_model as ppm   # noqa: E402
from oracle import lm_oracle as orc   # noqa: E402

pytestmark = pytest.mark.gpu


def _beta(J):
    """the perturbed beta of test_c2_assembly_paths_agree_and_match_oracle_terms (tests/test_gpu_edge_and_fullsize.py)"""
    rng = np.random.default_rng(9)
    return np.tile([1.0, 0, 0, 0, 0, 0, 0], (J, 1)) + np.concatenate([rng.normal(0, 0.01, (J, 4)), rng.normal(0, 0.002, (J, 3))], axis=1)


def _numbers_cases():
    return [(n, ppc.single(n)) for n in ppc.SINGLE] + [(_wide(n, K), ppc.widened(n, K)) for n in ppc.WIDENED for K in ppc.WIDEN_K]


@pytest.fixture(scope="module")
def oracle_refs(tmp_path_factory):
    """normal equations of the NumPy oracle for every frame whose numbers are checked, computed once for both children"""
    refs, matched = {}, {}
    for tag, sc in _numbers_cases():
        refs.setdefault(f"beta|{sc.J}", _beta(sc.J))
        dense = sc.J <= DENSE_J
        JtJ, jtl, M = orc.normal_equations(orc.Frame.from_scene(sc), refs[f"beta|{sc.J}"], orc.default_opt(), dense=dense)
        refs[f"{tag}|jtl"] = jtl
        if dense:
            refs[f"{tag}|jtj"] = JtJ
        matched[tag] = M
    path = str(tmp_path_factory.mktemp("prep_plan") / "refs.npz")
    np.savez(path, **refs)
    return path, refs, matched


def _run(legacy, refs_path, out_path):
    env = dict(os.environ)
    env.pop("SLM_PREP_LEGACY", None)
    if legacy:
        env["SLM_PREP_LEGACY"] = "1"
    p = subprocess.run([sys.executable, os.path.abspath(__file__), refs_path, out_path], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):]), np.load(out_path)


@pytest.fixture(scope="module")
def children(oracle_refs, tmp_path_factory):
    d = tmp_path_factory.mktemp("prep_plan_out")
    return {"binned": _run(False, oracle_refs[0], str(d / "binned.npz")), "rocprim": _run(True, oracle_refs[0], str(d / "rocprim.npz"))}


CHILDREN = ("binned", "rocprim")


@functools.lru_cache(maxsize=None)
def _model(name, f64):
    """the NumPy plan of a frame; name: a single case, `tiny`, or `pair/A` / `pair/B`"""
    if name == "tiny":
        sc = ppc.tiny()
    elif "/" in name:
        sc = ppc.pair(name.split("/")[0])["AB".index(name.split("/")[1])]
    else:
        sc = ppc.single(name)
    return ppm.build_plan(sc.sf_knn_idx, sc.sf_knn_w, sc.sf_points, sc.J, np.float64 if f64 else np.float32), ppm.plan_stats(sc.sf_knn_idx, sc.J)


def _arrays(child, key):
    report, npz = child
    rep = report[key]
    return [npz[f"{rep['same_as']}|{w}"] if w in rep["same"] else npz[f"{key}|{w}"] for w in range(13)]


def _assert_plan(child, key, model_name, f64):
    """the slot's thirteen arrays and sizes under `key` equal the model's, exactly"""
    m, _ = _model(model_name, f64)
    info = child[0][key]
    want = dict(tuples=m.tuples, positions=m.positions, runs=m.runs, pairs=m.pairs, merged_records=m.records if m.v2 else 0)
    assert {k: info[k] for k in want} == want, key
    for what, got in enumerate(_arrays(child, key)):
        tag = f"{key}: array {what} ({ppm.ARRAYS[what]})"
        if what in ppm.V2_ARRAYS and not m.v2:
            assert got.size == 0, tag                        # the merged form is off: nothing to read
            continue
        ref = m.arrays[what]
        assert got.size == ref.nbytes, (tag, "bytes", got.size, ref.nbytes)
        np.testing.assert_array_equal(got.view(ref.dtype), ref.reshape(-1), err_msg=tag)


def _expected_preparation(which, name):
    """(preparation, largest bin) plan_info must report for the first bind of a single case"""
    if which == "rocprim" or name in ppc.OVER_CAP:
        return ROCPRIM, 0
    return BINNED, _model(name, False)[1].max_bin


@pytest.mark.parametrize("which", CHILDREN)
def test_plan_equals_the_numpy_construction_exactly(children, which):
    child = children[which]
    for name in ppc.SINGLE:
        for f64 in (False, True):
            prec = "f64" if f64 else "f32"
            _assert_plan(child, f"{name}/{prec}/1", name, f64)
            _assert_plan(child, f"{name}/{prec}/2", name, f64)          # ... and again after the hinted build


@pytest.mark.parametrize("which", CHILDREN)
def test_which_preparation_ran_and_its_largest_bin(children, which):
    report = children[which][0]
    for name in ppc.SINGLE:
        st = _model(name, False)[1]
        assert (st.max_bin > ppm.BIN_CAP) == (name in ppc.OVER_CAP)
        for prec in ("f32", "f64"):
            for n in "12":
                got = report[f"{name}/{prec}/{n}"]
                assert (got["preparation"], got["largest_bin"]) == _expected_preparation(which, name), (name, prec, n, got)
            if name in ppc.OVER_CAP:                                     # sticky: the small frame that follows on the slot
                got = report[f"{name}/{prec}/then_tiny"]
                assert (got["preparation"], got["largest_bin"]) == (ROCPRIM, 0), (name, prec, got)
                _assert_plan(children[which], f"{name}/{prec}/then_tiny", "tiny", prec == "f64")
    for name in ("binA_1024", "binB_1024"):                              # the cap itself is still sorted in LDS
        assert _expected_preparation("binned", name) == (BINNED, ppm.BIN_CAP)


@pytest.mark.parametrize("which", CHILDREN)
def test_merged_form_switches_off_above_lb_max_records(children, which):
    child = children[which]
    for name in ("wg_96",) + ppc.NOT_MERGED:
        for prec in ("f32", "f64"):
            m, st = _model(name, prec == "f64")
            assert m.v2 == (name == "wg_96") and m.max_records_per_wg == st.wg_records.max()
            info, got = child[0][f"{name}/{prec}/1"], _arrays(child, f"{name}/{prec}/1")
            if name == "wg_96":
                assert info["merged_records"] == m.records > 0 and all(got[w].size > 0 for w in ppm.V2_ARRAYS)
            else:
                assert info["merged_records"] == 0 and all(got[w].size == 0 for w in ppm.V2_ARRAYS)
                for w in (0, 1, 2, 3, 4, 5, 6, 12):                      # (also part of the exact comparison above)
                    np.testing.assert_array_equal(got[w].view(m.arrays[w].dtype), m.arrays[w].reshape(-1))


@pytest.mark.parametrize("which", CHILDREN)
def test_hinted_bound_at_its_edge_and_a_plan_that_shrinks(children, which):
    child = children[which]
    for name in ppc.PAIRS:
        for f64 in (False, True):
            prec = "f64" if f64 else "f32"
            _assert_plan(child, f"{name}/{prec}/A", f"{name}/A", f64)
            _assert_plan(child, f"{name}/{prec}/fresh", f"{name}/B", f64)
            _assert_plan(child, f"{name}/{prec}/B", f"{name}/B", f64)    # the plan of a fresh slot, with its lengths
            rep = child[0][f"{name}/{prec}/B"]
            assert rep["same"] == list(range(13)), (name, prec, rep["same"])
            fresh = child[0][f"{name}/{prec}/fresh"]
            assert {k: rep[k] for k in INFO_KEYS} == {k: fresh[k] for k in INFO_KEYS}
    t0 = child[0]["hint_hold/f32/A"]["tuples"]
    assert child[0]["hint_hold/f32/B"]["tuples"] == t0 + t0 // 8 + 64 == child[0]["hint_miss/f32/B"]["tuples"] - 1


@pytest.mark.parametrize("which", CHILDREN)
def test_bad_rows_are_refused_and_the_slot_binds_again(children, which):
    child = children[which]
    for kind in ppc.REFUSED:
        err = child[0][f"{kind}/error"]
        assert err is not None and BAD_KNN in err, (kind, err)
        _assert_plan(child, f"{kind}/then_tiny", "tiny", False)
        got = child[0][f"{kind}/then_tiny"]
        assert got["preparation"] == (BINNED if which == "binned" else ROCPRIM)


def _check_numbers(tag, r, J, matched, stats=None, label=""):
    """the suite's bounds: 1e-7 max(1, |ref|max) against the oracle (test_gpu_parity.py), 1e-9 max(1, |.|max) between the data
    paths (test_gpu_edge_and_fullsize.py)"""
    kinds = ("jtj", "jtl") if r["dense"] else ("jtl",)
    print(f"MEASURE {label}{tag} J={J} M={matched} merged={r['merged_records']} " + " ".join(
        f"{k}: err={max(r[k + '_err']):.2e} ref_max={max(r[k + '_max']):.2e} between={max(r[k + '_between']):.2e}" for k in kinds)
        + (f" prep={stats[0]} bin={stats[1]} wg_max={stats[2]}" if stats else ""))
    assert r["finite"]
    for k in kinds:
        for dp in DATA_PATHS:
            ref_max = r[k + "_ref_max"]
            assert r[k + "_err"][dp] <= 1e-7 * max(1.0, ref_max), (tag, k, "data_path", dp, r[k + "_err"][dp], ref_max)
            assert r[k + "_between"][dp] <= 1e-9 * max(1.0, r[k + "_max"][dp]), (tag, k, "data_path 0 against", dp, r[k + "_between"][dp])
    if r["dense"]:
        assert max(r["jtj_asym"]) <= 1e-9 * max(1.0, max(r["jtj_max"])), (tag, r["jtj_asym"])


@pytest.mark.parametrize("which", CHILDREN)
def test_numbers_through_the_plan_match_the_oracle(children, oracle_refs, which):
    report = children[which][0]
    _, refs, matched = oracle_refs
    for name in ppc.SINGLE:
        sc = ppc.single(name)
        r = dict(report[f"num/{name}"])
        r["jtl_ref_max"] = float(np.abs(refs[f"{name}|jtl"]).max())
        if r["dense"]:
            r["jtj_ref_max"] = float(np.abs(refs[f"{name}|jtj"]).max())
        assert r["dense"] == (sc.J <= DENSE_J) and (matched[name] > 0 or sc.N < 63)
        m, st = _model(name, True)
        info = report[f"{name}/f64/1"]
        assert r["merged_records"] == [m.records if m.v2 else 0, 0, 0]          # the merged form only on data_path 0
        _check_numbers(name, r, sc.J, matched[name], (info["preparation"], info["largest_bin"], m.max_records_per_wg), f"{which} ")
    for name in ppc.NOT_MERGED:       # data_path 0 == data_path 2 on JtJ although the merged form is off there
        r = report[f"num/{name}"]
        assert r["merged_records"][0] == 0 and r["jtj_between"][2] <= 1e-9 * max(1.0, r["jtj_max"][2])


@pytest.mark.parametrize("which", CHILDREN)
def test_numbers_of_the_pair_record_form_match_the_oracle(children, oracle_refs, which):
    report = children[which][0]
    _, refs, matched = oracle_refs
    for name in ppc.WIDENED:
        for K in ppc.WIDEN_K:
            tag = _wide(name, K)
            r = dict(report[f"num/{tag}"])
            r["jtl_ref_max"], r["jtj_ref_max"] = float(np.abs(refs[f"{tag}|jtl"]).max()), float(np.abs(refs[f"{tag}|jtj"]).max())
            assert r["dense"] and matched[tag] > 0 and r["merged_records"] == [0, 0, 0]
            _check_numbers(tag, r, ppc.single(name).J, matched[tag], label=f"{which} ")


# ------------------------------------------------------------------------------------------------------------------- RECORD
# One run of this file on an MI355X (14 passed in 8 s, both children included).  Every array of every case equalled the NumPy
# construction in both children, for both state dtypes, after the first and after the hinted bind: the cases found no defect in
# slm_prep.hip, in the bind's use of the sizes or in slm_debug_read_plan's lengths.  Per case: surfels matched by the data term
# (M), the preparation and the largest bin that plan_info reports in the default child (under SLM_PREP_LEGACY=1: rocPRIM and 0
# for every case), the records of the fullest workgroup (the model's; 0 merged records = the per-run form), and the largest
# error of slm_assemble over the data paths 0, 1, 2 and both children -- against the oracle (bound 1e-7 max(1, |ref|max), |ref|max
# = 6.0e2 .. 1.2e3 for JtJ and 4.6 .. 7.2 for jtl) and between data path 0 and the others (bound 1e-9 max(1, |.|max)).  The
# error against the oracle is the same in every frame of one J whatever its surfels and their order: it belongs to the terms
# that do not depend on the surfels (the oracle evaluates the Rot term in float32, like the reference); what the plan can add
# to it is of the size of the between-paths column.  name@K: the frame at K neighbours (pair-record form; no K = 4 plan).
# case                    J     M   preparation  largest  records of the  merged    JtJ: against  between     jtl: against  between
#                                                    bin      fullest wg  records     the oracle  the paths     the oracle  the paths
# n1_j4                   4     1   binned           4        10             10        9.4e-08    0.0e+00       1.5e-09    0.0e+00
# n3_j4                   4     3   binned           4        10             10        9.4e-08    5.6e-17       1.5e-09    0.0e+00
# n63_j4                  4    63   binned          63        10             10        9.4e-08    2.8e-14       1.5e-09    0.0e+00
# n64_j4                  4    64   binned          64        10             10        9.4e-08    1.3e-15       1.5e-09    8.9e-16
# n65_j4                  4    65   binned          65        10             10        9.4e-08    1.8e-15       1.5e-09    1.1e-16
# n1_j48                 48     1   binned           4        10             10        2.3e-07    7.1e-15       3.0e-09    8.9e-16
# n3_j48                 48     3   binned           4        10             10        2.3e-07    7.1e-15       3.0e-09    8.9e-16
# n63_j48                48    63   binned          63        10             10        2.3e-07    7.1e-15       3.0e-09    8.9e-16
# n64_j48                48    64   binned          64        10             10        2.3e-07    7.1e-15       3.0e-09    8.9e-16
# n65_j48                48    65   binned          65        10             10        2.3e-07    7.1e-15       3.0e-09    8.9e-16
# pad_edges              48   507   binned         300        90            110        2.3e-07    1.2e-14       3.0e-09    8.9e-16
# shuffled_surfels       48  3000   binned         181        71            686        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# binA_1023              48  2523   binned        1023        58            393        2.3e-07    1.1e-13       3.0e-09    1.1e-15
# binA_1024              48  2524   binned        1024        55            365        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# binA_1025              48  2525   rocPRIM          0        54            374        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# binB_1024              48   436   binned        1024        55            258        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# binB_1028              48   437   rocPRIM          0        55            264        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# j1025                1025  3000   binned          80        80            802              -          -       6.1e-09    1.8e-15
# j2050                2050  3000   binned          80        77            813              -          -       6.4e-09    1.8e-15
# wg_96                  48   496   binned         100        96            131        2.3e-07    2.8e-14       3.0e-09    8.9e-16
# wg_97                  48   496   binned         100        97              0        2.3e-07    1.1e-14       3.0e-09    8.9e-16
# wg_dense               48    64   binned          39       366              0        2.3e-07    7.1e-15       3.0e-09    8.9e-16
# shuffled_surfels@K1    48  3000   -                -         -              0        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# shuffled_surfels@K6    48  3000   -                -         -              0        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# shuffled_surfels@K8    48  3000   -                -         -              0        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# binA_1025@K1           48  2520   -                -         -              0        2.3e-07    1.3e-13       3.0e-09    1.3e-15
# binA_1025@K6           48  2525   -                -         -              0        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# binA_1025@K8           48  2525   -                -         -              0        2.3e-07    1.1e-13       3.0e-09    8.9e-16
# wg_dense@K1            48    63   -                -         -              0        2.3e-07    7.1e-15       3.0e-09    8.9e-16
# wg_dense@K6            48    64   -                -         -              0        2.3e-07    7.1e-15       3.0e-09    4.4e-16
# wg_dense@K8            48    64   -                -         -              0        2.3e-07    7.1e-15       3.0e-09    8.9e-16
