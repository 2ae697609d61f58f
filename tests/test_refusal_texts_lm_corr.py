"""The refusal texts of slm_enable_corr, slm_bind_corr_flow, slm_bind_corr_points, slm_corr_get_targets and slm_corr_loss, byte
for byte, after the pattern of test_refusal_texts_render_in_run.py, and the exports, signatures and ABI version of the new
entry points.  What is refused on the arguments alone, and the export checks, run without a GPU; the refusals that need a
solver (slm_create needs a device) are marked gpu."""
import ctypes as C
import os
import re

import pytest

INVALID, UNBOUND, UNSUPPORTED = 1, 4, 5
NEW = ("slm_enable_corr", "slm_bind_corr_flow", "slm_bind_corr_points", "slm_corr_get_targets", "slm_corr_loss")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "super_lm.h")


@pytest.fixture(scope="module")
def lib():
    import os
    from super_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):      # (a tree that was never built; build() of the entry file is the usual way)
        build.build()
    return _lib.load()


def _refused(lib, name, args, code, text):
    rc = getattr(lib, name)(*args)
    got = lib.slm_last_error()
    print(name, rc, got)
    assert rc == code, (name, rc, got)
    assert got == text, (name, got)


def test_null_arguments_are_refused(lib):
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    _refused(lib, "slm_enable_corr", (None, 1, 1.0), INVALID, b"slm_enable_corr: null argument")
    _refused(lib, "slm_bind_corr_flow", (None, 0, one, None), INVALID, b"slm_bind_corr_flow: null argument")
    _refused(lib, "slm_bind_corr_points", (None, 0, one, one, one, None), INVALID, b"slm_bind_corr_points: null argument")
    _refused(lib, "slm_corr_get_targets", (None, 0, one, one, one, None), INVALID, b"slm_corr_get_targets: null argument")
    _refused(lib, "slm_corr_loss", (None, 0, one, None), INVALID, b"slm_corr_loss: null argument")


def _declaration(name):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_exports_signatures_and_abi_version(lib):
    from super_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(raw, name)                                   # the built library exports it
    assert _declaration("slm_enable_corr") == ["slm_solver* s", "int32_t mode", "double weight"]
    assert _declaration("slm_bind_corr_flow") == ["slm_solver* s", "int32_t slot", "const float* flow", "void* stream"]
    assert _declaration("slm_bind_corr_points") == ["slm_solver* s", "int32_t slot", "const double* pts", "const double* nrm",
                                                    "const uint8_t* valid", "void* stream"]
    assert _declaration("slm_corr_get_targets") == ["slm_solver* s", "int32_t slot", "double* pts", "double* nrm", "uint8_t* valid",
                                                    "void* stream"]
    assert _declaration("slm_corr_loss") == ["slm_solver* s", "int32_t slot", "double* out_device", "void* stream"]
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.slm_enable_corr.argtypes == [vp, i32, C.c_double]
    assert lib.slm_bind_corr_flow.argtypes == [vp, i32, vp, vp]
    assert lib.slm_bind_corr_points.argtypes == [vp, i32, vp, vp, vp, vp]
    assert lib.slm_corr_get_targets.argtypes == [vp, i32, vp, vp, vp, vp]
    assert lib.slm_corr_loss.argtypes == [vp, i32, vp, vp]
    for name in NEW:
        assert getattr(lib, name).restype == C.c_int
    assert re.search(r"#define\s+SLM_ABI_VERSION\s+3\b", open(HEADER).read())
    assert _lib.SLM_ABI_VERSION == 3 and lib.slm_abi_version() == 3


def test_every_refusal_text_is_listed_in_the_header():
    text = open(HEADER).read()
    for t in ("slm_enable_corr: null argument", "slm_enable_corr: mode must be 0 (off), 1 (point-point) or 2 (point-plane)",
              "slm_enable_corr: weight must be finite",
              "slm_enable_corr: a slot is already bound; call it after slm_create and before the first bind",
              "slm_enable_corr: needs the pair-record data path (data_path 0 or 2)",
              "slm_enable_corr: needs a nested-dissection solver_path (0, 2, 3 or 4)", "slm_enable_corr: needs the data term (use_data 1)",
              "slm_enable_corr: the solver is sharded (slm_set_shard); the term needs every surfel of the frame on one device",
              "slm_set_shard: the correspondence term is enabled (slm_enable_corr); it needs every surfel of the frame on one device",
              "slm_bind_frame: the correspondence term (slm_enable_corr) needs J < 65536",
              "slm_bind_corr_points: nrm is required in mode 2 (point-plane)", "<fn>: slm_enable_corr first", "<fn>: slm_bind_frame first",
              "slm_corr_get_targets: no correspondences bound to the slot"):
        assert '"' + t + '"' in text, t


def test_python_surface_has_the_keywords():
    import inspect
    from super_amd.LM import LM_Solver
    assert inspect.signature(LM_Solver.__init__).parameters["corr_term"].default is False
    for fn in (LM_Solver.LM, LM_Solver.prepareCostTerm):
        p = inspect.signature(fn).parameters
        assert p["flow"].default is None and p["corr_points"].default is None


@pytest.mark.gpu
def test_refusal_texts_with_a_solver(lib):
    import torch
    from helpers import load_corr_golden
    from super_amd.engine import DeviceFrame, Engine
    dev = torch.device("cuda", 0)
    g, sc = load_corr_golden()
    fr = DeviceFrame.from_scene(sc, dev, state_f64=True)
    flow = torch.from_numpy(sc.flow).to(dev).contiguous()
    pts = torch.zeros((sc.N, 3), dtype=torch.float64, device=dev)
    val = torch.zeros(sc.N, dtype=torch.uint8, device=dev)
    out = torch.zeros(2, dtype=torch.float64, device=dev)
    pre = b"slm_enable_corr: "

    # what the configuration refuses
    for kw, text in ((dict(data_path=1), b"needs the pair-record data path (data_path 0 or 2)"),
                     (dict(solver_path=1), b"needs a nested-dissection solver_path (0, 2, 3 or 4)"),
                     (dict(use_data=False), b"needs the data term (use_data 1)")):
        e = Engine(dev, **kw)
        _refused(lib, "slm_enable_corr", (e.h, 1, 1.0), UNSUPPORTED, pre + text)
        e.close()
    e = Engine(dev, max_frames=2)
    _refused(lib, "slm_enable_corr", (e.h, 3, 1.0), INVALID, pre + b"mode must be 0 (off), 1 (point-point) or 2 (point-plane)")
    _refused(lib, "slm_enable_corr", (e.h, -1, 1.0), INVALID, pre + b"mode must be 0 (off), 1 (point-point) or 2 (point-plane)")
    _refused(lib, "slm_enable_corr", (e.h, 1, float("nan")), INVALID, pre + b"weight must be finite")
    _refused(lib, "slm_enable_corr", (e.h, 1, float("inf")), INVALID, pre + b"weight must be finite")
    # the per-slot entry points before slm_enable_corr
    for name, args in (("slm_bind_corr_flow", (e.h, 0, flow.data_ptr(), None)),
                       ("slm_bind_corr_points", (e.h, 0, pts.data_ptr(), None, val.data_ptr(), None)),
                       ("slm_corr_get_targets", (e.h, 0, None, None, None, None)), ("slm_corr_loss", (e.h, 0, out.data_ptr(), None))):
        _refused(lib, name, args, UNSUPPORTED, name.encode() + b": slm_enable_corr first")
    # sharded, in either order
    assert lib.slm_set_shard(e.h, 0, 1) == 0
    _refused(lib, "slm_enable_corr", (e.h, 1, 1.0), UNSUPPORTED,
             pre + b"the solver is sharded (slm_set_shard); the term needs every surfel of the frame on one device")
    e.close()
    e = Engine(dev, max_frames=2)
    assert lib.slm_enable_corr(e.h, 2, 0.5) == 0, lib.slm_last_error()
    _refused(lib, "slm_set_shard", (e.h, 0, 2), UNSUPPORTED,
             b"slm_set_shard: the correspondence term is enabled (slm_enable_corr); it needs every surfel of the frame on one device")
    # bad slots, null arguments, unbound slots
    for name, args in (("slm_bind_corr_flow", (e.h, 2, flow.data_ptr(), None)),
                       ("slm_bind_corr_points", (e.h, -1, pts.data_ptr(), None, val.data_ptr(), None)),
                       ("slm_corr_get_targets", (e.h, 2, None, None, None, None)), ("slm_corr_loss", (e.h, 2, out.data_ptr(), None))):
        _refused(lib, name, args, INVALID, name.encode() + b": bad slot")
    _refused(lib, "slm_bind_corr_flow", (e.h, 0, None, None), INVALID, b"slm_bind_corr_flow: null argument")
    _refused(lib, "slm_bind_corr_points", (e.h, 0, None, None, val.data_ptr(), None), INVALID, b"slm_bind_corr_points: null argument")
    _refused(lib, "slm_bind_corr_points", (e.h, 0, pts.data_ptr(), None, None, None), INVALID, b"slm_bind_corr_points: null argument")
    _refused(lib, "slm_corr_loss", (e.h, 0, None, None), INVALID, b"slm_corr_loss: null argument")
    for name, args in (("slm_bind_corr_flow", (e.h, 0, flow.data_ptr(), None)),
                       ("slm_bind_corr_points", (e.h, 0, pts.data_ptr(), pts.data_ptr(), val.data_ptr(), None)),
                       ("slm_corr_get_targets", (e.h, 0, None, None, None, None)), ("slm_corr_loss", (e.h, 0, out.data_ptr(), None))):
        _refused(lib, name, args, UNBOUND, name.encode() + b": slm_bind_frame first")
    # at the bind: J >= 65536 (refused on the sizes, before anything is read)
    cs = fr.c_struct()
    cs.J = 65536
    _refused(lib, "slm_bind_frame", (e.h, 0, C.byref(cs), None), UNSUPPORTED,
             b"slm_bind_frame: the correspondence term (slm_enable_corr) needs J < 65536")
    e.bind(0, fr)
    _refused(lib, "slm_corr_get_targets", (e.h, 0, None, None, None, None), UNBOUND,
             b"slm_corr_get_targets: no correspondences bound to the slot")
    _refused(lib, "slm_bind_corr_points", (e.h, 0, pts.data_ptr(), None, val.data_ptr(), None), INVALID,
             b"slm_bind_corr_points: nrm is required in mode 2 (point-plane)")
    # a slot is bound: the option can no longer change
    _refused(lib, "slm_enable_corr", (e.h, 1, 1.0), INVALID,
             pre + b"a slot is already bound; call it after slm_create and before the first bind")
    _refused(lib, "slm_enable_corr", (e.h, 0, 0.0), INVALID,
             pre + b"a slot is already bound; call it after slm_create and before the first bind")
    # and the calls that are not refused
    assert lib.slm_bind_corr_flow(e.h, 0, flow.data_ptr(), None) == 0, lib.slm_last_error()
    assert lib.slm_corr_get_targets(e.h, 0, pts.data_ptr(), None, val.data_ptr(), None) == 0, lib.slm_last_error()
    assert lib.slm_corr_loss(e.h, 0, out.data_ptr(), None) == 0, lib.slm_last_error()
    torch.cuda.synchronize()
    assert int(val.sum()) > 1000 and float(out[0]) > 0 and int(out[1]) == int(val.sum())
    e.bind(0, fr)                                            # slm_bind_frame clears the slot's correspondences
    _refused(lib, "slm_corr_get_targets", (e.h, 0, None, None, None, None), UNBOUND,
             b"slm_corr_get_targets: no correspondences bound to the slot")
    e.close()


@pytest.mark.gpu
def test_python_refusals():
    from helpers import GF_CORR_VARIANTS, load_corr_golden, ref_opt, torch_frame
    from oracle import lm_oracle as orc
    from super_amd.LM import LM_Solver
    opt = ref_opt(orc.default_opt())
    with pytest.raises(ValueError, match="needs opt.sf_corr"):
        LM_Solver(opt, corr_term=True)
    opt.sf_corr, opt.sf_corr_weight, opt.sf_corr_loss_type = True, 0.05, "point-point"
    with pytest.raises(NotImplementedError, match="corr_term with shard_surfels"):
        LM_Solver(opt, corr_term=True, rank=0, world=2, all_reduce=lambda t: None, broadcast=lambda t: None)
    opt.sf_corr_loss_type = "plane-plane"
    with pytest.raises(ValueError, match="sf_corr_loss_type"):
        LM_Solver(opt, corr_term=True)
    opt.sf_corr_loss_type = "point-point"
    g, sc = load_corr_golden()
    sf, inputs, new_data = torch_frame(sc)
    with pytest.raises(ValueError, match="needs flow="):
        LM_Solver(opt, corr_term=True).LM(sf, inputs, new_data)
    with pytest.raises(ValueError, match="need LM_Solver\\(opt, corr_term=True\\)"):
        import torch
        LM_Solver(opt).LM(sf, inputs, new_data, flow=torch.from_numpy(sc.flow).cuda())
