"""The exports, signatures and refusals of the rigid stage's opt-in terms (slm_rigid_set_terms, _set_corr, _set_semantic,
_corr_targets, _get_terms) that need no device, the header's list of every refusal text and the refusals of the Python
mirror, after the pattern of test_refusal_texts_rigid.py.  The refusals that need a context are in
tests/test_gpu_rigid_terms.py."""
import ctypes as C
import os
import re

import pytest

INVALID = 1
NEW = ("slm_rigid_set_terms", "slm_rigid_set_corr", "slm_rigid_set_semantic", "slm_rigid_corr_targets", "slm_rigid_get_terms")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "super_lm.h")
SOURCE = os.path.join(ROOT, "python-super_amd", "csrc", "slm_rigid.hip")

LITERAL = ("slm_rigid_set_terms: null argument", "slm_rigid_set_corr: null argument", "slm_rigid_set_semantic: null argument",
           "slm_rigid_corr_targets: null argument", "slm_rigid_get_terms: null argument",
           "slm_rigid_set_corr: bad slot", "slm_rigid_set_semantic: bad slot", "slm_rigid_get_terms: bad slot",
           "slm_rigid_set_terms: corr_mode must be 0 (none), 1 (point-point) or 2 (point-plane)",
           "slm_rigid_set_terms: corr_weight must be finite",
           "slm_rigid_set_terms: seg_mode must be 0 (none), 1 (hard) or 2 (soft)",
           "slm_rigid_set_terms: pp_max must be finite and >= 0",
           "slm_rigid_set_corr: the correspondence term is off; call slm_rigid_set_terms with corr_mode 1 or 2 first",
           "slm_rigid_set_corr: corr_mode 2 (point-plane) needs nrm",
           "slm_rigid_set_semantic: the semantic weight is off; call slm_rigid_set_terms with seg_mode 1 or 2 first",
           "slm_rigid_set_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)",
           "slm_rigid_corr_targets: T must be > 0")


@pytest.fixture(scope="module")
def lib():
    from super_amd import build, _lib
    if not os.path.exists(_lib.LIB_PATH):      # (a tree that was never built; build() of the entry file is the usual way)
        build.build()
    return _lib.load()


def _declaration(name):
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", text)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_exports_and_signatures(lib):
    from super_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(raw, name)                                   # the built library exports it
        assert getattr(lib, name).restype == C.c_int
    assert _declaration("slm_rigid_set_terms") == ["slm_rigid* r", "int32_t corr_mode", "double corr_weight", "int32_t seg_mode",
                                                   "double pp_max"]
    assert _declaration("slm_rigid_set_corr") == ["slm_rigid* r", "int32_t slot", "const double* pts", "const double* nrm",
                                                  "const uint8_t* valid"]
    assert _declaration("slm_rigid_set_semantic") == ["slm_rigid* r", "int32_t slot", "int32_t num_classes",
                                                      "const int32_t* sf_seg", "const float* sf_seg_conf",
                                                      "const float* tgt_seg_conf"]
    assert _declaration("slm_rigid_corr_targets") == ["const slm_frame* frame", "const float* flow", "double* pts", "double* nrm",
                                                      "uint8_t* valid", "void* stream"]
    assert _declaration("slm_rigid_get_terms") == ["slm_rigid* r", "int32_t slot", "double* out4_device", "void* stream"]
    vp, i32, dbl = C.c_void_p, C.c_int32, C.c_double
    assert lib.slm_rigid_set_terms.argtypes == [vp, i32, dbl, i32, dbl]
    assert lib.slm_rigid_set_corr.argtypes == [vp, i32, vp, vp, vp]
    assert lib.slm_rigid_set_semantic.argtypes == [vp, i32, i32, vp, vp, vp]
    assert lib.slm_rigid_corr_targets.argtypes == [C.POINTER(_lib.SlmFrame), vp, vp, vp, vp, vp]
    assert lib.slm_rigid_get_terms.argtypes == [vp, i32, vp, vp]
    # additions only: the version and the stage's one struct stay
    assert re.search(r"#define\s+SLM_ABI_VERSION\s+3\b", open(HEADER).read())
    assert _lib.SLM_ABI_VERSION == 3 and lib.slm_abi_version() == 3
    assert C.sizeof(_lib.SlmRigidConfig) == 48 and lib.slm_rigid_abi_check(48) == 0


def test_null_arguments_and_ranges_are_refused_without_a_device(lib):
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    from super_amd._lib import SlmFrame
    fr = SlmFrame()
    calls = (("slm_rigid_set_terms", (None, 0, 0.0, 0, 0.0)),
             ("slm_rigid_set_corr", (None, 0, one, one, one)),
             ("slm_rigid_set_semantic", (None, 0, 3, one, one, one)),
             ("slm_rigid_corr_targets", (None, one, one, one, one, None)),
             ("slm_rigid_corr_targets", (C.byref(fr), None, one, one, one, None)),
             ("slm_rigid_corr_targets", (C.byref(fr), one, None, one, one, None)),
             ("slm_rigid_corr_targets", (C.byref(fr), one, one, None, one, None)),
             ("slm_rigid_corr_targets", (C.byref(fr), one, one, one, None, None)),
             ("slm_rigid_get_terms", (None, 0, one, None)), ("slm_rigid_get_terms", (one, 0, None, None)))
    for name, args in calls:
        assert getattr(lib, name)(*args) == INVALID, (name, args)
        assert lib.slm_last_error() == name.encode() + b": null argument", (name, args)
    # the values are checked before the context is touched
    for args, text in (((one, 3, 1.0, 0, 0.0), b"corr_mode must be 0 (none), 1 (point-point) or 2 (point-plane)"),
                       ((one, -1, 1.0, 0, 0.0), b"corr_mode must be 0 (none), 1 (point-point) or 2 (point-plane)"),
                       ((one, 1, float("nan"), 0, 0.0), b"corr_weight must be finite"),
                       ((one, 1, float("inf"), 0, 0.0), b"corr_weight must be finite"),
                       ((one, 1, 1.0, 3, 0.0), b"seg_mode must be 0 (none), 1 (hard) or 2 (soft)"),
                       ((one, 1, 1.0, -1, 0.0), b"seg_mode must be 0 (none), 1 (hard) or 2 (soft)"),
                       ((one, 1, 1.0, 0, -1e-9), b"pp_max must be finite and >= 0"),
                       ((one, 1, 1.0, 0, float("nan")), b"pp_max must be finite and >= 0"),
                       ((one, 1, 1.0, 0, float("inf")), b"pp_max must be finite and >= 0")):
        assert lib.slm_rigid_set_terms(*args) == INVALID, args
        assert lib.slm_last_error() == b"slm_rigid_set_terms: " + text, args
    # the frame of slm_rigid_corr_targets is checked like the run's
    bad = SlmFrame()
    bad.H, bad.W, bad.N = 1, 80, 4
    assert lib.slm_rigid_corr_targets(C.byref(bad), one, one, one, one, None) == INVALID
    assert lib.slm_last_error() == b"slm_rigid_corr_targets: H and W must be >= 2"
    bad.H = 60
    assert lib.slm_rigid_corr_targets(C.byref(bad), one, one, one, one, None) == INVALID
    assert lib.slm_last_error() == b"slm_rigid_corr_targets: N > 0 needs sf_points"
    bad.sf_points = 8
    assert lib.slm_rigid_corr_targets(C.byref(bad), one, one, one, one, None) == INVALID
    assert lib.slm_last_error() == b"slm_rigid_corr_targets: T must be > 0"
    bad.N = 0
    assert lib.slm_rigid_corr_targets(C.byref(bad), one, one, one, one, None) == 0      # nothing to do: no launch


def test_every_refusal_text_is_listed_in_the_header_and_raised_by_the_library():
    header = open(HEADER).read()
    source = re.sub(r'"\s*\n\s*"', "", open(SOURCE).read())   # adjacent string literals are one text
    for t in LITERAL:
        assert '"' + t + '"' in header or '"<fn>' + t[t.index(":"):] + '"' in header, t
        assert '"' + t + '"' in source, t
    assert '"<fn>: slot <k> has no semantic inputs; call slm_rigid_set_semantic"' in header
    assert '" has no semantic inputs; call slm_rigid_set_semantic"' in source
    for fn in ("slm_rigid_run", "slm_rigid_assemble"):
        assert 'check_semantic("' + fn + '"' in source
    assert 'check_frame("slm_rigid_corr_targets"' in source


def test_python_surface_and_its_refusals():
    import inspect
    from super_amd import rigid
    from super_amd.LM import LM_Solver
    from oracle.lm_oracle import default_opt
    sig = inspect.signature(rigid.RigidAlign.__init__).parameters
    assert sig["corr_term"].default is False and sig["weighted_data"].default is False and sig["max_frames"].default == 1
    assert inspect.signature(LM_Solver.__init__).parameters["rigid_terms"].default is False
    for name, kws in (("align", ("flow", "corr_points")), ("assemble", ("flow", "corr_points")), ("corr_targets", ("flow",))):
        for kw in kws:
            assert kw in inspect.signature(getattr(rigid.RigidAlign, name)).parameters, (name, kw)
    # refused before anything touches the device, with LM_Solver's rules
    with pytest.raises(ValueError, match=r"RigidAlign\(corr_term=True\) needs opt.sf_corr"):
        rigid.RigidAlign(default_opt(), corr_term=True)
    with pytest.raises(ValueError, match="sf_corr_loss_type 'plane'"):
        rigid.RigidAlign(default_opt(sf_corr=True, sf_corr_loss_type="plane"), corr_term=True)
    with pytest.raises(ValueError, match=r"LM_Solver\(corr_term=True\) needs opt.sf_corr"):
        LM_Solver(default_opt(), corr_term=True)
    with pytest.raises(ValueError, match=r"rigid_terms=True\) needs global_rigid=True"):
        LM_Solver(default_opt(sf_corr=True), corr_term=True, rigid_terms=True)
    with pytest.raises(ValueError, match=r"rigid_terms=True\) needs corr_term=True or weighted_data=True"):
        LM_Solver(default_opt(), global_rigid=True, rigid_terms=True)
    with pytest.raises(ValueError, match=r"rigid_terms=True\) needs corr_term=True or weighted_data=True"):
        LM_Solver(default_opt(), global_rigid=True, rigid_terms=True, weighted_data=True)   # no weight turned on in opt
    with pytest.raises(ValueError, match="give flow or corr_points, not both"):
        rigid.RigidAlign._corr_arg(object(), object())
