"""The exports, signatures and ABI version of slm_enable_data_weights, slm_bind_data_semantic and slm_data_weights, the
refusals that need no solver, and the header's list of every refusal text, after the pattern of
test_refusal_texts_lm_corr.py.  The refusals that need a solver (slm_create needs a device) are in
tests/test_gpu_lm_weights.py."""
import ctypes as C
import os
import re

import pytest

INVALID = 1
NEW = ("slm_enable_data_weights", "slm_bind_data_semantic", "slm_data_weights")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "super_lm.h")


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


def test_null_arguments_are_refused(lib):
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    for name, args in (("slm_enable_data_weights", (None, 1, 0.0)), ("slm_bind_data_semantic", (None, 0, 2, one, one, one, None)),
                       ("slm_data_weights", (None, 0, one, None))):
        assert getattr(lib, name)(*args) == INVALID
        assert lib.slm_last_error() == name.encode() + b": null argument"


def test_exports_signatures_and_abi_version(lib):
    from super_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(raw, name)                                   # the built library exports it
        assert getattr(lib, name).restype == C.c_int
    assert _declaration("slm_enable_data_weights") == ["slm_solver* s", "int32_t seg_mode", "double pp_max"]
    assert _declaration("slm_bind_data_semantic") == ["slm_solver* s", "int32_t slot", "int32_t num_classes", "const int32_t* sf_seg",
                                                      "const float* sf_seg_conf", "const float* tgt_seg_conf", "void* stream"]
    assert _declaration("slm_data_weights") == ["slm_solver* s", "int32_t slot", "double* w_device", "void* stream"]
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.slm_enable_data_weights.argtypes == [vp, i32, C.c_double]
    assert lib.slm_bind_data_semantic.argtypes == [vp, i32, i32, vp, vp, vp, vp]
    assert lib.slm_data_weights.argtypes == [vp, i32, vp, vp]
    # no struct of the ABI changed: the version stays
    assert re.search(r"#define\s+SLM_ABI_VERSION\s+3\b", open(HEADER).read())
    assert _lib.SLM_ABI_VERSION == 3 and lib.slm_abi_version() == 3


def test_every_refusal_text_is_listed_in_the_header():
    text = open(HEADER).read()
    pre = "slm_enable_data_weights: "
    for t in (pre + "null argument", pre + "seg_mode must be 0 (none), 1 (hard) or 2 (soft)", pre + "pp_max must be finite and >= 0",
              pre + "a slot is already bound; call it after slm_create and before the first bind",
              pre + "needs the pair-record data path (data_path 0 or 2)", pre + "needs a nested-dissection solver_path (0, 2, 3 or 4)",
              pre + "needs the data term (use_data 1)", "slm_bind_frame: the data weights (slm_enable_data_weights) need J < 65536",
              "<fn>: slm_enable_data_weights first", "slm_bind_data_semantic: num_classes must be in 1..SLM_MAX_CLASSES (4)",
              "<fn>: slot <i> has no semantic inputs; call slm_bind_data_semantic after slm_bind_frame"):
        assert '"' + t + '"' in text, t


def test_python_surface_has_the_keyword():
    import inspect
    from super_amd.LM import LM_Solver
    assert inspect.signature(LM_Solver.__init__).parameters["weighted_data"].default is False
    assert callable(LM_Solver.data_weights)
