"""The exports, signatures and ABI version of slm_enable_morph, slm_bind_morph, slm_morph_loss and slm_morph_targets, the
refusals that need no solver, and the header's list of every refusal text, after the pattern of
test_refusal_texts_lm_face.py.  The refusals that need a solver (slm_create needs a device) are in
tests/test_gpu_lm_morph.py."""
import ctypes as C
import os
import re

import pytest

INVALID = 1
NEW = ("slm_enable_morph", "slm_bind_morph", "slm_morph_loss", "slm_morph_targets")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "super_lm.h")
CSRC = os.path.join(ROOT, "python-super_amd", "csrc")

PRE = "slm_enable_morph: "
SHARDED = "the solver is sharded (slm_set_shard); the term needs every surfel of the frame on one device"
# texts the library holds as one literal
LITERAL = (PRE + "null argument", PRE + "weight must be finite",
           PRE + "a slot is already bound; call it after slm_create and before the first bind",
           PRE + "needs the pair-record data path (data_path 0 or 2)", PRE + "needs a nested-dissection solver_path (0, 2, 3 or 4)",
           PRE + "needs the data term (use_data 1)", PRE + SHARDED,
           "slm_set_shard: the boundary-morph term is enabled (slm_enable_morph); it needs every surfel of the frame on one device",
           "slm_bind_frame: the boundary-morph term (slm_enable_morph) needs J < 65536",
           "slm_bind_morph: num_classes must be in 1..SLM_MAX_CLASSES (4)", "slm_morph_targets: slm_bind_morph first")
# texts the per-slot entry points compose as "<function>: " + the shared tail (term_slot, slm_terms.hip)
COMPOSED = ("slm_bind_morph: null argument", "slm_bind_morph: bad slot", "slm_bind_morph: slm_enable_morph first",
            "slm_bind_morph: slm_bind_frame first", "<fn>: null argument", "<fn>: bad slot", "<fn>: slm_enable_morph first",
            "<fn>: slm_bind_frame first")


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
    for name, args in (("slm_enable_morph", (None, 1.0)), ("slm_bind_morph", (None, 0, 3, one, one, one, None, None)),
                       ("slm_morph_loss", (None, 0, one, None)), ("slm_morph_targets", (None, 0, one, one, one, None))):
        assert getattr(lib, name)(*args) == INVALID
        assert lib.slm_last_error() == name.encode() + b": null argument"


def test_exports_signatures_and_abi_version(lib):
    from super_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(raw, name)                                   # the built library exports it
        assert getattr(lib, name).restype == C.c_int
    assert _declaration("slm_enable_morph") == ["slm_solver* s", "double weight"]
    assert _declaration("slm_bind_morph") == ["slm_solver* s", "int32_t slot", "int32_t num_classes", "const int32_t* img_seg",
                                              "const float* img_seg_conf", "const int32_t* sf_seg", "int32_t* edge_counts_host",
                                              "void* stream"]
    assert _declaration("slm_morph_loss") == ["slm_solver* s", "int32_t slot", "double* out_device", "void* stream"]
    assert _declaration("slm_morph_targets") == ["slm_solver* s", "int32_t slot", "uint8_t* kept", "double* target_xy", "double* li",
                                                 "void* stream"]
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.slm_enable_morph.argtypes == [vp, C.c_double]
    assert lib.slm_bind_morph.argtypes == [vp, i32, i32, vp, vp, vp, C.POINTER(C.c_int32), vp]
    assert lib.slm_morph_loss.argtypes == [vp, i32, vp, vp]
    assert lib.slm_morph_targets.argtypes == [vp, i32, vp, vp, vp, vp]
    # no struct of the ABI changed: the version stays
    assert re.search(r"#define\s+SLM_ABI_VERSION\s+3\b", open(HEADER).read())
    assert _lib.SLM_ABI_VERSION == 3 and lib.slm_abi_version() == 3


def test_every_refusal_text_is_listed_in_the_header_and_raised_by_the_library():
    header = open(HEADER).read()
    source = "".join(open(os.path.join(CSRC, f)).read() for f in ("slm_lm.hip", "slm_terms.hip", "slm_bind.hip"))
    source = re.sub(r'"\s*\n\s*"', "", source)               # adjacent string literals are one text
    for t in LITERAL:
        assert '"' + t + '"' in header, t
        assert '"' + t + '"' in source, t
    for t in COMPOSED:
        assert '"' + t + '"' in header, t
    for fn in ("slm_bind_morph", "slm_morph_loss", "slm_morph_targets"):
        assert 'term_slot("' + fn + '"' in source and '"slm_enable_morph", &sp)' in source


def test_python_surface_has_the_keyword():
    import inspect
    from super_amd.LM import LM_Solver
    assert inspect.signature(LM_Solver.__init__).parameters["morph_term"].default is False
    assert isinstance(LM_Solver.last_morph_loss, property) and callable(LM_Solver.morph_targets)
