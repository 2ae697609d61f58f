"""The exports, signatures and ABI version of slm_enable_face, slm_set_face_mesh and slm_face_loss, the refusals that need no
solver, and the header's list of every refusal text, after the pattern of test_refusal_texts_lm_weights.py.  The refusals that
need a solver (slm_create needs a device) are in tests/test_gpu_lm_face.py."""
import ctypes as C
import os
import re

import pytest

INVALID = 1
NEW = ("slm_enable_face", "slm_set_face_mesh", "slm_face_loss")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "super_lm.h")
CSRC = os.path.join(ROOT, "python-super_amd", "csrc")


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
    for name, args in (("slm_enable_face", (None, 1.0)), ("slm_set_face_mesh", (None, 0, 1, one, one, None)),
                       ("slm_face_loss", (None, 0, one, None))):
        assert getattr(lib, name)(*args) == INVALID
        assert lib.slm_last_error() == name.encode() + b": null argument"


def test_exports_signatures_and_abi_version(lib):
    from super_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(raw, name)                                   # the built library exports it
        assert getattr(lib, name).restype == C.c_int
    assert _declaration("slm_enable_face") == ["slm_solver* s", "double weight"]
    assert _declaration("slm_set_face_mesh") == ["slm_solver* s", "int32_t slot", "int32_t n_triangles", "const int32_t* tri",
                                                 "const double* areas", "void* stream"]
    assert _declaration("slm_face_loss") == ["slm_solver* s", "int32_t slot", "double* out_device", "void* stream"]
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.slm_enable_face.argtypes == [vp, C.c_double]
    assert lib.slm_set_face_mesh.argtypes == [vp, i32, i32, vp, vp, vp]
    assert lib.slm_face_loss.argtypes == [vp, i32, vp, vp]
    # no struct of the ABI changed: the version stays
    assert re.search(r"#define\s+SLM_ABI_VERSION\s+3\b", open(HEADER).read())
    assert _lib.SLM_ABI_VERSION == 3 and lib.slm_abi_version() == 3


def test_every_refusal_text_is_listed_in_the_header_and_raised_by_the_library():
    header = open(HEADER).read()
    source = "".join(open(os.path.join(CSRC, f)).read() for f in ("slm_lm.hip", "slm_terms.hip", "slm_bind.hip"))
    source = re.sub(r'"\s*\n\s*"', "", source)               # adjacent string literals are one text
    pre = "slm_enable_face: "
    for t in (pre + "null argument", pre + "weight must be finite",
              pre + "a slot is already bound; call it after slm_create and before the first bind",
              pre + "needs the pair-record data path (data_path 0 or 2)", pre + "needs a nested-dissection solver_path (0, 2, 3 or 4)",
              pre + "needs the data term (use_data 1)",
              pre + "the solver is sharded (slm_set_shard); the term's mesh is not sharded",
              "slm_set_shard: the face term is enabled (slm_enable_face); its mesh is not sharded",
              "slm_bind_frame: the face term (slm_enable_face) needs J < 65536",
              "slm_set_face_mesh: null argument", "slm_set_face_mesh: bad slot", "slm_set_face_mesh: n_triangles must be >= 0",
              "slm_set_face_mesh: slm_enable_face first",
              "slm_bind_frame: a triangle of the slot's face mesh (slm_set_face_mesh) has a node id outside [0, J) or repeats an id",
              "slm_face_loss: null argument", "slm_face_loss: bad slot", "slm_face_loss: slm_enable_face first",
              "slm_face_loss: slm_bind_frame first"):
        assert '"' + t + '"' in header, t
        assert '"' + t + '"' in source, t


def test_python_surface_has_the_keyword():
    import inspect
    from super_amd.LM import LM_Solver
    assert inspect.signature(LM_Solver.__init__).parameters["face_term"].default is False
    assert callable(LM_Solver.face_loss)
