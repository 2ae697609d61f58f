"""The exports, signatures and struct of the rigid pre-alignment stage (slm_rigid_*), the refusals that need no context, the
header's list of every refusal text and the refusals of the Python mirror, after the pattern of
test_refusal_texts_lm_morph.py.  The refusals that need a context (slm_rigid_create needs a device) are in
tests/test_gpu_rigid.py."""
import ctypes as C
import os
import re

import pytest

INVALID = 1
NEW = ("slm_rigid_abi_check", "slm_rigid_create", "slm_rigid_destroy", "slm_rigid_run", "slm_rigid_get", "slm_rigid_get_beta",
       "slm_rigid_get_records", "slm_rigid_assemble", "slm_rigid_transform")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "super_lm.h")
SOURCE = os.path.join(ROOT, "python-super_amd", "csrc", "slm_rigid.hip")

# texts the library holds as one literal
LITERAL = ("slm_rigid_create: null argument", "slm_rigid_create: max_frames must be >= 1", "slm_rigid_create: no HIP device visible",
           "slm_rigid_run: null argument", "slm_rigid_run: n_frames must be in 1..max_frames",
           "slm_rigid_run: num_iterations must be >= 0", "slm_rigid_assemble: null argument",
           "slm_rigid_assemble: num_iterations must be >= 0", "slm_rigid_get_records: null argument",
           "slm_rigid_get_records: bad slot", "slm_rigid_get_records: max_records must be >= 0",
           "slm_rigid_transform: null argument", "slm_rigid_transform: n must be >= 0")
# the tails the frame check and the two read-backs put behind "<function>: "
TAILS = ("H and W must be >= 2", "N and T must be >= 0", "N > 0 needs sf_points",
         "T > 0 needs tgt_points, tgt_norms, index_map and tgt_valid", ": null argument", ": bad slot")


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


def test_null_arguments_and_ranges_are_refused_without_a_device(lib):
    one = C.c_void_p(8)   # a non-null pointer that is never followed
    from super_amd._lib import SlmFrame, SlmIterRecord, SlmRigidConfig
    cfg, fr, rec = SlmRigidConfig(), SlmFrame(), (SlmIterRecord * 1)()
    calls = (("slm_rigid_create", (1, None)),
             ("slm_rigid_run", (None, C.byref(cfg), 1, C.byref(fr), None)),
             ("slm_rigid_run", (one, None, 1, C.byref(fr), None)),
             ("slm_rigid_run", (one, C.byref(cfg), 1, None, None)),
             ("slm_rigid_get", (None, 0, one, None)), ("slm_rigid_get", (one, 0, None, None)),
             ("slm_rigid_get_beta", (None, 0, one, None)), ("slm_rigid_get_beta", (one, 0, None, None)),
             ("slm_rigid_get_records", (None, 0, rec, 1, None, None)), ("slm_rigid_get_records", (one, 0, None, 1, None, None)),
             ("slm_rigid_assemble", (None, C.byref(cfg), C.byref(fr), one, None, None, None, None)),
             ("slm_rigid_assemble", (one, None, C.byref(fr), one, None, None, None, None)),
             ("slm_rigid_assemble", (one, C.byref(cfg), None, one, None, None, None, None)),
             ("slm_rigid_assemble", (one, C.byref(cfg), C.byref(fr), None, None, None, None, None)),
             ("slm_rigid_transform", (5, one, one, 1, None, None)), ("slm_rigid_transform", (5, None, one, 1, one, None)))
    for name, args in calls:
        assert getattr(lib, name)(*args) == INVALID, (name, args)
        assert lib.slm_last_error() == name.encode() + b": null argument", (name, args)
    out = C.c_void_p()
    for n in (0, -3):
        assert lib.slm_rigid_create(n, C.byref(out)) == INVALID
        assert lib.slm_last_error() == b"slm_rigid_create: max_frames must be >= 1"
    assert lib.slm_rigid_transform(-1, one, None, 1, one, None) == INVALID
    assert lib.slm_last_error() == b"slm_rigid_transform: n must be >= 0"
    assert lib.slm_rigid_transform(0, None, None, 0, one, None) == 0       # nothing to move: no launch, no device needed
    assert lib.slm_rigid_destroy(None) == 0


def test_no_device_is_refused_loudly(lib):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    out = C.c_void_p()
    assert lib.slm_rigid_create(1, C.byref(out)) == 3
    assert lib.slm_last_error() == b"slm_rigid_create: no HIP device visible"
    from super_amd._lib import SuperLMError
    from super_amd.rigid import RigidAlign
    from oracle.lm_oracle import default_opt
    with pytest.raises(SuperLMError):
        RigidAlign(default_opt())


def test_struct_and_its_handshake(lib, tmp_path):
    import subprocess
    from super_amd._lib import SlmRigidConfig
    assert C.sizeof(SlmRigidConfig) == 2 * 4 + 5 * 8
    assert [f[0] for f in SlmRigidConfig._fields_] == ["num_iterations", "phase_test", "w_data", "w_rot", "u0", "v",
                                                        "minimal_loss0"]
    assert lib.slm_rigid_abi_check(C.sizeof(SlmRigidConfig)) == 0
    assert lib.slm_rigid_abi_check(C.sizeof(SlmRigidConfig) - 8) == INVALID
    assert lib.slm_last_error() == b"slm_rigid_abi_check: caller's slm_rigid_config has 40 bytes, the library's 48"
    # the header as plain C gives the same layout
    src = tmp_path / "size.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "super_lm.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu\\n", sizeof(slm_rigid_config), offsetof(slm_rigid_config, w_data),\n'
                   '         offsetof(slm_rigid_config, minimal_loss0));\n  return 0;\n}\n')
    exe = tmp_path / "size"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in got] == [C.sizeof(SlmRigidConfig), SlmRigidConfig.w_data.offset, SlmRigidConfig.minimal_loss0.offset]


def test_exports_and_signatures(lib):
    from super_amd import _lib
    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.EXPORTS
        getattr(raw, name)                                   # the built library exports it
        assert getattr(lib, name).restype == C.c_int
    assert _declaration("slm_rigid_create") == ["int32_t max_frames", "slm_rigid** out"]
    assert _declaration("slm_rigid_run") == ["slm_rigid* r", "const slm_rigid_config* cfg", "int32_t n_frames",
                                             "const slm_frame* frames", "void* stream"]
    assert _declaration("slm_rigid_get") == ["slm_rigid* r", "int32_t slot", "double* Tg7_device", "void* stream"]
    assert _declaration("slm_rigid_get_beta") == ["slm_rigid* r", "int32_t slot", "double* beta7_device", "void* stream"]
    assert _declaration("slm_rigid_get_records") == ["slm_rigid* r", "int32_t slot", "slm_iter_record* host_out",
                                                     "int32_t max_records", "int32_t* n_out", "void* stream"]
    assert _declaration("slm_rigid_assemble") == ["slm_rigid* r", "const slm_rigid_config* cfg", "const slm_frame* frame",
                                                  "const double* beta7_device", "double* JtJ49_device", "double* jtl7_device",
                                                  "double* loss_M_device", "void* stream"]
    assert _declaration("slm_rigid_transform") == ["int32_t n", "void* points", "void* norms", "int32_t f64",
                                                   "const double* Tg7_device", "void* stream"]
    vp, i32 = C.c_void_p, C.c_int32
    assert lib.slm_rigid_run.argtypes == [vp, C.POINTER(_lib.SlmRigidConfig), i32, C.POINTER(_lib.SlmFrame), vp]
    assert lib.slm_rigid_get_records.argtypes == [vp, i32, C.POINTER(_lib.SlmIterRecord), i32, C.POINTER(C.c_int32), vp]
    assert lib.slm_rigid_assemble.argtypes == [vp, C.POINTER(_lib.SlmRigidConfig), C.POINTER(_lib.SlmFrame), vp, vp, vp, vp, vp]
    assert lib.slm_rigid_transform.argtypes == [i32, vp, vp, i32, vp, vp]
    # the stage is an addition: no existing struct or entry point changed, the version stays
    assert re.search(r"#define\s+SLM_ABI_VERSION\s+3\b", open(HEADER).read())
    assert _lib.SLM_ABI_VERSION == 3 and lib.slm_abi_version() == 3


def test_every_refusal_text_is_listed_in_the_header_and_raised_by_the_library():
    header = open(HEADER).read()
    source = re.sub(r'"\s*\n\s*"', "", open(SOURCE).read())   # adjacent string literals are one text
    for t in LITERAL:
        assert '"' + t + '"' in header or '"<fn>' + t[t.index(":"):] + '"' in header, t
        assert '"' + t + '"' in source or '"' + t[t.index(":"):] + '"' in source, t
    for t in TAILS:
        assert t + '"' in header, t
        assert t + '"' in source, t
    assert '"slm_rigid_abi_check: caller\'s slm_rigid_config has <a> bytes, the library\'s <b>"' in header
    assert '"slm_rigid_abi_check: caller\'s slm_rigid_config has "' in source
    for fn in ("slm_rigid_run", "slm_rigid_assemble"):
        assert 'check_frame("' + fn + '"' in source
    for fn in ("slm_rigid_get", "slm_rigid_get_beta"):
        assert 'rg_get("' + fn + '"' in source


def test_python_surface_and_its_refusals():
    import inspect
    from types import SimpleNamespace
    from super_amd import rigid
    from super_amd.LM import LM_Solver
    from oracle.lm_oracle import default_opt
    assert inspect.signature(LM_Solver.__init__).parameters["global_rigid"].default is False
    assert inspect.signature(rigid.RigidAlign.__init__).parameters["max_frames"].default == 1
    for name in ("align", "align_batch", "assemble", "records", "beta"):
        assert callable(getattr(rigid.RigidAlign, name))
    assert callable(rigid.rigid_update) and callable(rigid.rigid_transform)
    # refused before anything touches the device
    with pytest.raises(NotImplementedError, match="global_rigid with shard_surfels is not built"):
        LM_Solver(default_opt(), global_rigid=True, shard_surfels=True)
    with pytest.raises(NotImplementedError, match="global_rigid with shard_surfels is not built"):
        LM_Solver(default_opt(), global_rigid=True, rank=0, world=2)
    with pytest.raises(ValueError, match="max_frames must be >= 1"):
        rigid.RigidAlign(default_opt(), max_frames=0)
    import torch
    cpu = SimpleNamespace(points=torch.zeros(4, 3, dtype=torch.float64))
    with pytest.raises(Exception, match="HIP device"):
        rigid.RigidFrame(cpu, {}, SimpleNamespace())
    with pytest.raises(ValueError, match="contiguous float32 or float64"):
        rigid.rigid_transform(torch.zeros(4, 3, dtype=torch.float16), None, torch.zeros(7))
    with pytest.raises(ValueError, match="agree in dtype and shape"):
        rigid.rigid_transform(torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.float64), torch.zeros(7))
