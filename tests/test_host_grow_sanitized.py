"""The shared growth function of the stage hosts (python-super_amd/csrc/slm_host.h: grow) under AddressSanitizer + UBSan,
compiled as plain C++ against a two-function stand-in for the HIP allocator: grow, fail, grow again.  After a failed
allocation the pointer is null AND the capacity is 0, so the next call allocates instead of handing out the null."""
import os
import shutil
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = textwrap.dedent('''
    #pragma once
    #include <cstdlib>
    enum hipError_t { hipSuccess = 0, hipErrorOutOfMemory = 2 };
    inline bool g_fail_next = false;
    inline int g_live = 0;
    inline hipError_t hipMalloc(void** p, size_t n) {
      if (g_fail_next) { g_fail_next = false; return hipErrorOutOfMemory; }
      *p = std::malloc(n ? n : 1); ++g_live; return hipSuccess;
    }
    inline hipError_t hipFree(void* p) { std::free(p); --g_live; return hipSuccess; }
    inline const char* hipGetErrorString(hipError_t) { return "out of memory"; }
''')
MAIN = textwrap.dedent('''
    #include <cassert>
    #include <cstdio>
    #include "slm_host.h"
    void slm_set_error_text(const char*) {}
    int main() {
      double* p = nullptr; size_t cap = 0;
      assert(grow(p, cap, 100, 112) == hipSuccess && p && cap == 112 && g_live == 1);
      p[111] = 1.0;
      double* q = p;
      assert(grow(p, cap, 112, 126) == hipSuccess && p == q && cap == 112);          // fits: untouched
      g_fail_next = true;
      assert(grow(p, cap, 200, 225) == hipErrorOutOfMemory && !p && cap == 0 && g_live == 0);
      assert(grow(p, cap, 50, 50) == hipSuccess && p && cap == 50 && g_live == 1);   // not "50 <= 112: nothing to do"
      p[49] = 2.0;
      void* t = nullptr; size_t tc = 0; int calls = 0;
      auto call = [&](void* tmp, size_t& bytes) { ++calls; if (!tmp) bytes = 64; else static_cast<char*>(tmp)[bytes - 1] = 1; return hipSuccess; };
      assert(with_scratch(t, tc, call) == hipSuccess && t && tc == 64 && calls == 2);
      hipFree(p); hipFree(t);
      assert(g_live == 0);
      std::puts("grow ok");
    }
''')


def test_grow_after_a_failed_allocation_is_clean_under_asan_and_ubsan(tmp_path):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text(SHIM)
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = str(tmp_path / "grow_asan")
    subprocess.check_call([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-std=c++17",
                           "-I", str(tmp_path), "-I", os.path.join(ROOT, "python-super_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "grow ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
