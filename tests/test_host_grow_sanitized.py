"""The shared growth function of the stage hosts (python-super_amd/csrc/slm_host.h: grow) under AddressSanitizer + UBSan,
compiled as plain C++ against a two-function stand-in for the HIP allocator: grow, fail, grow again.  After a failed
allocation the pointer is null AND the capacity is 0, so the next call allocates instead of handing out the null.
The same for its owning forms, DevBuf and PinnedBuf (a pinned pair in the stand-in): they free once, a move empties
its source, and a vector of structs of them leaves nothing live."""
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
    enum { hipHostMallocDefault = 0 };
    inline int g_live_pinned = 0;
    inline hipError_t hipHostMalloc(void** p, size_t n, unsigned) {
      if (g_fail_next) { g_fail_next = false; return hipErrorOutOfMemory; }
      *p = std::malloc(n ? n : 1); ++g_live_pinned; return hipSuccess;
    }
    inline hipError_t hipHostFree(void* p) { std::free(p); --g_live_pinned; return hipSuccess; }
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


# The owners over it (DevBuf, PinnedBuf): a slot of the LM solver is a struct of them with no release list.
MAIN_BUF = textwrap.dedent('''
    #include <cassert>
    #include <cstdio>
    #include <type_traits>
    #include <utility>
    #include <vector>
    #include "slm_host.h"
    void slm_set_error_text(const char*) {}
    struct Slot { DevBuf<double> a, b; DevBuf<int> c; PinnedBuf<float> h; int tag = 0; };
    template <typename B> void life() {   // grow, keep, fail, grow again; move
      int& live = std::is_same<B, DevBuf<double>>::value ? g_live : g_live_pinned;
      {
        B x;
        assert(x.grow(100, 112) == hipSuccess && x.p && x.cap == 112 && live == 1);
        x.p[111] = 1.0;
        double* q = x.p;
        assert(x.grow(112, 126) == hipSuccess && x.p == q && x.cap == 112 && live == 1);   // fits: untouched
        g_fail_next = true;
        assert(x.grow(200, 225) == hipErrorOutOfMemory && !x.p && x.cap == 0 && live == 0);
        assert(x.grow(50, 50) == hipSuccess && x.p && x.cap == 50 && live == 1);
        x.p[49] = 2.0;
        q = x.p;
        B y(std::move(x));
        assert(!x.p && x.cap == 0 && y.p == q && y.cap == 50 && live == 1);            // the source is empty ...
      }
      assert(live == 0);                                                               // ... and the buffer was freed once
    }
    int main() {
      life<DevBuf<double>>();
      life<PinnedBuf<double>>();
      { DevBuf<double> d; PinnedBuf<int> p; }                                          // never grown: nothing to free
      assert(g_live == 0 && g_live_pinned == 0);
      {
        DevBuf<double> d;
        assert(d.grow(8, 8) == hipSuccess);
        double* raw = d;                                                               // converts to T*
        assert(raw == d.p);
        PinnedBuf<int> p;
        assert(p.resize(10) == hipSuccess && p.size() == 10 && p.cap >= 10 && p.end() - p.begin() == 10);
        p[9] = 3;
        g_fail_next = true;
        assert(p.resize(1000) == hipErrorOutOfMemory && !p.data() && p.cap == 0 && p.size() == 0 && g_live_pinned == 0);
        assert(p.resize(20) == hipSuccess && p.size() == 20);
        p[19] = 4;
      }
      assert(g_live == 0 && g_live_pinned == 0);
      {
        std::vector<Slot> v;
        v.resize(3);
        for (Slot& s : v) assert(s.a.grow(4, 4) == hipSuccess && s.c.grow(2, 2) == hipSuccess && s.h.resize(5) == hipSuccess);
        assert(g_live == 6 && g_live_pinned == 3);
        double* a0 = v[0].a.p;
        v.resize(64);                                                                  // reallocates: the slots move
        assert(v[0].a.p == a0 && !v[0].b.p && g_live == 6 && g_live_pinned == 3);
        v[63].b.grow(1, 1);
        v.resize(2);                                                                   // destroys slot 2 and slot 63
        assert(g_live == 4 && g_live_pinned == 2);
      }
      assert(g_live == 0 && g_live_pinned == 0);
      std::puts("buffers ok");
    }
''')


def _run_sanitized(tmp_path, main, say):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text(SHIM)
    (tmp_path / "main.cpp").write_text(main)
    exe = str(tmp_path / "grow_asan")
    subprocess.check_call([gxx, "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-std=c++17",
                           "-I", str(tmp_path), "-I", os.path.join(ROOT, "python-super_amd", "csrc"),
                           "-I", os.path.join(ROOT, "include"), str(tmp_path / "main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and say in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])


def test_grow_after_a_failed_allocation_is_clean_under_asan_and_ubsan(tmp_path):
    _run_sanitized(tmp_path, MAIN, "grow ok")


def test_owning_buffers_free_once_under_asan_and_ubsan(tmp_path):
    _run_sanitized(tmp_path, MAIN_BUF, "buffers ok")
