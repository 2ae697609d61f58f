"""The two host thread pools of the LM host (python-super_amd/csrc/slm_workers.h: AsyncWorker behind slm_prepare_model,
BindPool behind slm_bind_frames) under ThreadSanitizer, and again under AddressSanitizer + UBSan.  The header is standard
library only, so this is a plain g++ program with its own main: no HIP, no GPU, at most 8 threads."""
import os
import shutil
import subprocess
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MAIN = textwrap.dedent('''
    #include <atomic>
    #include <cassert>
    #include <cstdio>
    #include <set>
    #include "slm_workers.h"
    int main() {
      { AsyncWorker never_started; }
      {
        AsyncWorker w;
        std::vector<int> order;                       // written by the worker only; read after wait / shutdown
        std::atomic<int> done{0};
        unsigned long long t100 = 0;
        for (int i = 0; i < 200; ++i) {
          const unsigned long long t = w.submit([&order, &done, i] { order.push_back(i); done.store(i + 1); });
          assert(t == (unsigned long long)i + 1);
          if (i == 99) t100 = t;
        }
        w.wait(t100);
        assert(done.load() >= 100);                   // wait(ticket) returns after that job
        w.shutdown();                                 // runs what is queued ...
        assert(order.size() == 200);
        for (int i = 0; i < 200; ++i) assert(order[i] == i);   // ... in submission order
        w.shutdown();                                 // idempotent
      }
      {
        BindPool pool;
        int calls[8];
        std::mutex m;
        std::set<std::thread::id> ids;
        for (int r = 0; r < 300; ++r) {
          const int n = r % 8 + 1;
          for (int& c : calls) c = 0;
          const std::function<void(int)> job = [&](int i) {
            ++calls[i];                               // job(i) is run by one thread: no two touch the same entry
            std::lock_guard<std::mutex> lk(m);
            ids.insert(std::this_thread::get_id());
          };
          pool.run(n, job);
          for (int i = 0; i < 8; ++i) assert(calls[i] == (i < n ? 1 : 0));   // each of job(0..n-1) exactly once
        }
        assert(ids.size() == 8);                      // the caller and 7 workers that persist between the calls
        pool.shutdown();
      }
      std::puts("workers ok");
    }
''')


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_worker_pools_are_clean_under_the_sanitizers(tmp_path, sanitizer):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    (tmp_path / "main.cpp").write_text(MAIN)
    exe = str(tmp_path / "workers")
    subprocess.check_call([gxx, "-O1", "-g", "-fsanitize=" + sanitizer, "-fno-sanitize-recover=all", "-std=c++17", "-pthread",
                           "-I", os.path.join(ROOT, "python-super_amd", "csrc"), str(tmp_path / "main.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "workers ok" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
