// slm_workers.h -- the two host thread pools of the LM host: AsyncWorker (slm_prepare_model) and BindPool
// (slm_bind_frames).  Standard library only, no HIP: the file builds, and is tested under the sanitizers, without hipcc.
#pragma once
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

// One persistent host thread running queued jobs in order (slm_prepare_model): created on first use, joined in slm_destroy.
class AsyncWorker {
 public:
  ~AsyncWorker() { shutdown(); }
  // returns the job's ticket (> 0); throws only from thread creation / allocation, before the job is queued
  unsigned long long submit(std::function<void()> job) {
    std::lock_guard<std::mutex> lk(m_);
    if (!started_) {
      thread_ = std::thread([this] { loop(); });
      started_ = true;
    }
    jobs_.push_back(std::move(job));
    cv_work_.notify_one();
    return ++submitted_;
  }
  void wait(unsigned long long ticket) {
    std::unique_lock<std::mutex> lk(m_);
    cv_done_.wait(lk, [&] { return completed_ >= ticket; });
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(m_);
      if (!started_) return;
      stop_ = true;
    }
    cv_work_.notify_all();
    if (thread_.joinable()) thread_.join();
    started_ = false;
  }

 private:
  void loop() {
    for (;;) {
      std::function<void()> job;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_work_.wait(lk, [&] { return stop_ || !jobs_.empty(); });
        if (jobs_.empty()) return;     // (stop: queued jobs are still run first)
        job = std::move(jobs_.front());
        jobs_.erase(jobs_.begin());
      }
      job();
      {
        std::lock_guard<std::mutex> lk(m_);
        ++completed_;
      }
      cv_done_.notify_all();
    }
  }
  std::thread thread_;
  std::mutex m_;
  std::condition_variable cv_work_, cv_done_;
  std::vector<std::function<void()>> jobs_;
  unsigned long long submitted_ = 0, completed_ = 0;
  bool started_ = false, stop_ = false;
};

// Persistent host workers of slm_bind_frames: created on first use, parked on a condition variable between calls, joined
// in slm_destroy.  (One std::thread per frame and call cost a spawn + join per tracking step inside the timed region
// and could throw through the extern "C" boundary.)
class BindPool {
 public:
  ~BindPool() { shutdown(); }
  // runs job(1) .. job(n - 1) on the workers and job(0) on the caller; returns when all are done.  Throws only from
  // ensure() (thread creation), before any job has started.
  void run(int n, const std::function<void(int)>& job) {
    ensure(n - 1);
    {
      std::lock_guard<std::mutex> lk(m_);
      job_ = &job;
      n_active_ = n - 1;
      pending_ = n - 1;
      ++generation_;
    }
    cv_work_.notify_all();
    job(0);
    std::unique_lock<std::mutex> lk(m_);
    cv_done_.wait(lk, [&] { return pending_ == 0; });
    job_ = nullptr;
  }
  void shutdown() {
    {
      std::lock_guard<std::mutex> lk(m_);
      stop_ = true;
    }
    cv_work_.notify_all();
    for (std::thread& t : threads_)
      if (t.joinable()) t.join();
    threads_.clear();
  }

 private:
  void ensure(int n_workers) {
    while ((int)threads_.size() < n_workers) {
      const int id = (int)threads_.size();      // worker id runs job(id + 1)
      threads_.emplace_back([this, id] { loop(id); });
    }
  }
  void loop(int id) {
    int seen = 0;
    for (;;) {
      const std::function<void(int)>* job = nullptr;
      {
        std::unique_lock<std::mutex> lk(m_);
        cv_work_.wait(lk, [&] { return stop_ || generation_ != seen; });
        if (stop_) return;
        seen = generation_;
        if (id < n_active_) job = job_;
      }
      if (job) {
        (*job)(id + 1);
        std::lock_guard<std::mutex> lk(m_);
        if (--pending_ == 0) cv_done_.notify_all();
      }
    }
  }
  std::vector<std::thread> threads_;
  std::mutex m_;
  std::condition_variable cv_work_, cv_done_;
  const std::function<void(int)>* job_ = nullptr;
  int generation_ = 0, n_active_ = 0, pending_ = 0;
  bool stop_ = false;
};
