// mifc_copypool.h -- the copy threads of the host pipeline (mifc_hostpipe.hip).  Plain C++ threads, no HIP: a host
// program can include this file alone (tests/host/copypool_main.cc does, also under the thread and address sanitizers).
#ifndef MIFC_COPYPOOL_H
#define MIFC_COPYPOOL_H

#include <condition_variable>
#include <cstddef>
#include <cstring>
#include <deque>
#include <mutex>
#include <thread>
#include <vector>

namespace mifc {

// A handful of threads that do nothing but memcpy between the caller's
// pageable memory and the pinned staging buffers.  copy() may be called from
// two threads at once (the feeding and the draining side of the pipeline).
class CopyPool
{
public:
  explicit CopyPool(int nthreads)
  {
    for (int t = 0; t < nthreads; ++t)
      workers_.emplace_back([this] { work(); });
  }
  ~CopyPool()
  {
    {
      std::lock_guard<std::mutex> g(m_);
      stop_ = true;
    }
    cv_job_.notify_all();
    for (auto& t : workers_)
      t.join();
  }
  void copy(void* dst, const void* src, size_t bytes)
  {
    const size_t slice = size_t(2) << 20;
    int pending = 0;
    {
      std::lock_guard<std::mutex> g(m_);
      for (size_t off = 0; off < bytes; off += slice) {
        Slice s;
        s.dst = static_cast<char*>(dst) + off;
        s.src = static_cast<const char*>(src) + off;
        s.bytes = (off + slice > bytes) ? bytes - off : slice;
        s.pending = &pending;
        jobs_.push_back(s);
        ++pending;
      }
    }
    cv_job_.notify_all();
    std::unique_lock<std::mutex> g(m_);
    cv_done_.wait(g, [&] { return pending == 0; });
  }

private:
  struct Slice
  {
    char* dst;
    const char* src;
    size_t bytes;
    int* pending; // guarded by m_
  };
  void work()
  {
    for (;;) {
      Slice s;
      {
        std::unique_lock<std::mutex> g(m_);
        cv_job_.wait(g, [&] { return stop_ || !jobs_.empty(); });
        if (jobs_.empty())
          return;
        s = jobs_.front();
        jobs_.pop_front();
      }
      std::memcpy(s.dst, s.src, s.bytes);
      {
        std::lock_guard<std::mutex> g(m_);
        if (--*s.pending == 0)
          cv_done_.notify_all();
      }
    }
  }
  std::vector<std::thread> workers_;
  std::mutex m_;
  std::condition_variable cv_job_, cv_done_;
  std::deque<Slice> jobs_;
  bool stop_ = false;
};

} // namespace mifc

#endif // MIFC_COPYPOOL_H
