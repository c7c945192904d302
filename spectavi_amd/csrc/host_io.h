// host_io.h -- the host-pointer paths' transfer machinery: cached device buffers, pre-faulting of the
// caller's result arrays, and the threaded pinned pipeline that brings large results back.
#pragma once

#include "common.h"

#include <atomic>
#include <condition_variable>
#include <initializer_list>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace spv {

// RAII device buffer for the host-pointer paths, allocated on the current device from a per-device
// cache of freed buffers: repeated calls (a front-end matching image pairs, RANSAC-style loops over
// dlt_triangulate) would otherwise pay a hipMalloc/hipFree pair per buffer.  The buffer goes back to
// the cache only after this thread's stream has drained (the destructor synchronises it: a no-op on
// the normal path, which has already synchronised, and the safety net on error paths), so a later
// owner on another stream never sees work in flight.
struct DevBuf {
  void *p = nullptr;
  size_t cap = 0;
  int dev = 0;
  ~DevBuf();
  int alloc(size_t bytes);
  template <typename T>
  T *as() {
    return static_cast<T *>(p);
  }
  // host -> this buffer / this buffer -> host, queued on `st`; nothing is queued for 0 bytes
  int copy_in(const void *src, size_t bytes, hipStream_t st) {
    if (bytes) SPV_HIP_CHECK(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, st));
    return SPV_OK;
  }
  int copy_out(void *dst, size_t bytes, hipStream_t st) {
    if (bytes) SPV_HIP_CHECK(hipMemcpyAsync(dst, p, bytes, hipMemcpyDeviceToHost, st));
    return SPV_OK;
  }
  int upload(const void *src, size_t bytes, hipStream_t st) {
    SPV_TRY(alloc(bytes));
    return copy_in(src, bytes, st);
  }
  // For a call that returns while its kernels are still queued on the caller's stream `st`: the buffer leaves
  // this holder now and goes back to the cache once everything queued on `st` so far has ended (an event; a later
  // alloc() or release_transfer_caches() collects it).  Nothing waits here unless the event cannot be made.
  void release_after(hipStream_t st);
};

// Allocates each (buffer, bytes) in turn; stops at the first failure.
inline int alloc_all(std::initializer_list<std::pair<DevBuf *, size_t>> bufs) {
  for (const auto &b : bufs) SPV_TRY(b.first->alloc(b.second));
  return SPV_OK;
}

// The most bytes the cache behind DevBuf keeps per device; a call that can run in pieces asks for no more at once.
constexpr size_t kDevicePoolCapBytes = (size_t)4 << 30;

// Empties the device buffer cache and the pinned staging cache (spv_release_cached_memory).
void release_transfer_caches();

// A caller's fresh result array (np.empty) has no pages yet: the device-to-host copy then
// runs at the page-fault rate (~11 GB/s measured) instead of the link rate.  Large outputs are
// therefore touched -- one byte per page, from a few threads -- while the inputs travel and the
// kernels run; the contents of an output buffer are undefined before the call returns, so
// writing to it early is allowed.  Skipped when the output overlaps an input.
class HostPrefault {
 public:
  // Pages are touched in 2 MB blocks dealt round-robin to the threads (block j belongs to thread
  // j % T), so the front of the array is ready first and wait_range() can release a consumer
  // that only needs a prefix while the rest is still being touched.
  static constexpr size_t kBlock = (size_t)2 << 20;
  HostPrefault(void *dst, size_t bytes, std::initializer_list<std::pair<const void *, size_t>> inputs);
  // Returns once no prefault store can land in [off, off + len) any more: a consumer must call
  // this (or wait()) before it writes real data there -- a late `p[off] = 0` would otherwise
  // overwrite one byte per page of the result.
  void wait_range(size_t off, size_t len) {
    if (nthreads_ == 0 || len == 0) return;
    const size_t b0 = off / kBlock, b1 = (off + len - 1) / kBlock;
    for (size_t b = b0; b <= b1; ++b) {
      const int owner = (int)(b % (size_t)nthreads_);
      const size_t need = b / (size_t)nthreads_ + 1;  // blocks the owner must have finished
      while (done_[owner].load(std::memory_order_acquire) < need) std::this_thread::yield();
    }
  }
  void wait() {
    for (auto &t : threads_)
      if (t.joinable()) t.join();
    threads_.clear();
  }
  ~HostPrefault() { wait(); }

 private:
  std::vector<std::thread> threads_;
  std::unique_ptr<std::atomic<size_t>[]> done_;
  int nthreads_ = 0;
};

// ---- results back to pageable host memory ------------------------------------------------
// A device-to-host copy into a caller's ordinary (pageable) array runs at ~16 GB/s: the runtime
// stages it through pinned memory and copies out of the staging buffer with one host thread.  For
// large results the library does that staging itself with several threads: each worker owns a slice
// of every chunk, two pinned bounce buffers and its own stream; it waits for the chunk's producer
// event on the device side, copies device -> pinned at the link rate, and copies pinned -> the
// caller's array while its next slice is already in flight.  Chunks become available as the caller
// announces them (ready()), so a chunked computation overlaps its uploads and kernels with the
// download of the chunks before.
class D2HPipeline {
 public:
  static constexpr size_t kMinBytes = (size_t)16 << 20;  // below this a plain copy is as good
  D2HPipeline(int dev, const void *d_src, void *h_dst, size_t bytes, size_t chunk_bytes);
  // The caller's array is still being pre-touched by `touch`: every slice waits for its own pages
  // before the pinned -> caller copy (call before the first ready(); touch must outlive finish()).
  void set_prefault(HostPrefault *touch) { prefault_ = touch; }
  // chunk k (bytes [k * chunk, (k+1) * chunk) of the source) is final once `ev` has passed;
  // chunks must be announced in order.  ev must outlive finish().
  void ready(int k, hipEvent_t ev) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      events_[k] = ev;
      ready_ = k + 1;
    }
    cv_.notify_all();
  }
  void abort() {
    {
      std::lock_guard<std::mutex> lk(mu_);
      aborted_ = true;
    }
    cv_.notify_all();
  }
  int finish() {
    for (auto &t : threads_)
      if (t.joinable()) t.join();
    threads_.clear();
    if (aborted_) return SPV_OK;  // the caller reports its own error
    if (status_.load() != SPV_OK) return set_error(status_.load(), "%s", message_.c_str());
    for (int t = started_; t < workers_; ++t) work(t);  // slices of workers that never started
    if (status_.load() != SPV_OK) return set_error(status_.load(), "%s", message_.c_str());
    return SPV_OK;
  }
  ~D2HPipeline() {
    abort();
    for (auto &t : threads_)
      if (t.joinable()) t.join();
  }

 private:
  void fail(int st, const char *what, hipError_t e) {
    std::lock_guard<std::mutex> lk(mu_);
    if (status_.load() == SPV_OK) {
      message_ = std::string(what) + ": " + hipGetErrorString(e);
      status_.store(st);
    }
  }
  void work(int t);

  int dev_;
  const char *src_;
  char *dst_;
  size_t bytes_, chunk_;
  int nchunks_;
  std::vector<hipEvent_t> events_;
  int workers_ = 1, started_ = 0;
  size_t piece_ = 0;
  HostPrefault *prefault_ = nullptr;
  std::vector<std::thread> threads_;
  std::mutex mu_;
  std::condition_variable cv_;
  int ready_ = 0;
  bool aborted_ = false;
  std::atomic<int> status_{SPV_OK};
  std::string message_;
};

// An event recorded on `st` now, destroyed with the holder.
struct ScopedEvent {
  hipEvent_t ev = nullptr;
  int record(hipStream_t st) {
    SPV_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    SPV_HIP_CHECK(hipEventRecord(ev, st));
    return SPV_OK;
  }
  ~ScopedEvent() {
    if (ev) (void)hipEventDestroy(ev);
  }
};

// Device result -> caller's array: through the threaded pinned pipeline when large, else one copy.
// `st` is the stream the producing kernels were enqueued on; returns after the data has arrived.
int download(int dev, void *h_dst, const void *d_src, size_t bytes, hipStream_t st);

}  // namespace spv
