// host_io.hip -- transfer machinery of the host-pointer paths (host_io.h).

#include "host_io.h"

#include <cstring>
#include <map>

namespace spv {

namespace {

// The per-device cache behind DevBuf.  Grow-only up to kPoolCapBytes per device;
// release_transfer_caches() empties it.
class DevicePool {
 public:
  static constexpr size_t kPoolCapBytes = kDevicePoolCapBytes;
  void *acquire(int dev, size_t bytes, size_t *got) {
    std::lock_guard<std::mutex> lk(mu_);
    auto &fl = free_[dev];
    size_t best = fl.size();
    for (size_t i = 0; i < fl.size(); ++i)
      if (fl[i].second >= bytes && fl[i].second <= 2 * bytes + 4096 &&
          (best == fl.size() || fl[i].second < fl[best].second))
        best = i;
    if (best == fl.size()) return nullptr;
    void *p = fl[best].first;
    *got = fl[best].second;
    held_[dev] -= fl[best].second;
    fl.erase(fl.begin() + best);
    return p;
  }
  void release(int dev, void *p, size_t bytes) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      if (held_[dev] + bytes <= kPoolCapBytes) {
        free_[dev].emplace_back(p, bytes);
        held_[dev] += bytes;
        return;
      }
    }
    (void)hipFree(p);
  }
  void clear() {
    std::lock_guard<std::mutex> lk(mu_);
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto &kv : free_) {
      (void)hipSetDevice(kv.first);
      for (auto &b : kv.second) (void)hipFree(b.first);
      kv.second.clear();
    }
    held_.clear();
    (void)hipSetDevice(cur);
  }

 private:
  std::mutex mu_;
  std::map<int, std::vector<std::pair<void *, size_t>>> free_;
  std::map<int, size_t> held_;
};
DevicePool g_pool;

// Pinned bounce buffers of the D2HPipeline workers.
class PinnedPool {
 public:
  static constexpr size_t kCapBytes = (size_t)256 << 20;  // kept for reuse; more is handed back
  void *acquire(size_t bytes) {
    {
      std::lock_guard<std::mutex> lk(mu_);
      for (size_t i = 0; i < free_.size(); ++i)
        if (free_[i].second >= bytes && free_[i].second <= 2 * bytes + 4096) {
          void *p = free_[i].first;
          held_ -= free_[i].second;
          free_.erase(free_.begin() + i);
          return p;
        }
    }
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lk(mu_);
    cap_[p] = bytes;
    return p;
  }
  void release(void *p) {
    if (!p) return;
    {
      std::lock_guard<std::mutex> lk(mu_);
      const size_t bytes = cap_[p];
      if (held_ + bytes <= kCapBytes) {
        free_.emplace_back(p, bytes);
        held_ += bytes;
        return;
      }
      cap_.erase(p);
    }
    (void)hipHostFree(p);
  }
  void clear() {
    std::lock_guard<std::mutex> lk(mu_);
    for (auto &b : free_) {
      cap_.erase(b.first);
      (void)hipHostFree(b.first);
    }
    free_.clear();
    held_ = 0;
  }

 private:
  std::mutex mu_;
  std::vector<std::pair<void *, size_t>> free_;
  std::map<void *, size_t> cap_;
  size_t held_ = 0;
};
PinnedPool g_pinned;

// Buffers given up by DevBuf::release_after, each with the event behind its last use.
struct Deferred {
  int dev;
  void *p;
  size_t cap;
  hipEvent_t ev;
};
std::mutex g_deferred_mu;
std::vector<Deferred> g_deferred;

// Those whose event has passed go back to the pool; wait: all of them, after their events.
void collect_deferred(bool wait) {
  std::lock_guard<std::mutex> lk(g_deferred_mu);
  size_t keep = 0;
  for (size_t i = 0; i < g_deferred.size(); ++i) {
    const Deferred d = g_deferred[i];
    if (wait) (void)hipEventSynchronize(d.ev);
    if (!wait && hipEventQuery(d.ev) == hipErrorNotReady) {
      (void)hipGetLastError();  // "not ready" is no error of the caller's
      g_deferred[keep++] = d;
      continue;
    }
    (void)hipEventDestroy(d.ev);
    g_pool.release(d.dev, d.p, d.cap);
  }
  g_deferred.resize(keep);
}

}  // namespace

void release_transfer_caches() {
  collect_deferred(true);
  g_pool.clear();
  g_pinned.clear();
}

DevBuf::~DevBuf() {
  if (!p) return;
  (void)hipStreamSynchronize(hipStreamPerThread);
  g_pool.release(dev, p, cap);
}

void DevBuf::release_after(hipStream_t st) {
  if (!p) return;
  hipEvent_t ev = nullptr;
  if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) == hipSuccess && hipEventRecord(ev, st) == hipSuccess) {
    std::lock_guard<std::mutex> lk(g_deferred_mu);
    g_deferred.push_back(Deferred{dev, p, cap, ev});
  } else {
    if (ev) (void)hipEventDestroy(ev);
    (void)hipStreamSynchronize(st);
    g_pool.release(dev, p, cap);
  }
  p = nullptr;
  cap = 0;
}

int DevBuf::alloc(size_t bytes) {
  if (bytes == 0) bytes = 16;
  collect_deferred(false);
  (void)hipGetDevice(&dev);
  p = g_pool.acquire(dev, bytes, &cap);
  if (p) return SPV_OK;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {
    // the cache may be what is exhausting the device: drop it and retry once
    g_pool.clear();
    e = hipMalloc(&p, bytes);
  }
  if (e != hipSuccess) {
    p = nullptr;
    return set_error(SPV_ERR_NOMEM, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  cap = bytes;
  return SPV_OK;
}

HostPrefault::HostPrefault(void *dst, size_t bytes, std::initializer_list<std::pair<const void *, size_t>> inputs) {
  constexpr size_t kMin = (size_t)16 << 20, kPage = 4096;
  if (!dst || bytes < kMin) return;
  const char *lo = static_cast<const char *>(dst), *hi = lo + bytes;
  for (const auto &in : inputs) {
    const char *a = static_cast<const char *>(in.first);
    if (a && a < hi && a + in.second > lo) return;
  }
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  const int T = (int)std::min<size_t>(std::min<unsigned>(8u, hw), bytes / kMin + 1);
  const size_t nblocks = (bytes + kBlock - 1) / kBlock;
  done_.reset(new std::atomic<size_t>[T]);
  for (int i = 0; i < T; ++i) done_[i].store(0, std::memory_order_relaxed);
  nthreads_ = T;
  try {
    for (int i = 0; i < T; ++i)
      threads_.emplace_back([=] {
        volatile char *p = static_cast<volatile char *>(dst);
        size_t mine = 0;
        for (size_t b = (size_t)i; b < nblocks; b += (size_t)T) {
          for (size_t off = b * kBlock; off < std::min(bytes, (b + 1) * kBlock); off += kPage) p[off] = 0;
          done_[i].store(++mine, std::memory_order_release);
        }
        done_[i].store(SIZE_MAX, std::memory_order_release);
      });
  } catch (...) {  // could not start a thread: the copy simply faults the pages itself
  }
  // a thread that never started owns blocks nobody touches: they count as done (the copy into
  // them then faults the pages itself, which is only slower)
  for (int i = (int)threads_.size(); i < T; ++i) done_[i].store(SIZE_MAX, std::memory_order_release);
}

D2HPipeline::D2HPipeline(int dev, const void *d_src, void *h_dst, size_t bytes, size_t chunk_bytes)
    : dev_(dev), src_(static_cast<const char *>(d_src)), dst_(static_cast<char *>(h_dst)), bytes_(bytes),
      chunk_(std::max<size_t>(chunk_bytes, 1)), nchunks_((int)((bytes + chunk_ - 1) / chunk_)),
      events_(nchunks_, nullptr) {
  const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
  workers_ = (int)std::min<size_t>(std::min<unsigned>(6u, hw), std::max<size_t>(1, std::min(chunk_, bytes) >> 20));
  piece_ = round_up((std::min(chunk_, bytes) + workers_ - 1) / workers_, 4096);
  try {
    for (int t = 0; t < workers_; ++t) threads_.emplace_back([this, t] { work(t); });
  } catch (...) {  // fewer workers than planned: the missing slices are copied by finish()
  }
  started_ = (int)threads_.size();
}

void D2HPipeline::work(int t) {
  if (hipSetDevice(dev_) != hipSuccess) return fail(SPV_ERR_HIP, "hipSetDevice", hipGetLastError());
  char *pin[2] = {static_cast<char *>(g_pinned.acquire(piece_)), static_cast<char *>(g_pinned.acquire(piece_))};
  hipEvent_t done[2] = {nullptr, nullptr};
  hipStream_t st = hipStreamPerThread;
  bool ok = pin[0] && pin[1];
  if (!ok) fail(SPV_ERR_NOMEM, "hipHostMalloc", hipErrorOutOfMemory);
  for (int i = 0; ok && i < 2; ++i)
    if (hipEventCreateWithFlags(&done[i], hipEventDisableTiming) != hipSuccess) {
      ok = false;
      fail(SPV_ERR_HIP, "hipEventCreate", hipGetLastError());
    }
  size_t prev_off = 0, prev_len = 0;
  int prev_slot = -1;
  auto drain = [&] {  // the slice whose download is in flight: pinned -> the caller's array
    if (prev_slot < 0) return;
    const hipError_t e = hipEventSynchronize(done[prev_slot]);
    if (e != hipSuccess) {
      ok = false;
      fail(SPV_ERR_HIP, "device-to-host copy", e);
    } else {
      if (prefault_) prefault_->wait_range(prev_off, prev_len);
      memcpy(dst_ + prev_off, pin[prev_slot], prev_len);
    }
    prev_slot = -1;
  };
  for (int k = 0; ok && k < nchunks_; ++k) {
    hipEvent_t ev;
    {
      std::unique_lock<std::mutex> lk(mu_);
      cv_.wait(lk, [&] { return ready_ > k || aborted_; });
      if (aborted_) {
        ok = false;
        break;
      }
      ev = events_[k];
    }
    const size_t c0 = (size_t)k * chunk_, c1 = std::min(bytes_, c0 + chunk_);
    const size_t off = c0 + (size_t)t * piece_;
    if (off >= c1) {
      continue;  // this chunk is shorter than t slices
    }
    const size_t len = std::min(piece_, c1 - off);
    const int slot = k & 1;
    if (prev_slot == slot) drain();  // (a skipped chunk in between) never overwrite an undrained buffer
    if (!ok) break;
    hipError_t e = ev ? hipStreamWaitEvent(st, ev, 0) : hipSuccess;
    if (e == hipSuccess) e = hipMemcpyAsync(pin[slot], src_ + off, len, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(done[slot], st);
    if (e != hipSuccess) {
      ok = false;
      fail(SPV_ERR_HIP, "device-to-host copy", e);
      break;
    }
    drain();  // the previous slice, while this one travels
    prev_off = off;
    prev_len = len;
    prev_slot = slot;
  }
  if (ok) drain();
  (void)hipStreamSynchronize(st);
  for (int i = 0; i < 2; ++i) {
    if (done[i]) (void)hipEventDestroy(done[i]);
    g_pinned.release(pin[i]);
  }
}

int download(int dev, void *h_dst, const void *d_src, size_t bytes, hipStream_t st) {
  if (bytes < D2HPipeline::kMinBytes) {
    SPV_HIP_CHECK(hipMemcpyAsync(h_dst, d_src, bytes, hipMemcpyDeviceToHost, st));
    SPV_HIP_CHECK(hipStreamSynchronize(st));
    return SPV_OK;
  }
  ScopedEvent produced;
  SPV_TRY(produced.record(st));
  const size_t chunk = (size_t)8 << 20;
  D2HPipeline pipe(dev, d_src, h_dst, bytes, chunk);
  const int n = (int)((bytes + chunk - 1) / chunk);
  for (int k = 0; k < n; ++k) pipe.ready(k, produced.ev);
  const int status = pipe.finish();
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return status;
}

}  // namespace spv
