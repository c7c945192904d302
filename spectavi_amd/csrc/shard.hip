// shard.hip -- device selection, and the host-pointer and device-resident calls gathered over RCCL
// (or peer copies) on the first listed GPU (shard.h).

#include "shard.h"
#include "host_io.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

namespace spv {

namespace {
std::mutex g_cfg_mutex;
int g_device = -1;           // -1: not chosen yet
std::vector<int> g_devices;  // empty: not chosen yet
int g_gather_mode = -1;      // -1: SPECTAVI_GATHER, else automatic; SPV_GATHER_DIRECT / SPV_GATHER_RCCL
}  // namespace

void set_device_list(const int *devices, int count) {
  std::lock_guard<std::mutex> lk(g_cfg_mutex);
  g_devices.assign(devices, devices + count);
  g_device = devices[0];
}

void set_gather_mode(int mode) {
  std::lock_guard<std::mutex> lk(g_cfg_mutex);
  g_gather_mode = mode;
}

int use_device(int dev) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0)
    return set_error(SPV_ERR_HIP, "no HIP device available (%s); libspectavi has no CPU fallback",
                     e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (dev < 0 || dev >= count)
    return set_error(SPV_ERR_HIP, "device %d requested but only %d devices are visible", dev, count);
  SPV_HIP_CHECK(hipSetDevice(dev));
  return SPV_OK;
}

std::vector<int> device_list() {
  std::lock_guard<std::mutex> lk(g_cfg_mutex);
  if (g_devices.empty()) {
    const char *e = getenv("SPECTAVI_DEVICES");
    if (e && *e) {
      if (!strcmp(e, "all")) {
        int count = 0;
        if (hipGetDeviceCount(&count) == hipSuccess)
          for (int d = 0; d < count; ++d) g_devices.push_back(d);
      } else {
        for (const char *c = e; *c;) {
          char *end = nullptr;
          const long v = strtol(c, &end, 10);
          if (end == c) break;
          g_devices.push_back((int)v);
          c = (*end == ',') ? end + 1 : end;
        }
      }
    }
    if (g_devices.empty()) {
      if (g_device < 0) {
        const char *d = getenv("SPECTAVI_DEVICE");
        g_device = (d && *d) ? atoi(d) : 0;
      }
      g_devices.push_back(g_device);
    }
  }
  return g_devices;
}

int ensure_device() { return use_device(device_list()[0]); }

// spv_set_gather_mode / SPECTAVI_GATHER choose the transport; left alone, RCCL is used exactly when
// more than one distinct device is configured and a clique over them can be built (north_star's
// "RCCL gather of (idx0, idx1, d0, d1)").  This answers the latter: librccl opened, ncclCommInitAll
// done; both cached, a refusal too, so a box without a usable RCCL pays once.
static bool rccl_clique_usable(const std::vector<int> &devs) {
  static std::mutex mu;
  static std::map<std::vector<int>, bool> known;
  std::lock_guard<std::mutex> lk(mu);
  auto it = known.find(devs);
  if (it != known.end()) return it->second;
  bool ok;
  {
    std::lock_guard<std::mutex> glk(gather_mutex());
    GatherCtx *ctx = nullptr;
    ok = gather_ctx_get(devs, true, &ctx) == SPV_OK;
  }
  if (!ok) {
    fprintf(stderr, "libspectavi: RCCL gather unavailable (%s); sharding with direct copies instead\n", spv_last_error());
    clear_error();
  }
  known[devs] = ok;
  return ok;
}

int gather_transport(const std::vector<int> &devs, long long total) {
  int mode;
  {
    std::lock_guard<std::mutex> lk(g_cfg_mutex);
    mode = g_gather_mode;
  }
  if (mode < 0) {
    const char *e = getenv("SPECTAVI_GATHER");
    if (e && !strcmp(e, "rccl")) mode = SPV_GATHER_RCCL;
    if (e && !strcmp(e, "direct")) mode = SPV_GATHER_DIRECT;
    if (e && !strcmp(e, "copy")) mode = SPV_GATHER_PEERCOPY;
  }
  if (mode >= 0) return mode;  // asked for by name: a failure of that transport is the caller's error
  if (devs.size() < 2) return SPV_GATHER_DIRECT;
  for (size_t a = 0; a < devs.size(); ++a)
    for (size_t b = a + 1; b < devs.size(); ++b)
      if (devs[a] == devs[b]) return SPV_GATHER_DIRECT;  // a clique needs distinct devices
  // the clique a call of `total` rows would use (run_gathered lists no more ranks than rows)
  const size_t G = total < 0 ? devs.size() : (size_t)std::min<long long>((long long)devs.size(), std::max<long long>(total, 1));
  if (!rccl_clique_usable(std::vector<int>(devs.begin(), devs.begin() + G))) return SPV_GATHER_DIRECT;
  return SPV_GATHER_RCCL;
}

namespace {

// Device buffers of one shard (or of the root), alive until every stream of the call has drained.
struct BufList {
  std::vector<std::unique_ptr<DevBuf>> v;
  template <typename T>
  int add(size_t bytes, T **out) {
    v.emplace_back(new DevBuf);
    SPV_TRY(v.back()->alloc(bytes));
    *out = v.back()->as<T>();
    return SPV_OK;
  }
  // a new buffer holding the host array src, its copy queued on st
  template <typename T>
  int upload(const T *src, size_t bytes, hipStream_t st, const T **out) {
    T *p = nullptr;
    SPV_TRY(add(bytes, &p));
    *out = p;
    return v.back()->copy_in(src, bytes, st);
  }
};

// total rows over the listed devices: rank r runs `produce` on a host thread of its own (device
// devs[r] current, work enqueued on the clique's stream r) and leaves its rows, row_bytes[k] each,
// in K send buffers of max_cnt rows; the calling thread then gathers each of the K buffers on rank 0
// with one ncclGather per rank (gather.hip) and runs `consume` on the root: recv[k] holds
// [G][max_cnt] rows in rank order.  Everything is synchronised before the buffers are released.
template <typename Produce, typename Consume>
int run_gathered(const std::vector<int> &all_devs, long long total, const std::vector<size_t> &row_bytes,
                 Produce produce, Consume consume, int transport) {
  const int G = (int)std::min<long long>((long long)all_devs.size(), std::max<long long>(total, 1));
  const std::vector<int> devs(all_devs.begin(), all_devs.begin() + G);
  const size_t K = row_bytes.size();
  // (decided before the clique lock is taken: the automatic rule may itself build a clique under it)
  const bool want_rccl = (transport == SPV_GATHER_AUTO ? gather_transport(all_devs, total) : transport) == SPV_GATHER_RCCL;
  std::lock_guard<std::mutex> lk(gather_mutex());  // one clique user at a time
  for (int d : devs) SPV_TRY(use_device(d));         // fail early on a bad device number
  GatherCtx *ctx = nullptr;
  SPV_TRY(gather_ctx_get(devs, want_rccl, &ctx));
  const long long max_cnt = shard_lo(total, G, 1);   // = size of shard 0, the largest
  std::vector<BufList> bufs(G + 1);                  // [G] = the root's receive / staging buffers
  std::vector<std::vector<const void *>> send(K, std::vector<const void *>(G, nullptr));
  int st = run_ranks(devs, G, [&](int r) {
    SPV_TRY(use_device(devs[r]));
    std::vector<const void *> mine(K, nullptr);
    const int s = produce(r, shard_lo(total, G, r), shard_lo(total, G, r + 1), max_cnt, gather_stream(ctx, r),
                          bufs[r], mine);
    for (size_t k = 0; k < K; ++k) send[k][r] = mine[k];
    return s;
  });
  std::vector<const void *> recv(K, nullptr);
  if (st == SPV_OK) st = use_device(devs[0]);
  for (size_t k = 0; k < K && st == SPV_OK; ++k) {
    void *rb = nullptr;
    st = bufs[G].add((size_t)G * max_cnt * row_bytes[k], &rb);
    if (st == SPV_OK) {
      recv[k] = rb;
      st = gather_bytes_run(ctx, send[k], rb, (size_t)max_cnt * row_bytes[k]);
    }
  }
  if (st == SPV_OK) st = use_device(devs[0]);
  if (st == SPV_OK) st = consume(recv, G, max_cnt, gather_stream(ctx, 0), bufs[G]);
  // drain every rank's stream before its buffers go back to the pool, error or not
  for (int r = 0; r < G; ++r)
    if (hipSetDevice(devs[r]) == hipSuccess) {
      const hipError_t e = hipStreamSynchronize(gather_stream(ctx, r));
      if (e != hipSuccess && st == SPV_OK)
        st = set_error(SPV_ERR_HIP, "device %d: %s", devs[r], hipGetErrorString(e));
    }
  return st;
}

// The gathered [G][max_cnt] rows of row_bytes each -> their slices of the `total` rows at dst: rank
// r's segment is its first shard_lo(r + 1) - shard_lo(r) rows.
int copy_shard_segments(void *dst, const void *recv, long long total, int G, long long max_cnt, size_t row_bytes,
                        hipMemcpyKind kind, hipStream_t st) {
  for (int r = 0; r < G; ++r) {
    const long long lo = shard_lo(total, G, r), hi = shard_lo(total, G, r + 1);
    SPV_HIP_CHECK(hipMemcpyAsync(static_cast<char *>(dst) + (size_t)lo * row_bytes,
                                 static_cast<const char *>(recv) + (size_t)r * max_cnt * row_bytes,
                                 (size_t)(hi - lo) * row_bytes, kind, st));
  }
  return SPV_OK;
}

// The gathered records -> idx uint64[total,2] and the 32-bit d32[total,2].  touch == nullptr: device
// arrays on the root, written by the widening kernel itself; otherwise the caller's host arrays (touch
// pre-faults idx), reached through scratch on the root.
int widen_records(const void *recv, long long total, int G, long long max_cnt, uint64_t *idx, void *d32,
                  HostPrefault *touch, hipStream_t st, BufList &b) {
  if (!touch) return gather_widen_run(recv, total, G, max_cnt, idx, d32, st);
  uint64_t *di = nullptr;
  void *dd = nullptr;
  SPV_TRY(b.add((size_t)total * 2 * sizeof(uint64_t), &di));
  SPV_TRY(b.add((size_t)total * 2 * 4, &dd));
  SPV_TRY(gather_widen_run(recv, total, G, max_cnt, di, dd, st));
  touch->wait();
  SPV_HIP_CHECK(hipMemcpyAsync(idx, di, (size_t)total * 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  SPV_HIP_CHECK(hipMemcpyAsync(d32, dd, (size_t)total * 2 * 4, hipMemcpyDeviceToHost, st));
  return SPV_OK;
}

hipMemcpyKind to_output(const HostPrefault *touch) { return touch ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice; }

// Rank r's elements [lo, lo + n) of an input: the caller's resident in.dev[r] as it is, or the rows of
// its host array staged into a buffer of b on st.
template <typename T>
int rank_input(const GatherInput<T> &in, int r, size_t lo, size_t n, hipStream_t st, BufList &b, const T **out) {
  if (in.dev) {
    *out = in.dev[r];
    return SPV_OK;
  }
  return b.upload(in.host + lo, n * sizeof(T), st, out);
}

}  // namespace

// One gathered core per op.  Host form: the result arrays start pre-faulting before the ranks start
// (HostPrefault does nothing for the null array of the device form), and `touch` is handed to the
// consumer, which waits for it before its first device-to-host copy.
int l1k2_gathered(const std::vector<int> &devs, GatherInput<uint8_t> x, GatherInput<uint8_t> y, int xrows,
                  long long yrows, int dim, uint64_t *idx, int32_t *dist, int transport) {
  const size_t xb = (size_t)xrows * dim;
  HostPrefault touch(y.dev ? nullptr : idx, (size_t)yrows * 2 * sizeof(uint64_t), {{x.host, xb}, {y.host, (size_t)yrows * dim}});
  auto produce = [&](int r, long long lo, long long hi, long long max_cnt, hipStream_t st, BufList &b,
                     std::vector<const void *> &send) {
    const int cnt = (int)(hi - lo);
    const uint8_t *dx = nullptr, *dy = nullptr;
    SPV_TRY(rank_input(x, r, 0, xb, st, b, &dx));
    SPV_TRY(rank_input(y, r, (size_t)lo * dim, (size_t)cnt * dim, st, b, &dy));
    const size_t wsb = spv_l1k2_workspace_bytes(xrows, cnt, dim);
    uint64_t *di = nullptr;
    int32_t *dd = nullptr;
    void *ws = nullptr, *rec = nullptr;
    SPV_TRY(b.add((size_t)cnt * 2 * sizeof(uint64_t), &di));
    SPV_TRY(b.add((size_t)cnt * 2 * sizeof(int32_t), &dd));
    SPV_TRY(b.add(wsb, &ws));
    SPV_TRY(b.add((size_t)max_cnt * sizeof(Record), &rec));
    SPV_TRY(l1k2_run(dx, dy, xrows, cnt, dim, di, dd, ws, wsb, st));
    SPV_TRY(gather_pack_run(di, dd, cnt, rec, st));
    send[0] = rec;
    return SPV_OK;
  };
  auto consume = [&](const std::vector<const void *> &recv, int G, long long max_cnt, hipStream_t st, BufList &b) {
    return widen_records(recv[0], yrows, G, max_cnt, idx, dist, y.dev ? nullptr : &touch, st, b);
  };
  return run_gathered(devs, yrows, {sizeof(Record)}, produce, consume, transport);
}

// Every rank holds a replica of the database and of the hyperplanes and rebuilds identical codes and
// bucket tables; ncand (may be NULL) travels as a second gathered buffer.
int cascade_gathered(const std::vector<int> &devs, GatherInput<float> x, GatherInput<float> y, GatherInput<float> dict,
                     int xrows, long long yrows, int dim, int m, int n, int g, uint64_t *idx, float *dist,
                     int32_t *ncand, int transport) {
  const size_t xn = (size_t)xrows * dim;
  HostPrefault touch(y.dev ? nullptr : idx, (size_t)yrows * 2 * sizeof(uint64_t),
                     {{x.host, xn * sizeof(float)}, {y.host, (size_t)yrows * dim * sizeof(float)}});
  auto produce = [&](int r, long long lo, long long hi, long long max_cnt, hipStream_t st, BufList &b,
                     std::vector<const void *> &send) {
    const int cnt = (int)(hi - lo);
    const float *dx = nullptr, *dy = nullptr, *dd = nullptr;
    SPV_TRY(rank_input(x, r, 0, xn, st, b, &dx));
    SPV_TRY(rank_input(y, r, (size_t)lo * dim, (size_t)cnt * dim, st, b, &dy));
    SPV_TRY(rank_input(dict, r, 0, (size_t)n * dim * m, st, b, &dd));
    const size_t wsb = cascade_workspace_bytes(xrows, cnt, dim, m, n, g);
    uint64_t *di = nullptr;
    float *dds = nullptr;
    int32_t *dn = nullptr;
    void *ws = nullptr, *rec = nullptr;
    SPV_TRY(b.add((size_t)cnt * 2 * sizeof(uint64_t), &di));
    SPV_TRY(b.add((size_t)cnt * 2 * sizeof(float), &dds));
    SPV_TRY(b.add((size_t)max_cnt * sizeof(int32_t), &dn));
    SPV_TRY(b.add(wsb, &ws));
    SPV_TRY(b.add((size_t)max_cnt * sizeof(Record), &rec));
    SPV_TRY(cascade_run(dx, dy, xrows, cnt, dim, m, n, g, dd, di, dds, ncand ? dn : nullptr, ws, wsb, st));
    SPV_TRY(gather_pack_run(di, dds, cnt, rec, st));  // float32 distances as their bits
    send[0] = rec;
    if (ncand) send[1] = dn;
    return SPV_OK;
  };
  auto consume = [&](const std::vector<const void *> &recv, int G, long long max_cnt, hipStream_t st, BufList &b) {
    HostPrefault *host = y.dev ? nullptr : &touch;
    SPV_TRY(widen_records(recv[0], yrows, G, max_cnt, idx, dist, host, st, b));
    if (!ncand) return SPV_OK;
    return copy_shard_segments(ncand, recv[1], yrows, G, max_cnt, sizeof(int32_t), to_output(host), st);
  };
  std::vector<size_t> rows = {sizeof(Record)};
  if (ncand) rows.push_back(sizeof(int32_t));
  return run_gathered(devs, yrows, rows, produce, consume, transport);
}

// The rows travel already in the ABI layout (32 or 8 bytes per point).
int dlt_gathered(const std::vector<int> &devs, const double *P0, const double *P1, GatherInput<double> x,
                 GatherInput<double> xp, long long npt, double *dst, bool want_error, int transport) {
  const size_t row = (want_error ? 1 : 4) * sizeof(double);
  HostPrefault touch(x.dev ? nullptr : dst, (size_t)npt * row, {{x.host, (size_t)npt * 24}, {xp.host, (size_t)npt * 24}});
  auto produce = [&](int r, long long lo, long long hi, long long max_cnt, hipStream_t st, BufList &b,
                     std::vector<const void *> &send) {
    const double *dx = nullptr, *dxp = nullptr;
    double *dd = nullptr;
    SPV_TRY(rank_input(x, r, (size_t)lo * 3, (size_t)(hi - lo) * 3, st, b, &dx));
    SPV_TRY(rank_input(xp, r, (size_t)lo * 3, (size_t)(hi - lo) * 3, st, b, &dxp));
    SPV_TRY(b.add((size_t)max_cnt * row, &dd));
    SPV_TRY(dlt_run(P0, P1, hi - lo, dx, dxp, dd, want_error, st));
    send[0] = dd;
    return SPV_OK;
  };
  auto consume = [&](const std::vector<const void *> &recv, int G, long long max_cnt, hipStream_t st, BufList &) {
    HostPrefault *host = x.dev ? nullptr : &touch;
    if (host) host->wait();
    return copy_shard_segments(dst, recv[0], npt, G, max_cnt, row, to_output(host), st);
  };
  return run_gathered(devs, npt, {row}, produce, consume, transport);
}

}  // namespace spv
