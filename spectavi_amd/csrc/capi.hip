// capi.hip -- extern "C" surface of libspectavi.so (declared in include/spectavi_amd.h).
//
// Host-pointer entry points own the H2D/D2H traffic and scratch allocation and
// call the same device-pointer runners (l1k2_run / cascade_run / dlt_run) the
// section-3 symbols expose.  No compute happens on the host and there is no
// CPU fallback: every path ends in a HIP kernel launch or in an error status.
// The transfer machinery is in host_io.hip, device selection and the gathered
// multi-device forms in shard.hip.

#include "common.h"
#include "host_io.h"
#include "records.h"
#include "shard.h"

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <string>

namespace spv {

namespace {
thread_local int g_status = SPV_OK;
thread_local char g_message[512] = "";

std::mutex g_seed_mutex;
bool g_seed_fixed = false;
uint32_t g_seed = 0;
}  // namespace

int set_error(int status, const char *fmt, ...) {
  g_status = status;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_message, sizeof(g_message), fmt, ap);
  va_end(ap);
  return status;
}

void clear_error() {
  g_status = SPV_OK;
  g_message[0] = '\0';
}

// ---- optional kernel timing ----------------------------------------------------------
namespace {
std::mutex g_prof_mutex;
std::atomic<bool> g_prof_on{false};
// Per kernel name: running totals of the launches whose events have completed, and the event
// pairs still in flight.  Completed pairs are folded into the totals (and their events destroyed)
// whenever the pending list grows past kProfFoldAt, when profiling is switched off, and on every
// read, so a long-running caller that leaves profiling enabled holds a bounded number of events.
struct ProfEntry {
  long long launches = 0;
  double total_ms = 0.0;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};
std::map<std::string, ProfEntry> g_prof;
constexpr size_t kProfFoldAt = 64;

// g_prof_mutex held.  wait = true: block on every pending pair; false: fold only finished ones.
void prof_fold(ProfEntry &e, bool wait) {
  size_t keep = 0;
  for (auto &ev : e.pending) {
    const hipError_t q = wait ? hipEventSynchronize(ev.second) : hipEventQuery(ev.second);
    if (q == hipSuccess) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) {
        e.total_ms += ms;
        e.launches += 1;
      }
    } else if (q == hipErrorNotReady) {
      e.pending[keep++] = ev;
      continue;
    }
    (void)hipEventDestroy(ev.first);
    (void)hipEventDestroy(ev.second);
  }
  e.pending.resize(keep);
}
}  // namespace

ProfScope::ProfScope(const char *name, hipStream_t stream) : name_(name), stream_(stream) {
  if (!g_prof_on.load(std::memory_order_relaxed)) return;
  if (hipEventCreate(&start_) != hipSuccess) {
    start_ = nullptr;
    return;
  }
  (void)hipEventRecord(start_, stream_);
}

ProfScope::~ProfScope() {
  if (!start_) return;
  hipEvent_t stop = nullptr;
  if (hipEventCreate(&stop) != hipSuccess) {
    (void)hipEventDestroy(start_);
    return;
  }
  (void)hipEventRecord(stop, stream_);
  std::lock_guard<std::mutex> lk(g_prof_mutex);
  ProfEntry &e = g_prof[name_];
  e.pending.emplace_back(start_, stop);
  if (e.pending.size() >= kProfFoldAt) prof_fold(e, false);
}

// The host-pointer entry points select their device(s) with hipSetDevice on the caller's thread
// (and on their own shard threads).  The caller's current device is part of ITS state -- a
// framework's tensors and streams hang off it -- so every such entry point restores it on exit.
struct DeviceRestore {
  int prev = -1;
  DeviceRestore() {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
  }
  ~DeviceRestore() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceRestore(const DeviceRestore &) = delete;
  DeviceRestore &operator=(const DeviceRestore &) = delete;
};

// guard() for entry points that may switch the current device.
template <typename Fn>
static int host_guard(Fn fn) {
  DeviceRestore restore;
  return guard(fn);
}

// The prologue of every exported entry point: a fresh status, then the body under guard() (api) or,
// when the body may switch the current device, host_guard() (host_api).
template <typename Fn>
static int api(Fn fn) {
  clear_error();
  return guard(fn);
}
template <typename Fn>
static int host_api(Fn fn) {
  clear_error();
  return host_guard(fn);
}

// What a *_batch_plan entry hands out of its items: the first min(n, items_cap) of them, as rows of N int32 columns,
// where the caller wants them (items_cap >= 0 is the entry's own rule).
template <int N, typename Item>
static void export_items(const std::vector<Item> &its, int32_t *items, long long items_cap) {
  static_assert(sizeof(Item) == N * sizeof(int32_t), "an item is N int32 columns");
  if (items) memcpy(items, its.data(), (size_t)std::min<long long>(items_cap, (long long)its.size()) * sizeof(Item));
}

// The body of a many-sets fit's *_fit_batch_plan entry behind its argument check: the first round's sets, tries
// (per_try candidates each), work items and blocks of 256 rows.
static int fit_batch_plan(void (*first_round)(const long long *, int, int, std::vector<RansacBatchSlot> *), int per_try,
                          const long long *off, int nsets, int maximum_tries, int compute_units, long long out[4],
                          int32_t *items, long long items_cap) {
  if (compute_units < 1 || !out || items_cap < 0) return set_error(SPV_ERR_INVALID, "bad arguments");
  std::vector<RansacBatchSlot> slots;
  std::vector<RansacBatchItem> its;
  first_round(off, nsets, maximum_tries, &slots);
  ransac_batch_items(slots, off, compute_units, &its);
  long long tries = 0, blocks = 0;
  for (const RansacBatchSlot &s : slots) {
    tries += s.ncand / per_try;
    blocks += (s.npt + 255) / 256;
  }
  out[0] = (long long)slots.size();
  out[1] = tries;
  out[2] = (long long)its.size();
  out[3] = blocks;
  export_items<5>(its, items, items_cap);
  return SPV_OK;
}

// The body of a *_batch_workspace_bytes query: the bytes of the plan `make` fills, or 0 where it refuses the
// arguments, with no error left behind.
template <typename Plan, typename Base, typename Fn>
static size_t plan_bytes(size_t Base::*bytes, Fn make) {
  Plan p;
  const int st = guard([&] { return make(&p); });
  if (st != SPV_OK) clear_error();
  return st == SPV_OK ? p.*bytes : 0;
}

int device_cu_count() {
  static std::atomic<int> cache[64];  // per device, 0 = not asked yet
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  int cus = (dev >= 0 && dev < 64) ? cache[dev].load(std::memory_order_relaxed) : 0;
  if (cus <= 0) {
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) return 1;
    if (dev >= 0 && dev < 64) cache[dev].store(cus, std::memory_order_relaxed);
  }
  return cus;
}

// ---- argument rules -------------------------------------------------------------------
// The row width of the L1 and cascade paths.  *_ok: the rule alone, which the workspace-size queries
// use without touching the thread's last error; check_*: the rule with its message.
static bool dim_ok(int dim) { return dim > 0 && dim % 16 == 0; }
static bool l1k2_shape_ok(int xrows, int yrows, int dim) { return xrows >= 0 && yrows >= 0 && dim_ok(dim); }
// (g up to m: the size query has never applied check_cascade_args' g <= 16)
static bool cascade_shape_ok(int xrows, int yrows, int dim, int m, int n, int g) {
  return l1k2_shape_ok(xrows, yrows, dim) && m >= 1 && m <= 31 && n >= 1 && g >= 0 && g <= m;
}

static int check_dim(int dim) {
  if (!dim_ok(dim))
    return set_error(SPV_ERR_INVALID, "Input matrix inner dimensions must be 16-byte aligned (dim=%d).", dim);
  return SPV_OK;
}

static int check_l1k2_args(const uint8_t *x, const uint8_t *y, int xrows, int yrows, int dim,
                           const uint64_t *idx, const int32_t *dist) {
  if (xrows < 0 || yrows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
  SPV_TRY(check_dim(dim));
  if (yrows > 0 && (!y || !idx || !dist || (xrows > 0 && !x))) return set_error(SPV_ERR_INVALID, "null pointer");
  return SPV_OK;
}

static int check_cascade_args(int xrows, int yrows, int dim, int m, int n, int g) {
  if (xrows < 0 || yrows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
  SPV_TRY(check_dim(dim));
  if (m < 1 || m > 31) return set_error(SPV_ERR_INVALID, "hash_bit_rate m=%d must be in [1,31]", m);
  if (n < 1) return set_error(SPV_ERR_INVALID, "num_hash_tables n=%d must be >= 1", n);
  if (g < 0 || g > m || g > 16)
    return set_error(SPV_ERR_INVALID, "num_candidate_neighbours g=%d must be in [0,min(m,16)]", g);
  return SPV_OK;
}

static int check_gathered_devices(int ndev, const int *devices, int transport) {
  if (ndev < 1 || ndev > 64 || !devices) return set_error(SPV_ERR_INVALID, "bad device list");
  if (transport != SPV_GATHER_RCCL && transport != SPV_GATHER_PEERCOPY)
    return set_error(SPV_ERR_INVALID, "transport must be SPV_GATHER_RCCL or SPV_GATHER_PEERCOPY");
  return SPV_OK;
}

namespace {

// ---- single-device host-pointer bodies ---------------------------------------------------
// Their prologue: makes `dev` current and names the stream their work is queued on.
int host_begin(int dev, hipStream_t *st) {
  *st = hipStreamPerThread;  // concurrent callers (ctypes drops the GIL) do not serialise on the null stream
  return use_device(dev);
}

// The L1, cascade and DLT bodies are bound by the PCIe link: the result arrays
// start pre-faulting first, every buffer is allocated before the first copy is queued, and the
// pre-faulting has ended before the first device-to-host copy.
int host_l1k2_one(int dev, const uint8_t *x, const uint8_t *y, int xrows, int yrows, int dim,
                  uint64_t *idx, int32_t *dist) {
  SPV_TRY(check_l1k2_args(x, y, xrows, yrows, dim, idx, dist));
  if (yrows == 0) return SPV_OK;
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t xb = (size_t)xrows * dim, yb = (size_t)yrows * dim;
  const size_t ib = (size_t)yrows * 2 * sizeof(uint64_t), db = (size_t)yrows * 2 * sizeof(int32_t);
  const size_t wsb = spv_l1k2_workspace_bytes(xrows, yrows, dim);
  HostPrefault touch_idx(idx, ib, {{x, xb}, {y, yb}});
  HostPrefault touch_dist(dist, db, {{x, xb}, {y, yb}});
  DevBuf dx, dy, di, dd, ws;
  SPV_TRY(alloc_all({{&dx, xb}, {&dy, yb}, {&di, ib}, {&dd, db}, {&ws, wsb}}));
  SPV_TRY(dx.copy_in(x, xb, st));
  SPV_TRY(dy.copy_in(y, yb, st));
  SPV_TRY(l1k2_run(dx.as<uint8_t>(), dy.as<uint8_t>(), xrows, yrows, dim, di.as<uint64_t>(),
                   dd.as<int32_t>(), ws.p, wsb, st));
  touch_idx.wait();
  touch_dist.wait();
  SPV_TRY(dd.copy_out(dist, db, st));
  return download(dev, idx, di.p, ib, st);
}

int host_l1k2(const uint8_t *x, const uint8_t *y, int xrows, int yrows, int dim, uint64_t *idx,
              int32_t *dist) {
  if (yrows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
  const std::vector<int> devs = device_list();
  if (yrows > 0 && gather_transport(devs, yrows) != SPV_GATHER_DIRECT) {
    SPV_TRY(check_l1k2_args(x, y, xrows, yrows, dim, idx, dist));
    return l1k2_gathered(devs, {x, nullptr}, {y, nullptr}, xrows, yrows, dim, idx, dist, SPV_GATHER_AUTO);
  }
  return run_sharded(yrows, [&](int dev, long long lo, long long hi) {
    return host_l1k2_one(dev, x, y ? y + (size_t)lo * dim : y, xrows, (int)(hi - lo), dim,
                         idx ? idx + 2 * lo : idx, dist ? dist + 2 * lo : dist);
  });
}

// The many-pairs L1 2-NN through host pointers, on the first selected device (no sharding): the whole of desc up,
// one l1k2_batch_run, both results back.
int host_l1k2_batch(const uint8_t *desc, const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs,
                    uint64_t *idx, int32_t *dist) {
  L1K2BatchPlan p;
  SPV_TRY(l1k2_batch_plan(seg_off, nseg, dim, pairs, npairs, &p));
  if (p.out_rows == 0) return SPV_OK;
  if (!desc || !idx || !dist) return set_error(SPV_ERR_INVALID, "null pointer");
  const int dev = device_list()[0];
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t xb = (size_t)p.total_rows * dim;
  const size_t ib = (size_t)p.out_rows * 2 * sizeof(uint64_t), db = (size_t)p.out_rows * 2 * sizeof(int32_t);
  HostPrefault touch_idx(idx, ib, {{desc, xb}});
  HostPrefault touch_dist(dist, db, {{desc, xb}});
  DevBuf dx, di, dd, ws;
  SPV_TRY(alloc_all({{&dx, xb}, {&di, ib}, {&dd, db}, {&ws, p.total_bytes}}));
  SPV_TRY(dx.copy_in(desc, xb, st));
  SPV_TRY(l1k2_batch_run(dx.as<uint8_t>(), seg_off, nseg, dim, pairs, npairs, di.as<uint64_t>(), dd.as<int32_t>(), ws.p,
                         p.total_bytes, st));
  touch_idx.wait();
  touch_dist.wait();
  SPV_TRY(dd.copy_out(dist, db, st));
  return download(dev, idx, di.p, ib, st);
}

// The guided many-pairs L1 2-NN through host pointers, on the first selected device: desc, geom and lines up, one
// l1k2_guided_run, the results back.
int host_l1k2_guided_batch(const uint8_t *desc, const float *geom, const long long *seg_off, int nseg, int dim,
                           const int32_t *pairs, int npairs, const double *lines, double max_dist, uint64_t *idx,
                           int32_t *dist, int32_t *ncand) {
  L1K2GuidedPlan p;
  SPV_TRY(l1k2_guided_plan(seg_off, nseg, dim, pairs, npairs, &p));
  if (p.out_rows == 0) return SPV_OK;
  if (!desc || !geom || !lines || !idx || !dist) return set_error(SPV_ERR_INVALID, "null pointer");
  const int dev = device_list()[0];
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t xb = (size_t)p.total_rows * dim, gb = (size_t)p.total_rows * 4 * sizeof(float);
  const size_t lb = (size_t)p.out_rows * 3 * sizeof(double), nb = ncand ? (size_t)p.out_rows * sizeof(int32_t) : 0;
  const size_t ib = (size_t)p.out_rows * 2 * sizeof(uint64_t), db = (size_t)p.out_rows * 2 * sizeof(int32_t);
  DevBuf dx, dg, dl, di, dd, dn, ws;
  SPV_TRY(alloc_all({{&dx, xb}, {&dg, gb}, {&dl, lb}, {&di, ib}, {&dd, db}, {&dn, nb}, {&ws, p.total_bytes}}));
  SPV_TRY(dx.copy_in(desc, xb, st));
  SPV_TRY(dg.copy_in(geom, gb, st));
  SPV_TRY(dl.copy_in(lines, lb, st));
  SPV_TRY(l1k2_guided_run(dx.as<uint8_t>(), dg.as<float>(), seg_off, nseg, dim, pairs, npairs, dl.as<double>(), max_dist,
                          di.as<uint64_t>(), dd.as<int32_t>(), ncand ? dn.as<int32_t>() : nullptr, ws.p, p.total_bytes, st));
  SPV_TRY(dd.copy_out(dist, db, st));
  SPV_TRY(dn.copy_out(ncand, nb, st));
  return download(dev, idx, di.p, ib, st);
}

// The tracks of a collection through host pointers, on the first selected device: matches, mask and (continuing)
// label up, one tracks_batch_run, the counts back, then as much of every output as the counts say.  A collection
// without a row touches no device.
int host_tracks_batch(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const int32_t *matches, int count,
                      const uint8_t *mask, int min_len, int accumulate, int32_t *label, int32_t *track, long long *track_off,
                      int32_t *members, uint8_t *flags, int32_t *counts) {
  SPV_TRY(tracks_batch_check(seg_off, nseg, pairs, npairs, count, min_len));
  const long long n = seg_off[nseg];
  const long long bound = tracks_batch_member_bound(n, count, accumulate);
  if (!counts || !track_off || (n > 0 && (!label || !track)) || (count > 0 && !matches) || (bound > 0 && !members) ||
      (bound > 1 && !flags))
    return set_error(SPV_ERR_INVALID, "null pointer");
  counts[0] = counts[1] = 0;
  track_off[0] = 0;
  if (n == 0) return SPV_OK;
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t mb = (size_t)count * 2 * sizeof(int32_t), kb = mask ? (size_t)count : 0, lb = (size_t)n * sizeof(int32_t);
  const size_t wsb = tracks_batch_workspace_bytes(n, count);
  const int32_t cnt = count;
  DevBuf dm, dk, dc, dl, dt, doff, dmem, df, dn, ws;
  SPV_TRY(alloc_all({{&dm, mb}, {&dk, kb}, {&dc, sizeof(int32_t)}, {&dl, lb}, {&dt, lb},
                     {&doff, (size_t)(bound / 2 + 1) * sizeof(long long)}, {&dmem, (size_t)bound * 2 * sizeof(int32_t)},
                     {&df, (size_t)(bound / 2)}, {&dn, 2 * sizeof(int32_t)}, {&ws, wsb}}));
  SPV_TRY(dm.copy_in(matches, mb, st));
  SPV_TRY(dk.copy_in(mask, kb, st));
  SPV_TRY(dc.copy_in(&cnt, sizeof(int32_t), st));
  if (accumulate) SPV_TRY(dl.copy_in(label, lb, st));
  SPV_TRY(tracks_batch_run(seg_off, nseg, pairs, npairs, dm.as<int32_t>(), dc.as<int32_t>(), count,
                           mask ? dk.as<uint8_t>() : nullptr, min_len, accumulate, dl.as<int32_t>(), dt.as<int32_t>(),
                           doff.as<long long>(), dmem.as<int32_t>(), df.as<uint8_t>(), dn.as<int32_t>(), ws.p, wsb, st));
  SPV_TRY(dn.copy_out(counts, 2 * sizeof(int32_t), st));
  SPV_TRY(dl.copy_out(label, lb, st));
  SPV_TRY(dt.copy_out(track, lb, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  SPV_TRY(doff.copy_out(track_off, (size_t)(counts[0] + 1) * sizeof(long long), st));
  SPV_TRY(dmem.copy_out(members, (size_t)counts[1] * 2 * sizeof(int32_t), st));
  SPV_TRY(df.copy_out(flags, (size_t)counts[0], st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

// The N-view triangulation of tracks through host pointers, on the first selected device: geom and the members up,
// one tracks_triangulate_run, the four results back.  A call without a track touches no device.
int host_tracks_triangulate(const float *geom, const long long *seg_off, int nseg, const double *cams, const int32_t *use_set,
                            const long long *track_off, int ntracks, const int32_t *members, long long nmembers,
                            double max_error, double *X, double *err, uint8_t *ok, int32_t *nused) {
  SPV_TRY(tracks_triangulate_check(geom, seg_off, nseg, cams, track_off, ntracks, members, nmembers, max_error, X, err, ok, nused));
  if (ntracks == 0) return SPV_OK;
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t gb = (size_t)seg_off[nseg] * 4 * sizeof(float), mb = (size_t)nmembers * 2 * sizeof(int32_t);
  const size_t nt = (size_t)ntracks, nm = (size_t)nmembers;
  DevBuf dg, dm, dX, de, dk, dn;
  SPV_TRY(alloc_all({{&dg, gb}, {&dm, mb}, {&dX, nt * 4 * sizeof(double)}, {&de, err ? nm * sizeof(double) : 0},
                     {&dk, ok ? nt : 0}, {&dn, nused ? nt * sizeof(int32_t) : 0}}));
  SPV_TRY(dg.copy_in(geom, gb, st));
  SPV_TRY(dm.copy_in(members, mb, st));
  SPV_TRY(tracks_triangulate_run(dg.as<float>(), seg_off, nseg, cams, use_set, track_off, ntracks, dm.as<int32_t>(), nmembers,
                                 max_error, dX.as<double>(), err ? de.as<double>() : nullptr, ok ? dk.as<uint8_t>() : nullptr,
                                 nused ? dn.as<int32_t>() : nullptr, st));
  SPV_TRY(dX.copy_out(X, nt * 4 * sizeof(double), st));
  if (err) SPV_TRY(de.copy_out(err, nm * sizeof(double), st));
  if (ok) SPV_TRY(dk.copy_out(ok, nt, st));
  if (nused) SPV_TRY(dn.copy_out(nused, nt * sizeof(int32_t), st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

// Bundle adjustment through host pointers, on the first selected device: geom, the members, X and use up, one
// bundle_adjust_run in a workspace of its own, X, err and active back.  A call without a track or without a camera
// touches no device.
int host_bundle_adjust(const float *geom, const long long *seg_off, int nseg, const double *K, double *poses, const int32_t *mode,
                       const long long *track_off, int ntracks, const int32_t *members, long long nmembers, double *X,
                       const uint8_t *use, const BundleAdjustOptions &o, double *err, uint8_t *active, double *trace, double *info) {
  SPV_TRY(bundle_adjust_check(geom, seg_off, nseg, K, poses, mode, track_off, ntracks, members, nmembers, X, o, err, trace, info));
  if (!bundle_adjust_has_work(mode, nseg, ntracks)) {
    bundle_adjust_idle(o, trace, info);
    if (active) memset(active, 0, (size_t)ntracks);
    if (err)
      for (long long i = 0; i < nmembers; ++i) err[i] = __builtin_nan("");
    return SPV_OK;
  }
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t gb = (size_t)seg_off[nseg] * 4 * sizeof(float), mb = (size_t)nmembers * 2 * sizeof(int32_t);
  const size_t nt = (size_t)ntracks, nm = (size_t)nmembers, wsb = bundle_adjust_workspace_bytes(nseg, ntracks, nmembers);
  DevBuf dg, dm, dX, du, de, da, ws;
  SPV_TRY(alloc_all({{&dg, gb}, {&dm, mb}, {&dX, nt * 4 * sizeof(double)}, {&du, use ? nt : 0}, {&de, err ? nm * sizeof(double) : 0},
                     {&da, active ? nt : 0}, {&ws, wsb}}));
  SPV_TRY(dg.copy_in(geom, gb, st));
  SPV_TRY(dm.copy_in(members, mb, st));
  SPV_TRY(dX.copy_in(X, nt * 4 * sizeof(double), st));
  if (use) SPV_TRY(du.copy_in(use, nt, st));
  SPV_TRY(bundle_adjust_run(dg.as<float>(), seg_off, nseg, K, poses, mode, track_off, ntracks, dm.as<int32_t>(), nmembers,
                            dX.as<double>(), use ? du.as<uint8_t>() : nullptr, o, err ? de.as<double>() : nullptr,
                            active ? da.as<uint8_t>() : nullptr, trace, info, ws.p, wsb, st));
  SPV_TRY(dX.copy_out(X, nt * 4 * sizeof(double), st));
  if (err) SPV_TRY(de.copy_out(err, nm * sizeof(double), st));
  if (active) SPV_TRY(da.copy_out(active, nt, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

// The many-sets RANSAC through host pointers, on the first selected device: both arrays up, one
// ransac_fit_batch_run.  A collection in which no set runs touches no device.
int host_ransac_fit_batch(const double *x0, const double *x1, const long long *pair_off, int npairs,
                          double required_percent, double max_error, int max_tries, int find_best, double ratio_allowed,
                          const int32_t *samples, const unsigned long long *seeds, int32_t *success, double *essential,
                          double *camera, double *inlier_percent, int32_t *inlier_idx, int32_t *n_inliers,
                          int32_t *best_try, int32_t *best_root, int32_t *tries_run) {
  SPV_TRY(ransac_batch_check(pair_off, npairs, max_tries, samples));
  const long long total = pair_off[npairs];
  if (total > 0 && (!x0 || !x1)) return set_error(SPV_ERR_INVALID, "null pointer");
  std::vector<RansacBatchSlot> first;
  ransac_batch_first_round(pair_off, npairs, max_tries, &first);
  DevBuf dx, dxp;
  hipStream_t st = hipStreamPerThread;
  if (!first.empty()) {
    if (!samples && !seeds) return set_error(SPV_ERR_INVALID, "neither samples nor seeds");
    if (!success || !essential || !camera || !inlier_percent || !n_inliers || !inlier_idx)
      return set_error(SPV_ERR_INVALID, "null pointer");
    SPV_TRY(host_begin(device_list()[0], &st));
    const size_t ib = (size_t)total * 3 * sizeof(double);
    SPV_TRY(alloc_all({{&dx, ib}, {&dxp, ib}}));
    SPV_TRY(dx.copy_in(x0, ib, st));
    SPV_TRY(dxp.copy_in(x1, ib, st));
    x0 = dx.as<double>();
    x1 = dxp.as<double>();
  }
  return ransac_fit_batch_run(x0, x1, pair_off, npairs, required_percent, max_error, max_tries, find_best, ratio_allowed,
                              samples, seeds, success, essential, camera, inlier_percent, inlier_idx, n_inliers, best_try,
                              best_root, tries_run, nullptr, st);
}

// The many-views resection through host pointers, on the first selected device: both arrays up, one
// resect_fit_batch_run, the mask and the per-try arrays back where they are wanted.  A collection in which no set
// runs touches no device.
int host_resect_fit_batch(const double *x, const double *Xw, const long long *view_off, int nviews, double required_percent,
                          double max_error, int max_tries, int find_best, const int32_t *samples,
                          const unsigned long long *seeds, int32_t *success, double *camera, double *inlier_percent,
                          int32_t *n_inliers, int32_t *best_try, int32_t *tries_run, uint8_t *inlier_mask,
                          double *try_cameras, int32_t *try_inliers) {
  SPV_TRY(resect_check(view_off, nviews, required_percent, max_error, max_tries, samples));
  const size_t total = (size_t)view_off[nviews], ntry = (size_t)nviews * (size_t)max_tries;
  if (total > 0 && (!x || !Xw)) return set_error(SPV_ERR_INVALID, "null pointer");
  std::vector<RansacBatchSlot> first;
  resect_first_round(view_off, nviews, max_tries, &first);
  if (first.empty()) {
    if (inlier_mask) memset(inlier_mask, 0, total);
    if (try_inliers) memset(try_inliers, 0, ntry * sizeof(int32_t));
    if (try_cameras) memset(try_cameras, 0xFF, ntry * 12 * sizeof(double));
    // (no set runs: the arrays are not read, every set reports what a skipped set reports)
    return resect_fit_batch_run(x, Xw, view_off, nviews, required_percent, max_error, max_tries, find_best, samples,
                                seeds, success, camera, inlier_percent, n_inliers, best_try, tries_run, nullptr, nullptr,
                                nullptr, hipStreamPerThread);
  }
  if (!samples && !seeds) return set_error(SPV_ERR_INVALID, "neither samples nor seeds");
  if (!success || !camera || !inlier_percent || !n_inliers) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  DevBuf dx, dX, dm, dc, di;
  SPV_TRY(alloc_all({{&dx, total * 3 * sizeof(double)}, {&dX, total * 4 * sizeof(double)}, {&dm, inlier_mask ? total : 0},
                     {&dc, try_cameras ? ntry * 12 * sizeof(double) : 0}, {&di, try_inliers ? ntry * sizeof(int32_t) : 0}}));
  SPV_TRY(dx.copy_in(x, total * 3 * sizeof(double), st));
  SPV_TRY(dX.copy_in(Xw, total * 4 * sizeof(double), st));
  SPV_TRY(resect_fit_batch_run(dx.as<double>(), dX.as<double>(), view_off, nviews, required_percent, max_error, max_tries,
                               find_best, samples, seeds, success, camera, inlier_percent, n_inliers, best_try, tries_run,
                               inlier_mask ? dm.as<uint8_t>() : nullptr, try_cameras ? dc.as<double>() : nullptr,
                               try_inliers ? di.as<int32_t>() : nullptr, st));
  if (inlier_mask) SPV_TRY(dm.copy_out(inlier_mask, total, st));
  if (try_cameras) SPV_TRY(dc.copy_out(try_cameras, ntry * 12 * sizeof(double), st));
  if (try_inliers) SPV_TRY(di.copy_out(try_inliers, ntry * sizeof(int32_t), st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

// The many-sets triangulation through host pointers, on the first selected device: both arrays and the mask up,
// one dlt_batch_run, the offsets back, then as many result rows as were selected and fit.  A collection without a
// row in a used set touches no device.
int host_dlt_batch(const double *x0, const double *x1, const long long *pair_off, int npairs, const double *P0s,
                   const double *P1s, const int32_t *use, const uint8_t *mask, double *X, double *err, int32_t *rows,
                   long long capacity, long long *out_off, long long *count) {
  SPV_TRY(dlt_batch_check(x0, x1, pair_off, npairs, P1s, X, err, capacity));
  std::vector<DltBatchItem> items;
  long long bound = 0;
  dlt_batch_items(pair_off, npairs, use, mask != nullptr, &items, nullptr, &bound);
  std::vector<long long> off((size_t)npairs + 2, 0);
  if (!items.empty()) {
    hipStream_t st;
    SPV_TRY(host_begin(device_list()[0], &st));
    const size_t total = (size_t)pair_off[npairs], ib = total * 3 * sizeof(double);
    const size_t cap = (size_t)std::min(capacity, bound);  // no more rows than that are ever written
    DevBuf dx, dxp, dm, dX, de, dr, doff;
    SPV_TRY(alloc_all({{&dx, ib}, {&dxp, ib}, {&doff, off.size() * sizeof(long long)}}));
    if (mask) SPV_TRY(dm.upload(mask, total, st));
    if (X) SPV_TRY(dX.alloc(cap * 4 * sizeof(double)));
    if (err) SPV_TRY(de.alloc(cap * sizeof(double)));
    if (rows) SPV_TRY(dr.alloc(cap * sizeof(int32_t)));
    SPV_TRY(dx.copy_in(x0, ib, st));
    SPV_TRY(dxp.copy_in(x1, ib, st));
    SPV_TRY(dlt_batch_run(dx.as<double>(), dxp.as<double>(), pair_off, npairs, P0s, P1s, use, mask ? dm.as<uint8_t>() : nullptr,
                          X ? dX.as<double>() : nullptr, err ? de.as<double>() : nullptr, rows ? dr.as<int32_t>() : nullptr,
                          (long long)cap, doff.as<long long>(), doff.as<long long>() + npairs + 1, st));
    SPV_TRY(doff.copy_out(off.data(), off.size() * sizeof(long long), st));
    SPV_HIP_CHECK(hipStreamSynchronize(st));
    const size_t n = (size_t)std::min<long long>(off[(size_t)npairs + 1], (long long)cap);
    if (X) SPV_TRY(dX.copy_out(X, n * 4 * sizeof(double), st));
    if (err) SPV_TRY(de.copy_out(err, n * sizeof(double), st));
    if (rows) SPV_TRY(dr.copy_out(rows, n * sizeof(int32_t), st));
    SPV_HIP_CHECK(hipStreamSynchronize(st));
  }
  if (out_off) memcpy(out_off, off.data(), ((size_t)npairs + 1) * sizeof(long long));
  if (count) *count = off[(size_t)npairs + 1];
  if (off[(size_t)npairs + 1] > capacity)
    return set_error(SPV_ERR_OVERFLOW, "dlt_triangulate_batch: %lld rows do not fit a capacity of %lld", off[(size_t)npairs + 1], capacity);
  return SPV_OK;
}

// Exact p-norm k-NN through host pointers, on the first selected device (no sharding).
int host_bruteforce(const void *x, const void *y, int is_int, int xrows, int yrows, int dim, int k, float p,
                    uint64_t *idx, void *dist) {
  SPV_TRY(bruteforce_check(xrows, yrows, dim, k, p));
  if (yrows == 0) return SPV_OK;
  if (!y || !idx || !dist || (xrows > 0 && !x)) return set_error(SPV_ERR_INVALID, "null pointer");
  const int dev = device_list()[0];
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t ib = (size_t)yrows * k * sizeof(uint64_t), db = (size_t)yrows * k * 4;
  const size_t wsb = bruteforce_plan(xrows, yrows, k, 0).part_bytes;
  DevBuf dx, dy, di, dd, ws;
  SPV_TRY(dx.upload(x, (size_t)xrows * dim * 4, st));
  SPV_TRY(dy.upload(y, (size_t)yrows * dim * 4, st));
  SPV_TRY(alloc_all({{&di, ib}, {&dd, db}, {&ws, wsb}}));
  SPV_TRY(bruteforce_run(dx.p, dy.p, is_int, xrows, yrows, dim, k, p, 0, di.as<uint64_t>(), dd.p, ws.p, wsb, st));
  SPV_TRY(dd.copy_out(dist, db, st));
  return download(dev, idx, di.p, ib, st);
}

// Approximate L2 k-NN through host pointers, on the first selected device (no sharding).  dist may be NULL.
int host_ann(const float *x, const float *y, int xrows, int yrows, int dim, int k, int ncand, uint64_t *idx,
             float *dist) {
  SPV_TRY(ann_check(xrows, yrows, dim, k, ncand));
  if (yrows == 0) return SPV_OK;
  if (!y || !idx || (xrows > 0 && !x)) return set_error(SPV_ERR_INVALID, "null pointer");
  const int dev = device_list()[0];
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t ib = (size_t)yrows * k * sizeof(uint64_t), db = (size_t)yrows * k * 4;
  const size_t wsb = std::max<size_t>(ann_plan(xrows, yrows, dim, k, ncand, 0).total_bytes, 256);
  DevBuf dx, dy, di, dd, ws;
  SPV_TRY(dx.upload(x, (size_t)xrows * dim * 4, st));
  SPV_TRY(dy.upload(y, (size_t)yrows * dim * 4, st));
  SPV_TRY(alloc_all({{&di, ib}, {&dd, db}, {&ws, wsb}}));
  SPV_TRY(ann_run(dx.as<float>(), dy.as<float>(), xrows, yrows, dim, k, ncand, 0, di.as<uint64_t>(), dd.as<float>(),
                  ws.p, wsb, st));
  if (dist) SPV_TRY(dd.copy_out(dist, db, st));
  return download(dev, idx, di.p, ib, st);
}

// Rectification through host pointers, on the first selected device: both images up, one kernel,
// the four outputs back.  r0 / r1 double[rows, cols, nchan], ri0 / ri1 int32[rows, cols].
int host_rectify(const double *P0, const double *P1, const double *im0, const double *im1, int wid, int hgt,
                 int nchan, double sf, double *r0, double *r1, int32_t *ri0, int32_t *ri1) {
  int shape[3];
  SPV_TRY(rectify_shape(wid, hgt, nchan, sf, shape));
  if (!P0 || !P1 || !im0 || !im1 || !r0 || !r1 || !ri0 || !ri1) return set_error(SPV_ERR_INVALID, "null pointer");
  double F[9];
  rectify_fundamental(P0, P1, F);
  const int dev = device_list()[0];
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t ib = (size_t)hgt * wid * nchan * sizeof(double);
  const size_t ob = (size_t)shape[0] * shape[1], vb = ob * nchan * sizeof(double), xb = ob * sizeof(int32_t);
  DevBuf di0, di1, dr0, dr1, dx0, dx1;
  SPV_TRY(alloc_all({{&di0, ib}, {&di1, ib}, {&dr0, vb}, {&dr1, vb}, {&dx0, xb}, {&dx1, xb}}));
  SPV_TRY(di0.copy_in(im0, ib, st));
  SPV_TRY(di1.copy_in(im1, ib, st));
  SPV_TRY(rectify_run(F, di0.p, di1.p, SPV_RECTIFY_F64, wid, hgt, nchan, sf, dr0.p, dr1.p, dx0.as<int32_t>(),
                      dx1.as<int32_t>(), st));
  SPV_TRY(dx0.copy_out(ri0, xb, st));
  SPV_TRY(dx1.copy_out(ri1, xb, st));
  SPV_TRY(download(dev, r0, dr0.p, vb, st));
  return download(dev, r1, dr1.p, vb, st);
}

int alloc_out(NdArray *arr, size_t rows, size_t cols, int itemsize, size_t depth);

// The many-pairs rectification through host pointers, on the first selected device: the images up, with `crop` the
// bounds step and its boxes back (the one synchronisation), the four flat outputs sized by the windows, one
// rectify_batch_run, the outputs back.  A collection without a used pair touches no device.
int host_rectify_batch(const void *images, int dtype, const int32_t *sizes, int nimg, int nchan, double sf,
                       const int32_t *pairs, int npairs, const double *P0s, const double *P1s, const int32_t *use,
                       int crop, NdArray *r0, NdArray *r1, NdArray *ri0, NdArray *ri1, int32_t *box,
                       long long *out_off) {
  if (dtype != SPV_RECTIFY_F64 && dtype != SPV_RECTIFY_U8 && dtype != SPV_RECTIFY_F32)
    return set_error(SPV_ERR_INVALID, "dtype %d", dtype);
  const int esize = dtype == SPV_RECTIFY_F64 ? 8 : dtype == SPV_RECTIFY_F32 ? 4 : 1;
  RectifyBatchPlan pl;
  SPV_TRY(rectify_batch_plan(sizes, nimg, nchan, sf, pairs, npairs, use, nullptr, &pl));
  if (!r0 || !r1 || !ri0 || !ri1 || !out_off || (npairs > 0 && !box)) return set_error(SPV_ERR_INVALID, "null output");
  if (pl.used > 0 && (!images || !P1s)) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st = nullptr;
  DevBuf dim;
  const int dev = device_list()[0];
  if (pl.used > 0) {
    SPV_TRY(host_begin(dev, &st));
    SPV_TRY(dim.upload(images, (size_t)pl.img_off[nimg] * nchan * esize, st));
    if (crop) {
      DevBuf dbox;
      const size_t bb = (size_t)npairs * 4 * sizeof(int32_t);
      SPV_TRY(dbox.alloc(bb));
      SPV_TRY(rectify_batch_bounds_run(sizes, nimg, nchan, sf, pairs, npairs, P0s, P1s, use, dbox.as<int32_t>(), st));
      SPV_TRY(dbox.copy_out(box, bb, st));
      SPV_HIP_CHECK(hipStreamSynchronize(st));
      SPV_TRY(rectify_batch_plan(sizes, nimg, nchan, sf, pairs, npairs, use, box, &pl));
    }
  }
  if (npairs > 0 && !(crop && pl.used > 0)) memcpy(box, pl.box.data(), (size_t)npairs * 4 * sizeof(int32_t));
  memcpy(out_off, pl.out_off.data(), ((size_t)npairs + 1) * sizeof(long long));
  const size_t total = (size_t)pl.out_off[npairs], vb = total * nchan * esize, xb = total * sizeof(int32_t);
  SPV_TRY(alloc_out(r0, total * nchan, 1, esize, 0));
  SPV_TRY(alloc_out(r1, total * nchan, 1, esize, 0));
  SPV_TRY(alloc_out(ri0, total, 1, (int)sizeof(int32_t), 0));
  SPV_TRY(alloc_out(ri1, total, 1, (int)sizeof(int32_t), 0));
  if (total == 0) return SPV_OK;
  DevBuf dr0, dr1, dx0, dx1;
  SPV_TRY(alloc_all({{&dr0, vb}, {&dr1, vb}, {&dx0, xb}, {&dx1, xb}}));
  SPV_TRY(rectify_batch_run(dim.p, dtype, sizes, nimg, nchan, sf, pairs, npairs, P0s, P1s, use, box, dr0.p, dr1.p,
                            dx0.as<int32_t>(), dx1.as<int32_t>(), st));
  SPV_TRY(dx0.copy_out(ri0->m_data, xb, st));
  SPV_TRY(dx1.copy_out(ri1->m_data, xb, st));
  SPV_TRY(download(dev, r0->m_data, dr0.p, vb, st));
  return download(dev, r1->m_data, dr1.p, vb, st);
}

// First table size of the host forms that size the table to the result (0: the default guess).
std::atomic<int> g_sift_first_rows{0};

// SIFT through host pointers, on the first selected device.  With `out` the table is sized to the
// true count: when the first guess is short, the pipeline runs again into a second, exact buffer (the
// first one goes back to the pool when the call ends).  Otherwise `table` holds `capacity` rows and a
// longer result is SPV_ERR_OVERFLOW with the true count in *count.
int host_sift(const float *im, int wid, int hgt, NdArray *out, float *table, int capacity, int32_t *count) {
  SPV_TRY(sift_check(wid, hgt));
  if (!im || (!out && (!count || (capacity > 0 && !table)))) return set_error(SPV_ERR_INVALID, "null pointer");
  if (capacity < 0) return set_error(SPV_ERR_INVALID, "negative capacity");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t wsb = sift_workspace_bytes(wid, hgt);
  const int first = g_sift_first_rows.load();
  int cap = !out ? capacity
                 : first > 0 ? first : std::max(1024, (int)std::min<long long>((long long)wid * hgt / 16, 1 << 20));
  DevBuf dim, ws, dt, dt_exact, dc;
  SPV_TRY(dim.upload(im, (size_t)wid * hgt * sizeof(float), st));
  SPV_TRY(alloc_all({{&ws, wsb}, {&dc, sizeof(int32_t)}, {&dt, (size_t)std::max(cap, 1) * 132 * sizeof(float)}}));
  DevBuf *tab = &dt;
  int32_t n = 0;
  for (int pass = 0; pass < 2; ++pass) {
    SPV_TRY(sift_run(dim.as<float>(), wid, hgt, ws.p, wsb, tab->as<float>(), cap, dc.as<int>(), st));
    SPV_TRY(dc.copy_out(&n, sizeof(n), st));
    SPV_HIP_CHECK(hipStreamSynchronize(st));
    if (!out || n <= cap) break;
    cap = n;
    SPV_TRY(dt_exact.alloc((size_t)cap * 132 * sizeof(float)));
    tab = &dt_exact;
  }
  const int rows = std::min(n, cap);
  if (out) {
    SPV_TRY(alloc_out(out, (size_t)n, 132, (int)sizeof(float), 0));
    table = static_cast<float *>(out->m_data);
  } else {
    *count = n;
  }
  SPV_TRY(tab->copy_out(table, (size_t)rows * 132 * sizeof(float), st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  if (!out && n > capacity)
    return set_error(SPV_ERR_OVERFLOW, "sift: %d rows do not fit a table of %d", (int)n, capacity);
  return SPV_OK;
}

// spv_sift_batch_device through host pointers, on the first selected device.  The workspace is what runs all
// images as one group, but no more than the buffer cache keeps (or than the largest image needs): the call
// then runs as several groups.
int host_sift_tables(const float *images, const int32_t *sizes, int nimg, float *table, const long long *cap_off,
                     int32_t *counts) {
  SiftBatchPlan plan;
  SPV_TRY(sift_batch_plan(sizes, nimg, 0, &plan));
  SPV_TRY(check_offsets(cap_off, nimg, "cap_off"));
  if (nimg == 0) return SPV_OK;
  if (!images || !counts || (cap_off[nimg] > 0 && !table)) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t wsb = std::min(plan.all_bytes, std::max(plan.min_bytes, kDevicePoolCapBytes));
  const size_t tb = (size_t)cap_off[nimg] * 132 * sizeof(float), cb = (size_t)nimg * sizeof(int32_t);
  DevBuf dim, ws, dt, dc;
  SPV_TRY(dim.upload(images, (size_t)plan.pixels * sizeof(float), st));
  SPV_TRY(alloc_all({{&ws, wsb}, {&dc, cb}, {&dt, std::max<size_t>(tb, 1)}}));
  SPV_TRY(sift_batch_run(dim.as<float>(), sizes, nimg, ws.p, wsb, dt.as<float>(), cap_off, dc.as<int32_t>(), st));
  SPV_TRY(dc.copy_out(counts, cb, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  int short_of = -1;
  for (int i = 0; i < nimg; ++i) {
    const long long cap = cap_off[i + 1] - cap_off[i], rows = std::min<long long>(counts[i], cap);
    if (counts[i] > cap && short_of < 0) short_of = i;
    if (rows > 0)
      SPV_HIP_CHECK(hipMemcpyAsync(table + (size_t)cap_off[i] * 132, dt.as<float>() + (size_t)cap_off[i] * 132,
                                 (size_t)rows * 132 * sizeof(float), hipMemcpyDeviceToHost, st));
  }
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  if (short_of >= 0)
    return set_error(SPV_ERR_OVERFLOW, "sift: the %d rows of image %d do not fit its region of %lld", (int)counts[short_of],
                     short_of, cap_off[short_of + 1] - cap_off[short_of]);
  return SPV_OK;
}

struct SiftBatch {
  struct Item {
    const float *im;
    int wid, hgt;
    NdArray *out;
  };
  std::vector<Item> items;
};

int host_cascade_one(int dev, const float *x, const float *y, int xrows, int yrows, int dim, int m,
                     int n, int g, const float *dict, uint64_t *idx, float *dist, int32_t *ncand) {
  SPV_TRY(check_cascade_args(xrows, yrows, dim, m, n, g));
  if (yrows == 0) return SPV_OK;
  if (!y || !idx || !dist || !dict || (xrows > 0 && !x))
    return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t xb = (size_t)xrows * dim * sizeof(float), yb = (size_t)yrows * dim * sizeof(float);
  const size_t db = (size_t)n * dim * m * sizeof(float);
  const size_t ib = (size_t)yrows * 2 * sizeof(uint64_t), sb = (size_t)yrows * 2 * sizeof(float);
  const size_t nb = (size_t)yrows * sizeof(int32_t);
  const size_t wsb = cascade_workspace_bytes(xrows, yrows, dim, m, n, g);
  HostPrefault touch_idx(idx, ib, {{x, xb}, {y, yb}});
  DevBuf dx, dy, dd, di, dds, dn, ws;
  SPV_TRY(alloc_all({{&dx, xb}, {&dy, yb}, {&dd, db}, {&di, ib}, {&dds, sb}, {&dn, nb}, {&ws, wsb}}));
  SPV_TRY(dx.copy_in(x, xb, st));
  SPV_TRY(dy.copy_in(y, yb, st));
  SPV_TRY(dd.copy_in(dict, db, st));
  SPV_TRY(cascade_run(dx.as<float>(), dy.as<float>(), xrows, yrows, dim, m, n, g, dd.as<float>(),
                      di.as<uint64_t>(), dds.as<float>(), dn.as<int32_t>(), ws.p, wsb, st));
  touch_idx.wait();
  SPV_TRY(dds.copy_out(dist, sb, st));
  if (ncand) SPV_TRY(dn.copy_out(ncand, nb, st));
  return download(dev, idx, di.p, ib, st);
}

int host_cascade(const float *x, const float *y, int xrows, int yrows, int dim, int m, int n,
                 int g, const float *dict, uint64_t *idx, float *dist, int32_t *ncand) {
  SPV_TRY(check_cascade_args(xrows, yrows, dim, m, n, g));
  const std::vector<int> devs = device_list();
  if (yrows > 0 && gather_transport(devs, yrows) != SPV_GATHER_DIRECT) {
    if (!y || !idx || !dist || !dict || (xrows > 0 && !x)) return set_error(SPV_ERR_INVALID, "null pointer");
    return cascade_gathered(devs, {x, nullptr}, {y, nullptr}, {dict, nullptr}, xrows, yrows, dim, m, n, g, idx, dist,
                            ncand, SPV_GATHER_AUTO);
  }
  return run_sharded(yrows, [&](int dev, long long lo, long long hi) {
    return host_cascade_one(dev, x, y ? y + (size_t)lo * dim : y, xrows, (int)(hi - lo), dim, m, n, g,
                            dict, idx ? idx + 2 * lo : idx, dist ? dist + 2 * lo : dist,
                            ncand ? ncand + lo : ncand);
  });
}

// The many-pairs cascade through host pointers, on the first selected device (no sharding): the whole of rows and
// the dictionary up, one cascade_batch_run, the results back.
int host_cascade_batch(const float *rows, const long long *seg_off, int nseg, int dim, int m, int n, int g,
                       const int32_t *pairs, int npairs, const float *dict, uint64_t *idx, float *dist, int32_t *ncand) {
  CascadeBatchPlan p;
  SPV_TRY(cascade_batch_plan(seg_off, nseg, dim, m, n, g, pairs, npairs, &p));
  if (p.out_rows == 0) return SPV_OK;
  if (!rows || !dict || !idx || !dist) return set_error(SPV_ERR_INVALID, "null pointer");
  const int dev = device_list()[0];
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t xb = (size_t)p.total_rows * dim * sizeof(float), db = (size_t)n * dim * m * sizeof(float);
  const size_t ib = (size_t)p.out_rows * 2 * sizeof(uint64_t), sb = (size_t)p.out_rows * 2 * sizeof(float);
  const size_t nb = (size_t)p.out_rows * sizeof(int32_t);
  HostPrefault touch_idx(idx, ib, {{rows, xb}});
  DevBuf dx, dd, di, dds, dn, ws;
  SPV_TRY(alloc_all({{&dx, xb}, {&dd, db}, {&di, ib}, {&dds, sb}, {&dn, nb}, {&ws, p.total_bytes}}));
  SPV_TRY(dx.copy_in(rows, xb, st));
  SPV_TRY(dd.copy_in(dict, db, st));
  SPV_TRY(cascade_batch_run(dx.as<float>(), seg_off, nseg, dim, m, n, g, pairs, npairs, dd.as<float>(), di.as<uint64_t>(),
                            dds.as<float>(), dn.as<int32_t>(), ws.p, p.total_bytes, st));
  touch_idx.wait();
  SPV_TRY(dds.copy_out(dist, sb, st));
  if (ncand) SPV_TRY(dn.copy_out(ncand, nb, st));
  return download(dev, idx, di.p, ib, st);
}

int host_dlt_one(int dev, const double *P0, const double *P1, int npt, const double *x,
                 const double *xp, double *dst, bool want_error) {
  if (npt < 0) return set_error(SPV_ERR_INVALID, "negative point count");
  if (npt == 0) return SPV_OK;
  if (!P0 || !P1 || !x || !xp || !dst) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(dev, &st));
  const size_t row = (want_error ? 1 : 4) * sizeof(double);
  const size_t ib = (size_t)npt * 3 * sizeof(double);
  const size_t ob = (size_t)npt * row;
  DevBuf dx, dxp, dd;
  SPV_TRY(alloc_all({{&dx, ib}, {&dxp, ib}, {&dd, ob}}));
  if (ob < D2HPipeline::kMinBytes) {
    HostPrefault touch(dst, ob, {{x, ib}, {xp, ib}});
    SPV_TRY(dx.copy_in(x, ib, st));
    SPV_TRY(dxp.copy_in(xp, ib, st));
    SPV_TRY(dlt_run(P0, P1, npt, dx.as<double>(), dxp.as<double>(), dd.as<double>(), want_error, st));
    touch.wait();
    SPV_TRY(dd.copy_out(dst, ob, st));
    SPV_HIP_CHECK(hipStreamSynchronize(st));
    return SPV_OK;
  }
  // Large batches are transfer-bound at this boundary (480 MB in, 320 MB out for 10M points against
  // 0.2 ms of kernel): the points are independent, so the call runs in chunks -- upload and solve
  // chunk k while the pinned pipeline brings chunk k-1's rows back over the other PCIe direction.
  // (measured on 10M points: 1M-point chunks 14.7 ms per call, 256k 16.5, 4M 18; a fresh result
  // array is touched by HostPrefault's threads meanwhile: the kernel zeroes 320 MB of new pages)
  const long long chunk_pts = 1 << 20;
  const int nchunks = (int)((npt + chunk_pts - 1) / chunk_pts);
  std::vector<ScopedEvent> produced(nchunks);
  HostPrefault touch(dst, ob, {{x, ib}, {xp, ib}});
  D2HPipeline pipe(dev, dd.p, dst, ob, (size_t)chunk_pts * row);
  pipe.set_prefault(&touch);  // a slice lands only after its own pages have been touched
  int status = SPV_OK;
  for (int k = 0; k < nchunks && status == SPV_OK; ++k) {
    const long long p0 = (long long)k * chunk_pts, cnt = std::min<long long>(chunk_pts, npt - p0);
    status = [&] {
      SPV_HIP_CHECK(hipMemcpyAsync(dx.as<double>() + 3 * p0, x + 3 * p0, (size_t)cnt * 24, hipMemcpyHostToDevice, st));
      SPV_HIP_CHECK(hipMemcpyAsync(dxp.as<double>() + 3 * p0, xp + 3 * p0, (size_t)cnt * 24, hipMemcpyHostToDevice, st));
      SPV_TRY(dlt_run(P0, P1, cnt, dx.as<double>() + 3 * p0, dxp.as<double>() + 3 * p0,
                      reinterpret_cast<double *>(dd.as<char>() + (size_t)p0 * row), want_error, st));
      SPV_TRY(produced[k].record(st));
      return SPV_OK;
    }();
    if (status == SPV_OK) pipe.ready(k, produced[k].ev);
  }
  if (status != SPV_OK) {
    const std::string msg = g_message;  // finish() may overwrite the thread's message
    pipe.abort();
    (void)pipe.finish();
    (void)hipStreamSynchronize(st);
    return set_error(status, "%s", msg.c_str());
  }
  status = pipe.finish();
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return status;
}

int host_dlt(const double *P0, const double *P1, int npt, const double *x, const double *xp,
             double *dst, bool want_error) {
  if (npt < 0) return set_error(SPV_ERR_INVALID, "negative point count");
  const int cols = want_error ? 1 : 4;
  const std::vector<int> devs = device_list();
  if (npt > 0 && gather_transport(devs, npt) != SPV_GATHER_DIRECT) {
    if (!P0 || !P1 || !x || !xp || !dst) return set_error(SPV_ERR_INVALID, "null pointer");
    return dlt_gathered(devs, P0, P1, {x, nullptr}, {xp, nullptr}, npt, dst, want_error, SPV_GATHER_AUTO);
  }
  return run_sharded(npt, [&](int dev, long long lo, long long hi) {
    return host_dlt_one(dev, P0, P1, (int)(hi - lo), x ? x + 3 * lo : x, xp ? xp + 3 * lo : xp,
                        dst ? dst + cols * lo : dst, want_error);
  });
}

int host_dlt_score(const double *P0, const double *P1s, int nhyp, int npt, const double *x,
                   const double *xp, double max_error, int32_t *counts, uint8_t *mask) {
  if (npt < 0 || nhyp < 0) return set_error(SPV_ERR_INVALID, "negative count");
  if (nhyp == 0) return SPV_OK;
  if (!P0 || !P1s || !counts || (npt > 0 && (!x || !xp))) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t ib = (size_t)npt * 3 * sizeof(double), cb = (size_t)nhyp * sizeof(int32_t);
  const size_t wsb = dlt_score_workspace_bytes(nhyp, npt);
  DevBuf dx, dxp, dp, dc, dm, ws;
  SPV_TRY(dx.upload(x, ib, st));
  SPV_TRY(dxp.upload(xp, ib, st));
  SPV_TRY(dp.upload(P1s, (size_t)nhyp * 12 * sizeof(double), st));
  SPV_TRY(dc.alloc(cb));
  if (mask) SPV_TRY(dm.alloc((size_t)nhyp * npt));
  SPV_TRY(ws.alloc(wsb));
  SPV_TRY(dlt_score_run(P0, dp.as<double>(), nhyp, npt, dx.as<double>(), dxp.as<double>(), max_error,
                        dc.as<int>(), mask ? dm.as<unsigned char>() : nullptr, ws.p, wsb, st));
  SPV_TRY(dc.copy_out(counts, cb, st));
  if (mask) SPV_TRY(dm.copy_out(mask, (size_t)nhyp * npt, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

int host_ransac_process(const double *Fs, int nF, const double *x0, const double *x1, int npt,
                        double ratio_allowed, double required_percent, double max_error, int find_best,
                        int32_t *success, int32_t *inlier_count, int32_t *best_cam, double *best_P, double *ratio,
                        double *E, int32_t *counts4, uint8_t *mask) {
  if (nF < 0 || npt < 0) return set_error(SPV_ERR_INVALID, "negative count");
  if (nF == 0) return SPV_OK;
  if (npt == 0) return set_error(SPV_ERR_INVALID, "no correspondences");
  if (!Fs || !x0 || !x1 || !success || !inlier_count || !best_cam) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  // candidates per launch: the scoring grid takes 65535 hypotheses (4 per candidate) and the
  // per-camera masks are kept under 1 GiB
  int chunk = 16383;
  if (mask) chunk = (int)std::max<long long>(1, std::min<long long>(chunk, ((long long)1 << 28) / npt));
  chunk = std::min(chunk, nF);
  const size_t ib = (size_t)npt * 3 * sizeof(double);
  const size_t wsb = ransac_workspace_bytes(chunk, npt, mask != nullptr);
  const size_t c4 = (size_t)chunk * sizeof(int32_t), c8 = (size_t)chunk * sizeof(double);
  DevBuf dx, dxp, dF, ds, dc, db, dP, dr, dE, d4, dm, ws;
  SPV_TRY(alloc_all({{&dx, ib}, {&dxp, ib}, {&dF, 9 * c8}, {&ds, c4}, {&dc, c4}, {&db, c4}, {&dP, 12 * c8},
                     {&dr, c8}, {&dE, 9 * c8}, {&d4, 4 * c4}}));
  if (mask) SPV_TRY(dm.alloc((size_t)chunk * npt));
  SPV_TRY(ws.alloc(wsb));
  SPV_TRY(dx.copy_in(x0, ib, st));
  SPV_TRY(dxp.copy_in(x1, ib, st));
  for (int f0 = 0; f0 < nF; f0 += chunk) {
    const int nf = std::min(chunk, nF - f0);
    const size_t n4 = (size_t)nf * sizeof(int32_t), n8 = (size_t)nf * sizeof(double);
    SPV_TRY(dF.copy_in(Fs + (size_t)f0 * 9, 9 * n8, st));
    SPV_TRY(ransac_process_run(dF.as<double>(), nf, npt, dx.as<double>(), dxp.as<double>(), ratio_allowed,
                               required_percent, max_error, find_best, ds.as<int>(), dc.as<int>(), db.as<int>(),
                               dP.as<double>(), dr.as<double>(), dE.as<double>(), d4.as<int>(),
                               mask ? dm.as<unsigned char>() : nullptr, ws.p, wsb, st));
    SPV_TRY(ds.copy_out(success + f0, n4, st));
    SPV_TRY(dc.copy_out(inlier_count + f0, n4, st));
    SPV_TRY(db.copy_out(best_cam + f0, n4, st));
    if (best_P) SPV_TRY(dP.copy_out(best_P + (size_t)f0 * 12, 12 * n8, st));
    if (ratio) SPV_TRY(dr.copy_out(ratio + f0, n8, st));
    if (E) SPV_TRY(dE.copy_out(E + (size_t)f0 * 9, 9 * n8, st));
    if (counts4) SPV_TRY(d4.copy_out(counts4 + (size_t)f0 * 4, 4 * n4, st));
    if (mask) SPV_TRY(dm.copy_out(mask + (size_t)f0 * npt, (size_t)nf * npt, st));
    SPV_HIP_CHECK(hipStreamSynchronize(st));  // the staging buffers are reused by the next chunk
  }
  return SPV_OK;
}

// ---- seven-point solver + RANSAC loop (ransac.hip) -----------------------------------
int host_seven_point(const double *x, const double *xp, int n, int32_t *nroot, double *Fs, double *basis) {
  if (n < 0) return set_error(SPV_ERR_INVALID, "negative count");
  if (n == 0) return SPV_OK;
  if (!x || !xp || !nroot || !Fs) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t ib = (size_t)n * 14 * sizeof(double), fb = (size_t)n * 27 * sizeof(double);
  const size_t nb = (size_t)n * sizeof(int32_t), bb = (size_t)n * 18 * sizeof(double);
  DevBuf dx, dxp, dF, dn, db;
  SPV_TRY(dx.upload(x, ib, st));
  SPV_TRY(dxp.upload(xp, ib, st));
  SPV_TRY(alloc_all({{&dF, fb}, {&dn, nb}}));
  if (basis) SPV_TRY(db.alloc(bb));
  SPV_TRY(seven_point_run(dx.as<double>(), dxp.as<double>(), n, dF.as<double>(), dn.as<int>(),
                          basis ? db.as<double>() : nullptr, st));
  SPV_TRY(dF.copy_out(Fs, fb, st));
  SPV_TRY(dn.copy_out(nroot, nb, st));
  if (basis) SPV_TRY(db.copy_out(basis, bb, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

}  // namespace

// (floyd_sample, ransac_seed and check_fit_args also serve ransac_batch.hip: common.h)
// One 7-subset of [0, N) the way the reference draws it (floyd_sample, src/RansacFitter.h:120-132):
// for r = N-7 .. N-1 a value v uniform on [1, r] is taken unless already present, else r.  (Row 0 is
// therefore never drawn: the reference's range starts at 1.)  The reference seeds a fresh mt19937 from
// std::random_device for every subset and walks an unordered_set; here one generator serves all the
// tries of a call and the rows keep their insertion order.
void floyd_sample(std::mt19937 &gen, int N, int *out) {
  int n = 0;
  for (int r = N - 7; r < N; ++r) {
    const int v = std::uniform_int_distribution<>(1, r)(gen);
    bool present = false;
    for (int i = 0; i < n; ++i) present |= (out[i] == v);
    out[n++] = present ? r : v;
  }
}

uint32_t ransac_seed(uint64_t seed) {
  if (seed) return (uint32_t)(seed ^ (seed >> 32));
  if (const char *e = getenv("SPECTAVI_RANSAC_SEED")) return (uint32_t)strtoul(e, nullptr, 0);
  return std::random_device{}();
}

int check_fit_args(const double *x0, const double *x1, int npt, int max_tries) {
  if (!x0 || !x1) return set_error(SPV_ERR_INVALID, "null pointer");
  // RansacFitter's constructor, src/RansacFitter.h:146-149
  if (npt < 10) return set_error(SPV_ERR_INVALID, "Supplied less than 10 point matches, unsupported.");
  if (max_tries < 0) return set_error(SPV_ERR_INVALID, "negative maximum_tries");
  if (max_tries > 700000000) return set_error(SPV_ERR_INVALID, "maximum_tries above 7e8 (candidate ids are 32-bit: 3 per try)");
  return SPV_OK;
}

namespace {

// samples != NULL: the 7-subsets of the tries, int32[max_tries,7]; otherwise drawn from `seed`.
// inputs_on_device: x0 / x1 are device pointers (the caller's current device) and `st` the caller's stream.
int host_ransac_fit(const double *x0, const double *x1, int npt, double required_percent, double max_error,
                    int max_tries, int find_best, double ratio_allowed, const int32_t *samples, uint64_t seed,
                    int32_t *success, double *essential, double *camera, double *inlier_percent,
                    int32_t *inlier_idx, int32_t *n_inliers, int32_t *best_try, int32_t *best_root,
                    int32_t *tries_run, bool inputs_on_device = false, hipStream_t st = hipStreamPerThread) {
  SPV_TRY(check_fit_args(x0, x1, npt, max_tries));
  if (!success || !essential || !camera || !inlier_percent || !inlier_idx || !n_inliers)
    return set_error(SPV_ERR_INVALID, "null pointer");
  if (!inputs_on_device) SPV_TRY(ensure_device());
  const int batch = std::min(ransac_fit_batch_limit(npt), std::max(max_tries, 1));
  const size_t wsb = ransac_fit_workspace_bytes(batch, npt);
  const size_t ib = (size_t)npt * 3 * sizeof(double);
  DevBuf dx, dxp, ws;
  SPV_TRY(ws.alloc(wsb));
  const double *d_x0 = x0, *d_x1 = x1;
  if (!inputs_on_device) {
    SPV_TRY(dx.upload(x0, ib, st));
    SPV_TRY(dxp.upload(x1, ib, st));
    d_x0 = dx.as<double>();
    d_x1 = dxp.as<double>();
  }
  std::mt19937 gen(samples ? 0u : ransac_seed(seed));
  auto next = [&](int first, int n, int *dst) {
    if (samples) {
      memcpy(dst, samples + (size_t)first * 7, (size_t)n * 7 * sizeof(int));
    } else {
      for (int t = 0; t < n; ++t) floyd_sample(gen, npt, dst + 7 * (size_t)t);
    }
  };
  std::vector<unsigned char> mask((size_t)npt, 0);
  int ok = 0, ninl = 0, bt = -1, br = -1, ran = 0;
  const int rc = ransac_fit_run(d_x0, d_x1, npt, required_percent, max_error, max_tries, find_best, ratio_allowed, next,
                                &ok, essential, camera, &ninl, mask.data(), &bt, &br, &ran, ws.p, wsb, batch, st);
  // the workspace goes back to the pool below: nothing may still be queued on a caller's stream
  // (DevBuf's destructor only drains this thread's own stream; error paths and a call with zero
  // tries return without the per-batch synchronisation)
  if (st != hipStreamPerThread) (void)hipStreamSynchronize(st);
  SPV_TRY(rc);
  *success = ok;
  *inlier_percent = (double)ninl / (double)npt;
  int n = 0;
  if (bt >= 0)
    for (int i = 0; i < npt; ++i)
      if (mask[i]) inlier_idx[n++] = i;
  if (n != ninl) return set_error(SPV_ERR_HIP, "inlier list has %d entries, the count was %d", n, ninl);
  *n_inliers = n;
  if (best_try) *best_try = bt;
  if (best_root) *best_root = br;
  if (tries_run) *tries_run = ran;
  return SPV_OK;
}

int host_ratio(const uint64_t *idx, const void *dist, int dist_is_float, int yrows, double min_ratio,
               int32_t *matches, int32_t *count) {
  if (yrows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
  if (!count) return set_error(SPV_ERR_INVALID, "null pointer");
  *count = 0;
  if (yrows == 0) return SPV_OK;
  if (!idx || !dist || !matches) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t wsb = ratio_workspace_bytes(yrows);
  DevBuf di, dd, dm, dc, ws;
  SPV_TRY(di.upload(idx, (size_t)yrows * 2 * sizeof(uint64_t), st));
  SPV_TRY(dd.upload(dist, (size_t)yrows * 2 * 4, st));
  SPV_TRY(alloc_all({{&dm, (size_t)yrows * 2 * sizeof(int32_t)}, {&dc, sizeof(int32_t)}, {&ws, wsb}}));
  SPV_TRY(ratio_run(di.as<uint64_t>(), dd.p, dist_is_float, yrows, min_ratio, dm.as<int>(), dc.as<int>(),
                    ws.p, wsb, st));
  SPV_TRY(dc.copy_out(count, sizeof(int32_t), st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  if (*count > 0)
    SPV_HIP_CHECK(hipMemcpy(matches, dm.p, (size_t)*count * 2 * sizeof(int32_t), hipMemcpyDeviceToHost));
  return SPV_OK;
}

int host_sift_split(const float *table, int rows, float *geom, uint8_t *desc) {
  if (rows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
  if (rows == 0) return SPV_OK;
  if (!table || !geom || !desc) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t gb = (size_t)rows * 4 * sizeof(float), db = (size_t)rows * 128;
  DevBuf dt, dg, dd;
  SPV_TRY(dt.upload(table, (size_t)rows * 132 * sizeof(float), st));
  SPV_TRY(alloc_all({{&dg, gb}, {&dd, db}}));
  SPV_TRY(sift_split_run(dt.as<float>(), rows, dg.as<float>(), dd.as<uint8_t>(), st));
  SPV_TRY(dg.copy_out(geom, gb, st));
  SPV_TRY(dd.copy_out(desc, db, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

int host_normalize(const float *x, int rows, int dim, float *out_f32, uint8_t *out_u8) {
  if (rows < 0 || dim <= 0) return set_error(SPV_ERR_INVALID, "bad shape");
  if (rows == 0) return SPV_OK;
  if (dim == 1 && rows > 1)
    return set_error(SPV_ERR_INVALID, "normalisation of a single-column table is not supported (dim=1)");
  if (!x || (!out_f32 && !out_u8)) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t ub = (size_t)rows * ((dim + 15) / 16 * 16), fb = ub * sizeof(float);
  const size_t wsb = normalize_workspace_bytes_rows(rows, dim);
  DevBuf dx, df, du, ws;
  SPV_TRY(dx.upload(x, (size_t)rows * dim * sizeof(float), st));
  if (out_f32) SPV_TRY(df.alloc(fb));
  if (out_u8) SPV_TRY(du.alloc(ub));
  SPV_TRY(ws.alloc(wsb));
  SPV_TRY(normalize_run(dx.as<float>(), rows, dim, out_f32 ? df.as<float>() : nullptr,
                        out_u8 ? du.as<unsigned char>() : nullptr, ws.p, wsb, st));
  if (out_f32) SPV_TRY(df.copy_out(out_f32, fb, st));
  if (out_u8) SPV_TRY(du.copy_out(out_u8, ub, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

// The many-tables normalisation through host pointers, on the first selected device: the whole of x up, one
// normalize_batch_run, the wanted tables back.  A collection without a row touches no device.
int host_normalize_batch(const void *x, int dtype, const long long *seg_off, int nseg, int dim, float *out_f32,
                         uint8_t *out_u8) {
  NormalizeBatchPlan p;
  SPV_TRY(normalize_batch_plan(seg_off, nseg, dim, dtype, &p));
  if (!out_f32 && !out_u8) return set_error(SPV_ERR_INVALID, "neither the float32 nor the uint8 table is wanted");
  if (p.total_rows == 0) return SPV_OK;
  if (!x) return set_error(SPV_ERR_INVALID, "null pointer");
  hipStream_t st;
  SPV_TRY(host_begin(device_list()[0], &st));
  const size_t xb = (size_t)p.total_rows * dim * (dtype == SPV_NORMALIZE_U8 ? 1 : sizeof(float));
  const size_t ub = (size_t)p.total_rows * ((dim + 15) / 16 * 16), fb = ub * sizeof(float);
  DevBuf dx, df, du, ws;
  SPV_TRY(dx.upload(x, xb, st));
  if (out_f32) SPV_TRY(df.alloc(fb));
  if (out_u8) SPV_TRY(du.alloc(ub));
  SPV_TRY(ws.alloc(p.total_bytes));
  SPV_TRY(normalize_batch_run(dx.p, dtype, seg_off, nseg, dim, out_f32 ? df.as<float>() : nullptr,
                              out_u8 ? du.as<uint8_t>() : nullptr, ws.p, p.total_bytes, st));
  if (out_f32) SPV_TRY(df.copy_out(out_f32, fb, st));
  if (out_u8) SPV_TRY(du.copy_out(out_u8, ub, st));
  SPV_HIP_CHECK(hipStreamSynchronize(st));
  return SPV_OK;
}

// Hyperplanes as the reference draws them (src/CascadingHashNn.h:86-100):
// one std::mt19937 stream, std::normal_distribution<float>(0,1), table-major,
// then dim (i), then bit (j).
void fill_hash_dict(uint32_t seed, int dim, int m, int n, float *dict) {
  std::mt19937 gen(seed);
  std::normal_distribution<float> normal(0.f, 1.f);
  const size_t total = (size_t)n * dim * m;
  for (size_t e = 0; e < total; ++e) dict[e] = normal(gen);
}

// The only place that touches NdArray members besides the callers' m_data reads.  With the in-repo
// header (include/NdArray.h) the item size fixed by the Python constructor is cross-checked; when
// built against the upstream ctypes_ndarray header (make NDARRAY_INC=...) define
// SPV_NDARRAY_ITEMSIZE(arr) to its item-size member if it has one, else nothing is checked and the
// upstream ndarray_alloc sizes the buffer as it always did for the reference.
#if !defined(SPECTAVI_EXTERNAL_NDARRAY) && !defined(SPV_NDARRAY_ITEMSIZE)
#define SPV_NDARRAY_ITEMSIZE(arr) ((arr)->m_itemsize)
#endif
int alloc_out(NdArray *arr, size_t rows, size_t cols, int itemsize, size_t depth = 0) {
  if (!arr) return set_error(SPV_ERR_INVALID, "null NdArray");
#ifdef SPV_NDARRAY_ITEMSIZE
  if ((int)SPV_NDARRAY_ITEMSIZE(arr) != itemsize)
    return set_error(SPV_ERR_INVALID, "NdArray itemsize %d, expected %d", (int)SPV_NDARRAY_ITEMSIZE(arr), itemsize);
#else
  (void)itemsize;
#endif
  if (depth) ndarray_set_size3(arr, rows, cols, depth);
  else ndarray_set_size(arr, rows, cols);
  ndarray_alloc(arr);
  if (!arr->m_data) return set_error(SPV_ERR_NOMEM, "ndarray_alloc failed");
  return SPV_OK;
}

}  // namespace
}  // namespace spv

using namespace spv;

extern "C" {

// ---- NdArray ------------------------------------------------------------------------
// In-repo implementation of the helpers the reference takes from its ctypes_ndarray submodule;
// compiled out when the library is built against the upstream header and library
// (make NDARRAY_INC=... NDARRAY_LIB=...), which then provide them.
#ifndef SPECTAVI_EXTERNAL_NDARRAY
void ndarray_set_size(NdArray *arr, size_t d0, size_t d1) {
  arr->m_ndim = 2;
  arr->m_shape[0] = d0;
  arr->m_shape[1] = d1;
  arr->m_shape[2] = arr->m_shape[3] = 1;
}
void ndarray_set_size3(NdArray *arr, size_t d0, size_t d1, size_t d2) {
  arr->m_ndim = 3;
  arr->m_shape[0] = d0;
  arr->m_shape[1] = d1;
  arr->m_shape[2] = d2;
  arr->m_shape[3] = 1;
}
int ndarray_alloc(NdArray *arr) {
  size_t n = (size_t)(arr->m_itemsize > 0 ? arr->m_itemsize : 1);
  for (int i = 0; i < arr->m_ndim; ++i) n *= arr->m_shape[i];
  if (arr->m_data) free(arr->m_data);
  arr->m_data = malloc(n ? n : 1);
  return arr->m_data ? 0 : 1;
}
void ndarray_free(NdArray *arr) {
  if (arr && arr->m_data) {
    free(arr->m_data);
    arr->m_data = nullptr;
  }
}
#endif  // !SPECTAVI_EXTERNAL_NDARRAY

// ---- status -------------------------------------------------------------------------
int spv_last_status(void) { return g_status; }
const char *spv_last_error(void) { return g_message; }
const char *spv_version(void) { return "spectavi_amd 0.1 (gfx950)"; }
int spv_device_count(void) {
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) return 0;
  return c;
}
int spv_set_device(int device) { return spv_set_devices(&device, 1); }
int spv_set_devices(const int *devices, int count) {
  clear_error();
  if (count < 1 || !devices) return set_error(SPV_ERR_INVALID, "need at least one device");
  for (int i = 0; i < count; ++i)
    if (devices[i] < 0) return set_error(SPV_ERR_INVALID, "device %d", devices[i]);
  set_device_list(devices, count);
  return SPV_OK;
}

int spv_set_gather_mode(int mode) {
  clear_error();
  if (mode != SPV_GATHER_AUTO && mode != SPV_GATHER_DIRECT && mode != SPV_GATHER_RCCL && mode != SPV_GATHER_PEERCOPY)
    return set_error(SPV_ERR_INVALID, "gather mode %d", mode);
  set_gather_mode(mode);
  return SPV_OK;
}

int spv_l1k2_set_prune(int mode) {
  clear_error();
  if (mode != SPV_L1K2_PRUNE_AUTO && mode != SPV_L1K2_PRUNE_OFF && mode != SPV_L1K2_PRUNE_ON)
    return set_error(SPV_ERR_INVALID, "prune mode %d", mode);
  l1k2_set_prune(mode);
  return SPV_OK;
}

int spv_l1k2_get_prune(void) { return l1k2_get_prune(); }

int spv_l1k2_prune_stats(unsigned long long out[3]) {
  clear_error();
  if (!out) return set_error(SPV_ERR_INVALID, "null output");
  return guard([&] { return l1k2_prune_last_stats(out); });
}

int spv_l1k2_bound_table(int8_t phi[256][4], int *p, int *m) {
  clear_error();
  if (!phi || !p || !m) return set_error(SPV_ERR_INVALID, "null output");
  const L1K2Bound &b = l1k2_bound();
  for (int a = 0; a < 256; ++a)
    for (int f = 0; f < 4; ++f) phi[a][f] = b.phi[a][f];
  *p = b.p;
  *m = b.m;
  return b.ok ? SPV_OK : set_error(SPV_ERR_INTERNAL, "the L1 bound table failed its own check");
}

int spv_l1k2_set_bound(int which) {
  clear_error();
  if (which != SPV_L1K2_BOUND_DEFAULT && which != SPV_L1K2_BOUND_RECIPE && which != SPV_L1K2_BOUND_TUNED)
    return set_error(SPV_ERR_INVALID, "bound table %d", which);
  l1k2_set_bound(which);
  return SPV_OK;
}

int spv_l1k2_get_bound(void) { return l1k2_get_bound(); }

int spv_l1k2_set_prune_form(int form) {
  clear_error();
  if (form != SPV_L1K2_PRUNE_FORM_DEFAULT && form != SPV_L1K2_PRUNE_FORM_NARROW && form != SPV_L1K2_PRUNE_FORM_WIDE)
    return set_error(SPV_ERR_INVALID, "bound kernel form %d", form);
  l1k2_set_prune_form(form);
  return SPV_OK;
}

int spv_l1k2_get_prune_form(void) { return l1k2_get_prune_form(); }

int spv_l1k2_prune_form_of(int xrows, int yrows, int dim) {
  if (!l1k2_shape_ok(xrows, yrows, dim)) return -1;
  const L1K2Plan p = l1k2_plan(xrows, yrows, dim);
  return p.dim_pad >= 0 && p.path == kL1K2Bound ? p.form : -1;
}

int spv_l1k2_bound_table_of(int which, int8_t phi[256][4], int *p, int *m) {
  clear_error();
  if (!phi || !p || !m) return set_error(SPV_ERR_INVALID, "null output");
  if (which != SPV_L1K2_BOUND_RECIPE && which != SPV_L1K2_BOUND_TUNED) return set_error(SPV_ERR_INVALID, "bound table %d", which);
  const L1K2Bound &b = l1k2_bound_of(which);
  for (int a = 0; a < 256; ++a)
    for (int f = 0; f < 4; ++f) phi[a][f] = b.phi[a][f];
  *p = b.p;
  *m = b.m;
  return b.ok ? SPV_OK : set_error(SPV_ERR_INTERNAL, "the L1 bound table failed its own check");
}

int spv_l1k2_set_prune_matrix(int matrix) {
  clear_error();
  if (matrix != SPV_L1K2_PRUNE_MATRIX_DEFAULT && matrix != SPV_L1K2_PRUNE_MATRIX_I8 && matrix != SPV_L1K2_PRUNE_MATRIX_FP6)
    return set_error(SPV_ERR_INVALID, "bound matrix format %d", matrix);
  l1k2_set_prune_matrix(matrix);
  return SPV_OK;
}

int spv_l1k2_get_prune_matrix(void) { return l1k2_get_prune_matrix(); }

int spv_l1k2_prune_matrix_of(int xrows, int yrows, int dim) {
  if (!l1k2_shape_ok(xrows, yrows, dim)) return -1;
  const L1K2Plan p = l1k2_plan(xrows, yrows, dim);
  return p.dim_pad >= 0 && p.path == kL1K2Bound ? p.matrix : -1;
}

int spv_l1k2_bound6_table(int8_t k[256][5], int *p, int *m) {
  clear_error();
  if (!k || !p || !m) return set_error(SPV_ERR_INVALID, "null output");
  const L1K2Bound6 &b = l1k2_bound6();
  for (int a = 0; a < 256; ++a)
    for (int f = 0; f < 5; ++f) k[a][f] = b.k[a][f];
  *p = b.p;
  *m = b.m;
  return b.ok ? SPV_OK : set_error(SPV_ERR_INTERNAL, "the FP6 L1 bound table failed its own check");
}

void spv_release_cached_memory(void) { release_transfer_caches(); }

void spv_profile_enable(int on) {
  g_prof_on.store(on != 0);
  if (!on) {  // release the events of everything that has finished; totals stay readable
    std::lock_guard<std::mutex> lk(g_prof_mutex);
    for (auto &kv : g_prof) prof_fold(kv.second, false);
  }
}

void spv_profile_reset(void) {
  std::lock_guard<std::mutex> lk(g_prof_mutex);
  for (auto &kv : g_prof)
    for (auto &ev : kv.second.pending) {
      (void)hipEventDestroy(ev.first);
      (void)hipEventDestroy(ev.second);
    }
  g_prof.clear();
}

int spv_profile_read(const char *kernel, long long *launches, double *total_ms) {
  clear_error();
  if (!kernel || !launches || !total_ms) return set_error(SPV_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> lk(g_prof_mutex);
  *launches = 0;
  *total_ms = 0.0;
  auto it = g_prof.find(kernel);
  if (it == g_prof.end()) return SPV_OK;
  prof_fold(it->second, true);
  *launches = it->second.launches;
  *total_ms = it->second.total_ms;
  return SPV_OK;
}

// ---- reference-compatible symbols ---------------------------------------------------
void nn_bruteforcel1k2(const uint8_t *x, const uint8_t *y, int xrows, int yrows, int dim,
                       int nthreads, NdArray *outidx, NdArray *outdist) {
  (void)nthreads;  // OpenMP team size in the reference; the GPU path has no use for it
  clear_error();
  if (yrows < 0) {
    set_error(SPV_ERR_INVALID, "negative row count");
    return;
  }
  (void)host_guard([&] {
    SPV_TRY(alloc_out(outidx, (size_t)yrows, 2, (int)sizeof(size_t)));
    SPV_TRY(alloc_out(outdist, (size_t)yrows, 2, (int)sizeof(int)));
    return host_l1k2(x, y, xrows, yrows, dim, static_cast<uint64_t *>(outidx->m_data),
                     static_cast<int32_t *>(outdist->m_data));
  });
}

static void nn_bruteforce_ref(const void *x, const void *y, int is_int, int xrows, int yrows, int dim, int k,
                              float p, float mu, NdArray *outidx, NdArray *outdist) {
  (void)mu;  // the result is always exact (include/spectavi_amd.h)
  clear_error();
  if (bruteforce_check(xrows, yrows, dim, k, p) != SPV_OK) return;
  (void)host_guard([&] {
    SPV_TRY(alloc_out(outidx, (size_t)yrows, (size_t)k, (int)sizeof(size_t)));
    SPV_TRY(alloc_out(outdist, (size_t)yrows, (size_t)k, 4));
    return host_bruteforce(x, y, is_int, xrows, yrows, dim, k, p, static_cast<uint64_t *>(outidx->m_data),
                           outdist->m_data);
  });
}

void nn_bruteforce(const float *x, const float *y, int xrows, int yrows, int dim, int k, float p, float mu,
                   NdArray *outidx, NdArray *outdist) {
  nn_bruteforce_ref(x, y, 0, xrows, yrows, dim, k, p, mu, outidx, outdist);
}

void nn_bruteforcei(const int *x, const int *y, int xrows, int yrows, int dim, int k, float p, float mu,
                    NdArray *outidx, NdArray *outdist) {
  nn_bruteforce_ref(x, y, 1, xrows, yrows, dim, k, p, mu, outidx, outdist);
}

void ann_hnswlib(const float *x, const float *y, int xrows, int yrows, int dim, int k, NdArray *out) {
  clear_error();
  if (ann_check(xrows, yrows, dim, k, 0) != SPV_OK) return;
  (void)host_guard([&] {
    SPV_TRY(alloc_out(out, (size_t)yrows, (size_t)k, (int)sizeof(size_t)));
    return host_ann(x, y, xrows, yrows, dim, k, 0, static_cast<uint64_t *>(out->m_data), nullptr);
  });
}

void nn_kmedians(const float *x, const float *y, int xrows, int yrows, int dim, int nmx, int nmy, int c, int k,
                 NdArray *outidx, NdArray *outdist) {
  (void)nmx, (void)nmy, (void)c;  // cluster counts of the reference's filter; the result here is exact
  nn_bruteforce_ref(x, y, 0, xrows, yrows, dim, k, 1.f, 0.f, outidx, outdist);
}

void kmedians(const float *x, int xrows, int dim, int k) {
  clear_error();
  if (!x || xrows < 0 || dim < 1 || k < 1) set_error(SPV_ERR_INVALID, "kmedians: bad arguments");
}

void nn_cascading_hash(const float *x, const float *y, int xrows, int yrows, int dim, int k,
                       int hash_bit_rate, int num_hash_tables, int num_candidate_neighbours,
                       NdArray *outidx, NdArray *outdist) {
  clear_error();
  if (k != 2) {
    set_error(SPV_ERR_INVALID, "k=%d: only k=2 is defined (reference writes exactly two columns)", k);
    return;
  }
  (void)host_guard([&] {
    SPV_TRY(check_cascade_args(xrows, yrows, dim, hash_bit_rate, num_hash_tables, num_candidate_neighbours));
    SPV_TRY(alloc_out(outidx, (size_t)yrows, 2, (int)sizeof(size_t)));
    SPV_TRY(alloc_out(outdist, (size_t)yrows, 2, (int)sizeof(float)));
    uint32_t seed;
    {
      std::lock_guard<std::mutex> lk(g_seed_mutex);
      const char *e = getenv("SPECTAVI_HASH_SEED");
      if (g_seed_fixed)
        seed = g_seed;
      else if (e && *e)
        seed = (uint32_t)strtoul(e, nullptr, 0);
      else
        seed = std::random_device{}();  // as reference src/CascadingHashNn.h:87-88
    }
    std::vector<float> dict((size_t)num_hash_tables * dim * hash_bit_rate);
    fill_hash_dict(seed, dim, hash_bit_rate, num_hash_tables, dict.data());
    return host_cascade(x, y, xrows, yrows, dim, hash_bit_rate, num_hash_tables, num_candidate_neighbours,
                        dict.data(), static_cast<uint64_t *>(outidx->m_data),
                        static_cast<float *>(outdist->m_data), nullptr);
  });
}

void dlt_triangulate(const double *P0, const double *P1, int npt, const double *x,
                     const double *xp, double *dst) {
  (void)host_api([&] { return host_dlt(P0, P1, npt, x, xp, dst, false); });
}

void dlt_reprojection_error(const double *P0, const double *P1, int npt, const double *x,
                            const double *xp, double *dst) {
  (void)host_api([&] { return host_dlt(P0, P1, npt, x, xp, dst, true); });
}

void image_pair_rectification(const double *P0, const double *P1, const double *im0, const double *im1, int wid,
                              int hgt, int nchan, double sampling_factor, NdArray *rectified0, NdArray *rectified1,
                              NdArray *rectified_idx0, NdArray *rectified_idx1) {
  clear_error();
  int shape[3];
  if (rectify_shape(wid, hgt, nchan, sampling_factor, shape) != SPV_OK) return;
  (void)host_guard([&] {
    const size_t rows = (size_t)shape[0], cols = (size_t)shape[1], depth = nchan > 1 ? (size_t)nchan : 0;
    SPV_TRY(alloc_out(rectified0, rows, cols, (int)sizeof(double), depth));
    SPV_TRY(alloc_out(rectified1, rows, cols, (int)sizeof(double), depth));
    SPV_TRY(alloc_out(rectified_idx0, rows, cols, (int)sizeof(int32_t)));
    SPV_TRY(alloc_out(rectified_idx1, rows, cols, (int)sizeof(int32_t)));
    return host_rectify(P0, P1, im0, im1, wid, hgt, nchan, sampling_factor,
                        static_cast<double *>(rectified0->m_data), static_cast<double *>(rectified1->m_data),
                        static_cast<int32_t *>(rectified_idx0->m_data), static_cast<int32_t *>(rectified_idx1->m_data));
  });
}

void sift_filter(const float *im, int wid, int hgt, NdArray *out) {
  (void)host_api([&] {
    if (!out) return set_error(SPV_ERR_INVALID, "null NdArray");
    return host_sift(im, wid, hgt, out, nullptr, 0, nullptr);
  });
}

void *sift_filter_batch_create(void) {
  clear_error();
  return new (std::nothrow) SiftBatch();
}

void sift_filter_batch_register_image(void *sfb, const float *im, int wid, int hgt, NdArray *out) {
  (void)api([&] {
    if (!sfb) return set_error(SPV_ERR_INVALID, "null batch");
    static_cast<SiftBatch *>(sfb)->items.push_back({im, wid, hgt, out});
    return SPV_OK;
  });
}

// nthread is accepted and ignored: the images run one after another on the device.  Every image is
// processed; the status is the first failure's.
void sift_filter_batch_process(void *sfb, int nthread) {
  (void)nthread;
  (void)host_api([&] {
    if (!sfb) return set_error(SPV_ERR_INVALID, "null batch");
    int first = SPV_OK;
    std::string msg;
    for (const SiftBatch::Item &it : static_cast<SiftBatch *>(sfb)->items) {
      const int s = it.out ? host_sift(it.im, it.wid, it.hgt, it.out, nullptr, 0, nullptr)
                           : set_error(SPV_ERR_INVALID, "null NdArray");
      if (s != SPV_OK && first == SPV_OK) {
        first = s;
        msg = spv_last_error();
      }
    }
    return first == SPV_OK ? SPV_OK : set_error(first, "%s", msg.c_str());
  });
}

void sift_filter_batch_destroy(void *sfb) { delete static_cast<SiftBatch *>(sfb); }

// ---- host-pointer status variants ---------------------------------------------------
int spv_nn_bruteforcel1k2(const uint8_t *x, const uint8_t *y, int xrows, int yrows, int dim,
                          uint64_t *idx, int32_t *dist) {
  return host_api([&] { return host_l1k2(x, y, xrows, yrows, dim, idx, dist); });
}

int spv_nn_bruteforcel1k2_batch(const uint8_t *desc, const long long *seg_off, int nseg, int dim, const int32_t *pairs,
                                int npairs, uint64_t *idx, int32_t *dist) {
  return host_api([&] { return host_l1k2_batch(desc, seg_off, nseg, dim, pairs, npairs, idx, dist); });
}

int spv_nn_bruteforcel1k2_guided_batch(const uint8_t *desc, const float *geom, const long long *seg_off, int nseg, int dim,
                                       const int32_t *pairs, int npairs, const double *lines, double max_dist,
                                       uint64_t *idx, int32_t *dist, int32_t *ncand) {
  return host_api([&] {
    return host_l1k2_guided_batch(desc, geom, seg_off, nseg, dim, pairs, npairs, lines, max_dist, idx, dist, ncand);
  });
}

int spv_nn_bruteforce(const void *x, const void *y, int is_int, int xrows, int yrows, int dim, int k, float p,
                      uint64_t *idx, void *dist) {
  return host_api([&] { return host_bruteforce(x, y, is_int, xrows, yrows, dim, k, p, idx, dist); });
}

int spv_ann_l2(const float *x, const float *y, int xrows, int yrows, int dim, int k, int ncand, uint64_t *idx,
               float *dist) {
  return host_api([&] { return host_ann(x, y, xrows, yrows, dim, k, ncand, idx, dist); });
}

int spv_nn_cascading_hash(const float *x, const float *y, int xrows, int yrows, int dim, int m,
                          int n, int g, const float *dict, uint64_t *idx, float *dist,
                          int32_t *ncand) {
  return host_api([&] { return host_cascade(x, y, xrows, yrows, dim, m, n, g, dict, idx, dist, ncand); });
}

int spv_nn_cascading_hash_batch(const float *rows, const long long *seg_off, int nseg, int dim, int m, int n, int g,
                                const int32_t *pairs, int npairs, const float *dict, uint64_t *idx, float *dist,
                                int32_t *ncand) {
  return host_api([&] { return host_cascade_batch(rows, seg_off, nseg, dim, m, n, g, pairs, npairs, dict, idx, dist, ncand); });
}

int spv_generate_hash_dict(uint32_t seed, int dim, int m, int n, float *dict) {
  clear_error();
  if (dim <= 0 || m <= 0 || n <= 0 || !dict) return set_error(SPV_ERR_INVALID, "bad dict shape");
  fill_hash_dict(seed, dim, m, n, dict);
  return SPV_OK;
}

void spv_set_hash_seed(uint32_t seed, int use_fixed) {
  std::lock_guard<std::mutex> lk(g_seed_mutex);
  g_seed = seed;
  g_seed_fixed = use_fixed != 0;
}

int spv_dlt_triangulate(const double *P0, const double *P1, int npt, const double *x,
                        const double *xp, double *dst) {
  return host_api([&] { return host_dlt(P0, P1, npt, x, xp, dst, false); });
}
int spv_normalize(const float *x, int rows, int dim, float *out_f32, uint8_t *out_u8) {
  return host_api([&] { return host_normalize(x, rows, dim, out_f32, out_u8); });
}
size_t spv_normalize_workspace_bytes(int dim) { return dim <= 0 ? 0 : normalize_workspace_bytes(dim); }
size_t spv_normalize_workspace_bytes_rows(int rows, int dim) {
  return (dim <= 0 || rows < 0) ? 0 : normalize_workspace_bytes_rows(rows, dim);
}
int spv_normalize_device(const float *d_x, int rows, int dim, float *d_out_f32, uint8_t *d_out_u8,
                         void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] { return normalize_run(d_x, rows, dim, d_out_f32, d_out_u8, d_ws, ws_bytes, static_cast<hipStream_t>(stream)); });
}

int spv_normalize_batch(const void *x, int dtype, const long long *seg_off, int nseg, int dim, float *out_f32,
                        uint8_t *out_u8) {
  return host_api([&] { return host_normalize_batch(x, dtype, seg_off, nseg, dim, out_f32, out_u8); });
}
int spv_normalize_batch_plan(const long long *seg_off, int nseg, int dim, int dtype, int compute_units, long long out[4],
                             int32_t *items, long long items_cap) {
  return api([&] {
    if (compute_units < 1 || !out || items_cap < 0) return set_error(SPV_ERR_INVALID, "bad arguments");
    NormalizeBatchPlan p;
    SPV_TRY(normalize_batch_plan(seg_off, nseg, dim, dtype, &p));
    out[0] = p.sets;
    out[1] = (long long)p.items.size();
    out[2] = (long long)p.total_bytes;
    out[3] = p.total_rows;
    export_items<3>(p.items, items, items_cap);
    return (int)SPV_OK;
  });
}
size_t spv_normalize_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, int dtype) {
  return plan_bytes<NormalizeBatchPlan>(&NormalizeBatchPlan::total_bytes,
                                        [&](NormalizeBatchPlan *p) { return normalize_batch_plan(seg_off, nseg, dim, dtype, p); });
}
int spv_normalize_batch_device(const void *d_x, int dtype, const long long *seg_off, int nseg, int dim, float *d_out_f32,
                               uint8_t *d_out_u8, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] {
    return normalize_batch_run(d_x, dtype, seg_off, nseg, dim, d_out_f32, d_out_u8, d_ws, ws_bytes,
                               static_cast<hipStream_t>(stream));
  });
}
int spv_sift_split(const float *table, int rows, float *geom, uint8_t *desc) {
  return host_api([&] { return host_sift_split(table, rows, geom, desc); });
}
int spv_sift_split_device(const float *d_table, int rows, float *d_geom, uint8_t *d_desc,
                          void *stream) {
  return api([&] { return sift_split_run(d_table, rows, d_geom, d_desc, static_cast<hipStream_t>(stream)); });
}
int spv_gather_match_coords_device(const float *d_geom_x, const float *d_geom_y,
                                   const int32_t *d_matches, const int32_t *d_count, int capacity,
                                   double *d_x0, double *d_x1, void *stream) {
  return api([&] { return gather_match_coords_run(d_geom_x, d_geom_y, d_matches, d_count, capacity, d_x0, d_x1,
                                                  static_cast<hipStream_t>(stream)); });
}
int spv_gather_match_coords_batch_device(const float *d_geom, const long long *seg_off, int nseg, const int32_t *pairs,
                                         int npairs, const int32_t *d_matches, const int32_t *d_count, int capacity,
                                         double *d_x0, double *d_x1, long long *d_pair_off, void *stream) {
  return api([&] {
    return gather_match_coords_batch_run(d_geom, seg_off, nseg, pairs, npairs, d_matches, d_count, capacity, d_x0, d_x1,
                                         d_pair_off, static_cast<hipStream_t>(stream));
  });
}
size_t spv_tracks_batch_workspace_bytes(long long total_rows, int capacity) {
  return (total_rows < 0 || total_rows >= (1ll << 31) || capacity < 0) ? 0 : tracks_batch_workspace_bytes(total_rows, capacity);
}
int spv_tracks_batch_device(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const int32_t *d_matches,
                            const int32_t *d_count, int capacity, const uint8_t *d_mask, int min_len, int accumulate,
                            int32_t *d_label, int32_t *d_track, long long *d_track_off, int32_t *d_members,
                            uint8_t *d_flags, int32_t *d_counts, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] {
    return tracks_batch_run(seg_off, nseg, pairs, npairs, d_matches, d_count, capacity, d_mask, min_len, accumulate, d_label,
                            d_track, d_track_off, d_members, d_flags, d_counts, d_ws, ws_bytes, static_cast<hipStream_t>(stream));
  });
}
int spv_tracks_batch(const long long *seg_off, int nseg, const int32_t *pairs, int npairs, const int32_t *matches, int count,
                     const uint8_t *mask, int min_len, int accumulate, int32_t *label, int32_t *track, long long *track_off,
                     int32_t *members, uint8_t *flags, int32_t *counts) {
  return host_api([&] {
    return host_tracks_batch(seg_off, nseg, pairs, npairs, matches, count, mask, min_len, accumulate, label, track, track_off,
                             members, flags, counts);
  });
}
int spv_tracks_triangulate_set_long(int L) {
  clear_error();
  if (L < 0) return set_error(SPV_ERR_INVALID, "longest lane-form track %d", L);
  tracks_triangulate_set_long(L);
  return SPV_OK;
}
int spv_tracks_triangulate_get_long(void) { return tracks_triangulate_get_long(); }
int spv_tracks_triangulate_plan(const long long *track_off, int ntracks, long long out[4]) {
  return api([&] {
    if (ntracks < 0 || !out) return set_error(SPV_ERR_INVALID, "bad arguments");
    SPV_TRY(check_offsets(track_off, ntracks, "track_off"));
    TracksTriangulatePlan pl;
    tracks_triangulate_plan(track_off, ntracks, &pl);
    out[0] = pl.lane_tracks;
    out[1] = pl.wave_tracks;
    out[2] = pl.lane_groups;
    out[3] = pl.longest;
    return (int)SPV_OK;
  });
}
int spv_tracks_triangulate_device(const float *d_geom, const long long *seg_off, int nseg, const double *cams,
                                  const int32_t *use_set, const long long *track_off, int ntracks, const int32_t *d_members,
                                  long long nmembers, double max_error, double *d_X, double *d_err, uint8_t *d_ok,
                                  int32_t *d_nused, void *stream) {
  return api([&] {
    return tracks_triangulate_run(d_geom, seg_off, nseg, cams, use_set, track_off, ntracks, d_members, nmembers, max_error, d_X,
                                  d_err, d_ok, d_nused, static_cast<hipStream_t>(stream));
  });
}
int spv_tracks_triangulate(const float *geom, const long long *seg_off, int nseg, const double *cams, const int32_t *use_set,
                           const long long *track_off, int ntracks, const int32_t *members, long long nmembers,
                           double max_error, double *X, double *err, uint8_t *ok, int32_t *nused) {
  return host_api([&] {
    return host_tracks_triangulate(geom, seg_off, nseg, cams, use_set, track_off, ntracks, members, nmembers, max_error, X, err,
                                   ok, nused);
  });
}
int spv_bundle_adjust_plan(const long long *track_off, int ntracks, const int32_t *members, const long long *seg_off, int nseg,
                           const int32_t *mode, long long out[5]) {
  return api([&] {
    if (ntracks < 0 || nseg < 0 || !out) return set_error(SPV_ERR_INVALID, "bad arguments");
    SPV_TRY(check_offsets(track_off, ntracks, "track_off"));
    if (members) SPV_TRY(check_offsets(seg_off, nseg, "seg_off"));
    BundleAdjustPlan pl;
    bundle_adjust_plan(track_off, ntracks, members, seg_off, nseg, mode, &pl);
    out[0] = pl.lane_tracks;
    out[1] = pl.wave_tracks;
    out[2] = pl.chunk;
    out[3] = pl.chunks;
    out[4] = pl.longest;
    return (int)SPV_OK;
  });
}
size_t spv_bundle_adjust_workspace_bytes(int nseg, int ntracks, long long nmembers) {
  return (nseg < 0 || ntracks < 0 || nmembers < 0) ? 0 : bundle_adjust_workspace_bytes(nseg, ntracks, nmembers);
}
int spv_bundle_adjust_device(const float *d_geom, const long long *seg_off, int nseg, const double *K, double *poses,
                             const int32_t *mode, const long long *track_off, int ntracks, const int32_t *d_members,
                             long long nmembers, double *d_X, const uint8_t *d_use, double huber, int max_steps, double lambda0,
                             double ftol, double gtol, double cg_tol, int cg_max, double *d_err, uint8_t *d_active, double *trace,
                             double *info, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] {
    const BundleAdjustOptions o{huber, lambda0, ftol, gtol, cg_tol, max_steps, cg_max};
    return bundle_adjust_run(d_geom, seg_off, nseg, K, poses, mode, track_off, ntracks, d_members, nmembers, d_X, d_use, o, d_err,
                             d_active, trace, info, d_ws, ws_bytes, static_cast<hipStream_t>(stream));
  });
}
int spv_bundle_adjust(const float *geom, const long long *seg_off, int nseg, const double *K, double *poses, const int32_t *mode,
                      const long long *track_off, int ntracks, const int32_t *members, long long nmembers, double *X,
                      const uint8_t *use, double huber, int max_steps, double lambda0, double ftol, double gtol, double cg_tol,
                      int cg_max, double *err, uint8_t *active, double *trace, double *info) {
  return host_api([&] {
    const BundleAdjustOptions o{huber, lambda0, ftol, gtol, cg_tol, max_steps, cg_max};
    return host_bundle_adjust(geom, seg_off, nseg, K, poses, mode, track_off, ntracks, members, nmembers, X, use, o, err, active,
                              trace, info);
  });
}
int spv_ratio_test(const uint64_t *idx, const void *dist, int dist_is_float, int yrows,
                   double min_ratio, int32_t *matches, int32_t *count) {
  return host_api([&] { return host_ratio(idx, dist, dist_is_float, yrows, min_ratio, matches, count); });
}
size_t spv_ratio_test_workspace_bytes(int yrows) { return yrows < 0 ? 0 : ratio_workspace_bytes(yrows); }
int spv_ratio_test_device(const uint64_t *d_idx, const void *d_dist, int dist_is_float, int yrows,
                          double min_ratio, int32_t *d_matches, int32_t *d_count, void *d_ws,
                          size_t ws_bytes, void *stream) {
  return api([&] { return ratio_run(d_idx, d_dist, dist_is_float, yrows, min_ratio, d_matches, d_count, d_ws, ws_bytes,
                                    static_cast<hipStream_t>(stream)); });
}
int spv_dlt_score_hypotheses(const double *P0, const double *P1s, int nhyp, int npt,
                             const double *x, const double *xp, double max_error,
                             int32_t *counts, uint8_t *mask) {
  return host_api([&] { return host_dlt_score(P0, P1s, nhyp, npt, x, xp, max_error, counts, mask); });
}
int spv_ransac_process_candidates(const double *Fs, int nF, const double *x0, const double *x1, int npt,
                                  double singular_value_ratio_allowed, double required_percent_inliers,
                                  double reprojection_error_allowed, int find_best_even_in_failure,
                                  int32_t *success, int32_t *inlier_count, int32_t *best_camera, double *best_P,
                                  double *gate_ratio, double *E, int32_t *counts4, uint8_t *inlier_mask) {
  return host_api([&] {
    return host_ransac_process(Fs, nF, x0, x1, npt, singular_value_ratio_allowed, required_percent_inliers,
                               reprojection_error_allowed, find_best_even_in_failure, success, inlier_count,
                               best_camera, best_P, gate_ratio, E, counts4, inlier_mask);
  });
}
int spv_seven_point(const double *x, const double *xp, int n, int32_t *nroot, double *Fs, double *basis) {
  return host_api([&] { return host_seven_point(x, xp, n, nroot, Fs, basis); });
}
int spv_seven_point_device(const double *d_x, const double *d_xp, int n, double *d_Fs, int32_t *d_nroot,
                           double *d_basis, void *stream) {
  return api([&] { return seven_point_run(d_x, d_xp, n, d_Fs, d_nroot, d_basis, static_cast<hipStream_t>(stream)); });
}
int spv_ransac_sample(unsigned long long seed, int npt, int ntries, int32_t *samples) {
  clear_error();
  if (npt < 10) return set_error(SPV_ERR_INVALID, "Supplied less than 10 point matches, unsupported.");
  if (ntries < 0 || (ntries > 0 && !samples)) return set_error(SPV_ERR_INVALID, "bad arguments");
  std::mt19937 gen(ransac_seed(seed));
  for (int t = 0; t < ntries; ++t) floyd_sample(gen, npt, samples + 7 * (size_t)t);
  return SPV_OK;
}
int spv_ransac_fit(const double *x0, const double *x1, int npt, double required_percent_inliers,
                   double reprojection_error_allowed, int maximum_tries, int find_best_even_in_failure,
                   double singular_value_ratio_allowed, unsigned long long seed, int32_t *success,
                   double *essential, double *camera, double *inlier_percent, int32_t *inlier_idx,
                   int32_t *n_inliers, int32_t *best_try, int32_t *best_root, int32_t *tries_run) {
  return host_api([&] {
    return host_ransac_fit(x0, x1, npt, required_percent_inliers, reprojection_error_allowed, maximum_tries,
                           find_best_even_in_failure, singular_value_ratio_allowed, nullptr, seed, success, essential,
                           camera, inlier_percent, inlier_idx, n_inliers, best_try, best_root, tries_run);
  });
}
int spv_ransac_fit_device(const double *d_x0, const double *d_x1, int npt, double required_percent_inliers,
                          double reprojection_error_allowed, int maximum_tries, int find_best_even_in_failure,
                          double singular_value_ratio_allowed, unsigned long long seed, const int32_t *samples,
                          int32_t *success, double *essential, double *camera, double *inlier_percent,
                          int32_t *inlier_idx, int32_t *n_inliers, int32_t *best_try, int32_t *best_root,
                          int32_t *tries_run, void *stream) {
  return api([&] {
    return host_ransac_fit(d_x0, d_x1, npt, required_percent_inliers, reprojection_error_allowed, maximum_tries,
                           find_best_even_in_failure, singular_value_ratio_allowed, samples, seed, success, essential,
                           camera, inlier_percent, inlier_idx, n_inliers, best_try, best_root, tries_run, true,
                           static_cast<hipStream_t>(stream));
  });
}
int spv_ransac_fit_samples(const double *x0, const double *x1, int npt, double required_percent_inliers,
                           double reprojection_error_allowed, const int32_t *samples, int ntries,
                           int find_best_even_in_failure, double singular_value_ratio_allowed, int32_t *success,
                           double *essential, double *camera, double *inlier_percent, int32_t *inlier_idx,
                           int32_t *n_inliers, int32_t *best_try, int32_t *best_root, int32_t *tries_run) {
  clear_error();
  if (ntries > 0 && !samples) return set_error(SPV_ERR_INVALID, "null samples");
  return host_guard([&] {
    return host_ransac_fit(x0, x1, npt, required_percent_inliers, reprojection_error_allowed, ntries,
                           find_best_even_in_failure, singular_value_ratio_allowed, samples, 0, success, essential,
                           camera, inlier_percent, inlier_idx, n_inliers, best_try, best_root, tries_run);
  });
}

// ---- the reference's own symbols for this path (src/Spectavi.cpp:14-36, :70-87) ------------
void seven_point_algorithm(const double *x, const double *xp, int *nroot, double *dst) {
  clear_error();
  if (!nroot || !dst) {
    set_error(SPV_ERR_INVALID, "null pointer");
    return;
  }
  *nroot = 0;
  int32_t nr = 0;
  double Fs[27];
  if (host_guard([&] { return host_seven_point(x, xp, 1, &nr, Fs, nullptr); }) != SPV_OK) return;
  *nroot = nr;
  memcpy(dst, Fs, (size_t)nr * 9 * sizeof(double));  // only the roots found are written, as in the reference
}

void ransac_fitter(const double *x0, const double *x1, int npt, double required_percent_inliers,
                   double reprojection_error_allowed, int maximum_tries, bool find_best_even_in_failure,
                   double singular_value_ratio_allowed, bool progressbar, bool *success, NdArray *essential,
                   NdArray *camera, double *inlier_percent, NdArray *inlier_idx) {
  (void)progressbar;  // the reference draws a text bar on stdout per try; tries run in batches here
  clear_error();
  if (!success || !inlier_percent) {
    set_error(SPV_ERR_INVALID, "null pointer");
    return;
  }
  *success = false;
  *inlier_percent = 0.0;
  host_guard([&] {
    SPV_TRY(check_fit_args(x0, x1, npt, maximum_tries));
    int32_t ok = 0, n = 0, bt = -1;
    double F[9], P[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, pct = 0.0;  // Camera(): Identity(3,4), src/Camera.h:27
    std::vector<int32_t> idx((size_t)npt);
    SPV_TRY(host_ransac_fit(x0, x1, npt, required_percent_inliers, reprojection_error_allowed, maximum_tries,
                            find_best_even_in_failure ? 1 : 0, singular_value_ratio_allowed, nullptr, 0, &ok, F, P, &pct,
                            idx.data(), &n, &bt, nullptr, nullptr));
    // ndarray_copy_matrix of the fitter's members (src/Spectavi.cpp:82-86): an untouched
    // m_best_fit_essential_matrix / m_inlier_idx is a 0 x 0 matrix
    const bool found = bt >= 0;
    SPV_TRY(alloc_out(essential, found ? 3 : 0, found ? 3 : 0, sizeof(double)));
    if (found) memcpy(essential->m_data, F, sizeof(F));
    SPV_TRY(alloc_out(camera, 3, 4, sizeof(double)));
    memcpy(camera->m_data, P, sizeof(P));
    SPV_TRY(alloc_out(inlier_idx, found ? (size_t)n : 0, found ? 1 : 0, sizeof(int32_t)));
    if (found && n > 0) memcpy(inlier_idx->m_data, idx.data(), (size_t)n * sizeof(int32_t));
    *success = ok != 0;
    *inlier_percent = pct;
    return (int)SPV_OK;
  });
}

size_t spv_ransac_workspace_bytes(int nF, long long npt, int want_mask) {
  return (nF < 0 || npt < 0) ? 0 : ransac_workspace_bytes(nF, npt, want_mask != 0);
}
int spv_ransac_process_candidates_device(const double *d_Fs, int nF, long long npt, const double *d_x0,
                                         const double *d_x1, double singular_value_ratio_allowed,
                                         double required_percent_inliers, double reprojection_error_allowed,
                                         int find_best_even_in_failure, int32_t *d_success, int32_t *d_inlier_count,
                                         int32_t *d_best_camera, double *d_best_P, double *d_gate_ratio, double *d_E,
                                         int32_t *d_counts4, uint8_t *d_inlier_mask, void *d_ws, size_t ws_bytes,
                                         void *stream) {
  return api([&] {
    return ransac_process_run(d_Fs, nF, npt, d_x0, d_x1, singular_value_ratio_allowed, required_percent_inliers,
                              reprojection_error_allowed, find_best_even_in_failure, d_success, d_inlier_count,
                              d_best_camera, d_best_P, d_gate_ratio, d_E, d_counts4, d_inlier_mask, d_ws, ws_bytes,
                              static_cast<hipStream_t>(stream));
  });
}
int spv_dlt_score_hypotheses_device(const double *P0, const double *d_P1s, int nhyp,
                                    long long npt, const double *d_x, const double *d_xp,
                                    double max_error, int32_t *d_counts, uint8_t *d_mask,
                                    void *stream) {
  return api([&] { return dlt_score_run(P0, d_P1s, nhyp, npt, d_x, d_xp, max_error, d_counts, d_mask, nullptr, 0,
                                        static_cast<hipStream_t>(stream)); });
}
size_t spv_dlt_score_workspace_bytes(int nhyp, long long npt) { return dlt_score_workspace_bytes(nhyp, npt); }
int spv_dlt_score_hypotheses_device_ws(const double *P0, const double *d_P1s, int nhyp, long long npt,
                                       const double *d_x, const double *d_xp, double max_error,
                                       int32_t *d_counts, uint8_t *d_mask, void *d_ws, size_t ws_bytes,
                                       void *stream) {
  return api([&] { return dlt_score_run(P0, d_P1s, nhyp, npt, d_x, d_xp, max_error, d_counts, d_mask, d_ws,
                                        ws_bytes, static_cast<hipStream_t>(stream)); });
}
int spv_ransac_fit_batch(const double *x0, const double *x1, const long long *pair_off, int npairs,
                         double required_percent_inliers, double reprojection_error_allowed, int maximum_tries,
                         int find_best_even_in_failure, double singular_value_ratio_allowed, const int32_t *samples,
                         const unsigned long long *seeds, int32_t *success, double *essential, double *camera,
                         double *inlier_percent, int32_t *inlier_idx, int32_t *n_inliers, int32_t *best_try,
                         int32_t *best_root, int32_t *tries_run) {
  return host_api([&] {
    return host_ransac_fit_batch(x0, x1, pair_off, npairs, required_percent_inliers, reprojection_error_allowed,
                                 maximum_tries, find_best_even_in_failure, singular_value_ratio_allowed, samples, seeds,
                                 success, essential, camera, inlier_percent, inlier_idx, n_inliers, best_try, best_root,
                                 tries_run);
  });
}
int spv_ransac_fit_batch_device(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs,
                                double required_percent_inliers, double reprojection_error_allowed, int maximum_tries,
                                int find_best_even_in_failure, double singular_value_ratio_allowed,
                                const int32_t *samples, const unsigned long long *seeds, int32_t *success,
                                double *essential, double *camera, double *inlier_percent, int32_t *inlier_idx,
                                int32_t *n_inliers, int32_t *best_try, int32_t *best_root, int32_t *tries_run,
                                uint8_t *d_inlier_mask, void *stream) {
  return api([&] {
    return ransac_fit_batch_run(d_x0, d_x1, pair_off, npairs, required_percent_inliers, reprojection_error_allowed,
                                maximum_tries, find_best_even_in_failure, singular_value_ratio_allowed, samples, seeds,
                                success, essential, camera, inlier_percent, inlier_idx, n_inliers, best_try, best_root,
                                tries_run, d_inlier_mask, static_cast<hipStream_t>(stream));
  });
}
int spv_ransac_fit_batch_plan(const long long *pair_off, int npairs, int maximum_tries, int compute_units,
                              long long out[4], int32_t *items, long long items_cap) {
  return api([&] {
    SPV_TRY(ransac_batch_check(pair_off, npairs, maximum_tries, nullptr));
    return fit_batch_plan(ransac_batch_first_round, 3, pair_off, npairs, maximum_tries, compute_units, out, items, items_cap);
  });
}
int spv_resect_gather_device(const float *d_geom, const int32_t *d_track, const long long *seg_off, int nseg,
                             const int32_t *views, int nviews, const double *d_X, const uint8_t *d_ok, int ntracks,
                             long long capacity, double *d_x, double *d_Xw, int32_t *d_rows, long long *d_view_off,
                             long long *view_off, void *stream) {
  return api([&] {
    return resect_gather_run(d_geom, d_track, seg_off, nseg, views, nviews, d_X, d_ok, ntracks, capacity, d_x, d_Xw, d_rows,
                             d_view_off, view_off, static_cast<hipStream_t>(stream));
  });
}
int spv_resect_fit_batch(const double *x, const double *Xw, const long long *view_off, int nviews,
                         double required_percent_inliers, double max_error, int maximum_tries,
                         int find_best_even_in_failure, const int32_t *samples, const unsigned long long *seeds,
                         int32_t *success, double *camera, double *inlier_percent, int32_t *n_inliers, int32_t *best_try,
                         int32_t *tries_run, uint8_t *inlier_mask, double *try_cameras, int32_t *try_inliers) {
  return host_api([&] {
    return host_resect_fit_batch(x, Xw, view_off, nviews, required_percent_inliers, max_error, maximum_tries,
                                 find_best_even_in_failure, samples, seeds, success, camera, inlier_percent, n_inliers,
                                 best_try, tries_run, inlier_mask, try_cameras, try_inliers);
  });
}
int spv_resect_fit_batch_device(const double *d_x, const double *d_Xw, const long long *view_off, int nviews,
                                double required_percent_inliers, double max_error, int maximum_tries,
                                int find_best_even_in_failure, const int32_t *samples, const unsigned long long *seeds,
                                int32_t *success, double *camera, double *inlier_percent, int32_t *n_inliers,
                                int32_t *best_try, int32_t *tries_run, uint8_t *d_inlier_mask, double *d_try_cameras,
                                int32_t *d_try_inliers, void *stream) {
  return api([&] {
    return resect_fit_batch_run(d_x, d_Xw, view_off, nviews, required_percent_inliers, max_error, maximum_tries,
                                find_best_even_in_failure, samples, seeds, success, camera, inlier_percent, n_inliers,
                                best_try, tries_run, d_inlier_mask, d_try_cameras, d_try_inliers,
                                static_cast<hipStream_t>(stream));
  });
}
int spv_resect_fit_batch_plan(const long long *view_off, int nviews, int maximum_tries, int compute_units, long long out[4],
                              int32_t *items, long long items_cap) {
  return api([&] {
    SPV_TRY(resect_check(view_off, nviews, 0.0, 0.0, maximum_tries, nullptr));
    return fit_batch_plan(resect_first_round, 1, view_off, nviews, maximum_tries, compute_units, out, items, items_cap);
  });
}
int spv_dlt_triangulate_batch(const double *x0, const double *x1, const long long *pair_off, int npairs,
                              const double *P0s, const double *P1s, const int32_t *use, const uint8_t *mask, double *X,
                              double *err, int32_t *rows, long long capacity, long long *out_off, long long *count) {
  return host_api([&] {
    return host_dlt_batch(x0, x1, pair_off, npairs, P0s, P1s, use, mask, X, err, rows, capacity, out_off, count);
  });
}
int spv_dlt_triangulate_batch_plan(const long long *pair_off, int npairs, const int32_t *use, int compute_units,
                                   long long out[3], int32_t *items, long long items_cap) {
  return api([&] {
    SPV_TRY(ransac_batch_check(pair_off, npairs, 0, nullptr));
    if (compute_units < 1 || !out || items_cap < 0) return set_error(SPV_ERR_INVALID, "bad arguments");
    std::vector<DltBatchItem> its;
    long long used = 0, bound = 0;
    dlt_batch_items(pair_off, npairs, use, false, &its, &used, &bound);
    out[0] = used;
    out[1] = (long long)its.size();
    out[2] = bound;
    export_items<4>(its, items, items_cap);
    return (int)SPV_OK;
  });
}
int spv_rectify_batch(const void *images, int dtype, const int32_t *sizes, int nimg, int nchan, double sampling_factor,
                      const int32_t *pairs, int npairs, const double *P0s, const double *P1s, const int32_t *use,
                      int crop, NdArray *rectified0, NdArray *rectified1, NdArray *rectified_idx0,
                      NdArray *rectified_idx1, int32_t *box, long long *out_off) {
  return host_api([&] {
    return host_rectify_batch(images, dtype, sizes, nimg, nchan, sampling_factor, pairs, npairs, P0s, P1s, use, crop,
                              rectified0, rectified1, rectified_idx0, rectified_idx1, box, out_off);
  });
}
int spv_rectify_batch_plan(const int32_t *sizes, int nimg, int nchan, double sampling_factor, const int32_t *pairs,
                           int npairs, const int32_t *use, const int32_t *box, long long out[3], long long *out_off,
                           int32_t *items, long long items_cap) {
  return api([&] {
    if (!out || !out_off || items_cap < 0) return set_error(SPV_ERR_INVALID, "bad arguments");
    RectifyBatchPlan pl;
    SPV_TRY(rectify_batch_plan(sizes, nimg, nchan, sampling_factor, pairs, npairs, use, box, &pl));
    out[0] = pl.used;
    out[1] = (long long)pl.items.size();
    out[2] = pl.out_off[npairs];
    memcpy(out_off, pl.out_off.data(), ((size_t)npairs + 1) * sizeof(long long));
    export_items<4>(pl.items, items, items_cap);
    return (int)SPV_OK;
  });
}
int spv_rectify_shape(int wid, int hgt, int nchan, double sf, int out[3]) {
  return api([&] {
    if (!out) return set_error(SPV_ERR_INVALID, "null output");
    return rectify_shape(wid, hgt, nchan, sf, out);
  });
}

int spv_rectify_fundamental(const double *P0, const double *P1, double *F) {
  return api([&] {
    if (!P0 || !P1 || !F) return set_error(SPV_ERR_INVALID, "null pointer");
    rectify_fundamental(P0, P1, F);
    return SPV_OK;
  });
}

int spv_dlt_reprojection_error(const double *P0, const double *P1, int npt, const double *x,
                               const double *xp, double *dst) {
  return host_api([&] { return host_dlt(P0, P1, npt, x, xp, dst, true); });
}

int spv_sift_filter(const float *im, int wid, int hgt, NdArray *out) {
  return host_api([&] {
    if (!out) return set_error(SPV_ERR_INVALID, "null NdArray");
    return host_sift(im, wid, hgt, out, nullptr, 0, nullptr);
  });
}

int spv_sift_set_first_capacity(int rows) {
  return api([&] {
    if (rows < 0) return set_error(SPV_ERR_INVALID, "negative row count");
    g_sift_first_rows.store(rows);
    return SPV_OK;
  });
}

int spv_sift_table(const float *im, int wid, int hgt, float *table, int capacity, int32_t *count) {
  return host_api([&] { return host_sift(im, wid, hgt, nullptr, table, capacity, count); });
}

int spv_sift_tables(const float *images, const int32_t *sizes, int nimg, float *table, const long long *cap_off,
                    int32_t *counts) {
  return host_api([&] { return host_sift_tables(images, sizes, nimg, table, cap_off, counts); });
}

// ---- device-pointer variants --------------------------------------------------------
size_t spv_l1k2_workspace_bytes(int xrows, int yrows, int dim) {
  if (!l1k2_shape_ok(xrows, yrows, dim)) return 0;
  const L1K2Plan p = l1k2_plan(xrows, yrows, dim);
  return p.dim_pad < 0 ? 0 : p.total_bytes;
}

int spv_l1k2_plan(int xrows, int yrows, int dim, int out[5]) {
  clear_error();
  if (!out) return set_error(SPV_ERR_INVALID, "null output");
  if (!l1k2_shape_ok(xrows, yrows, dim))
    return set_error(SPV_ERR_INVALID, "bad shape (xrows=%d, yrows=%d, dim=%d)", xrows, yrows, dim);
  const L1K2Plan p = l1k2_plan(xrows, yrows, dim);
  if (p.dim_pad < 0) return set_error(SPV_ERR_INVALID, "dim=%d is not supported by the L1 kernels", dim);
  out[0] = p.dim_pad;
  out[1] = p.q;
  out[2] = p.slices;
  out[3] = p.slice_rows;
  out[4] = p.path == kL1K2Wide ? 1 : 0;
  return SPV_OK;
}

int spv_l1k2_device(const uint8_t *d_x, const uint8_t *d_y, int xrows, int yrows, int dim,
                    uint64_t *d_idx, int32_t *d_dist, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] { return l1k2_run(d_x, d_y, xrows, yrows, dim, d_idx, d_dist, d_ws, ws_bytes,
                                   static_cast<hipStream_t>(stream)); });
}

int spv_l1k2_batch_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs, long long out[6],
                        int32_t *items, long long items_cap) {
  return api([&] {
    if (!out || (items && items_cap < 0)) return set_error(SPV_ERR_INVALID, "null output or negative items_cap");
    L1K2BatchPlan p;
    SPV_TRY(l1k2_batch_plan(seg_off, nseg, dim, pairs, npairs, &p));
    const long long n = (long long)p.items.size();
    out[0] = p.dim_pad;
    out[1] = p.q;
    out[2] = n;
    out[3] = p.out_rows;
    out[4] = p.max_slices;
    out[5] = (long long)p.total_bytes;
    export_items<5>(p.items, items, items_cap);
    return (int)SPV_OK;
  });
}

size_t spv_l1k2_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs) {
  return plan_bytes<L1K2BatchPlan>(&L1K2BatchPlan::total_bytes,
                                   [&](L1K2BatchPlan *p) { return l1k2_batch_plan(seg_off, nseg, dim, pairs, npairs, p); });
}

int spv_l1k2_batch_device(const uint8_t *d_desc, const long long *seg_off, int nseg, int dim, const int32_t *pairs,
                          int npairs, uint64_t *d_idx, int32_t *d_dist, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] {
    return l1k2_batch_run(d_desc, seg_off, nseg, dim, pairs, npairs, d_idx, d_dist, d_ws, ws_bytes,
                          static_cast<hipStream_t>(stream));
  });
}

int spv_l1k2_guided_batch_plan(const long long *seg_off, int nseg, int dim, const int32_t *pairs, int npairs,
                               long long out[4], int32_t *items, long long items_cap) {
  return api([&] {
    if (!out || (items && items_cap < 0)) return set_error(SPV_ERR_INVALID, "null output or negative items_cap");
    L1K2GuidedPlan p;
    SPV_TRY(l1k2_guided_plan(seg_off, nseg, dim, pairs, npairs, &p));
    const long long n = (long long)p.items.size();
    out[0] = n;
    out[1] = p.out_rows;
    out[2] = p.max_slices;
    out[3] = (long long)p.total_bytes;
    export_items<5>(p.items, items, items_cap);
    return (int)SPV_OK;
  });
}

size_t spv_l1k2_guided_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, const int32_t *pairs,
                                             int npairs) {
  return plan_bytes<L1K2GuidedPlan>(&L1K2GuidedPlan::total_bytes,
                                    [&](L1K2GuidedPlan *p) { return l1k2_guided_plan(seg_off, nseg, dim, pairs, npairs, p); });
}

int spv_l1k2_guided_batch_device(const uint8_t *d_desc, const float *d_geom, const long long *seg_off, int nseg, int dim,
                                 const int32_t *pairs, int npairs, const double *d_lines, double max_dist,
                                 uint64_t *d_idx, int32_t *d_dist, int32_t *d_ncand, void *d_ws, size_t ws_bytes,
                                 void *stream) {
  return api([&] {
    return l1k2_guided_run(d_desc, d_geom, seg_off, nseg, dim, pairs, npairs, d_lines, max_dist, d_idx, d_dist, d_ncand,
                           d_ws, ws_bytes, static_cast<hipStream_t>(stream));
  });
}

int spv_epipolar_lines_batch_device(const float *d_geom, const long long *seg_off, int nseg, const int32_t *pairs,
                                    int npairs, const double *G, const int32_t *use, double *d_lines, void *stream) {
  return api([&] {
    return epipolar_lines_run(d_geom, seg_off, nseg, pairs, npairs, G, use, d_lines, static_cast<hipStream_t>(stream));
  });
}

size_t spv_bruteforce_workspace_bytes(int xrows, int yrows, int dim, int k) {
  if (bruteforce_check(xrows, yrows, dim, k, 1.f) != SPV_OK) {
    clear_error();
    return 0;
  }
  return bruteforce_plan(xrows, yrows, k, 0).part_bytes;
}

int spv_bruteforce_device(const void *d_x, const void *d_y, int is_int, int xrows, int yrows, int dim, int k,
                          float p, int slices, uint64_t *d_idx, void *d_dist, void *d_ws, size_t ws_bytes,
                          void *stream) {
  return api([&] {
    return bruteforce_run(d_x, d_y, is_int, xrows, yrows, dim, k, p, slices, d_idx, d_dist, d_ws, ws_bytes,
                          static_cast<hipStream_t>(stream));
  });
}

size_t spv_ann_l2_workspace_bytes(int xrows, int yrows, int dim, int k, int ncand) {
  if (ann_check(xrows, yrows, dim, k, ncand) != SPV_OK) {
    clear_error();
    return 0;
  }
  return ann_plan(xrows, yrows, dim, k, ncand, 0).total_bytes;
}

int spv_ann_l2_plan(int xrows, int yrows, int dim, int k, int ncand, int slices, int out[8]) {
  clear_error();
  if (!out) return set_error(SPV_ERR_INVALID, "null output");
  SPV_TRY(ann_check(xrows, yrows, dim, k, ncand));
  if (slices < 0) return set_error(SPV_ERR_INVALID, "slices=%d", slices);
  const AnnPlan p = ann_plan(xrows, yrows, dim, k, ncand, slices);
  out[0] = p.kpad;
  out[1] = p.qtile;
  out[2] = p.rtile;
  out[3] = p.slices;
  out[4] = p.slice_rows;
  out[5] = p.ncand;
  out[6] = p.buflen;
  out[7] = p.mfma;
  return SPV_OK;
}

int spv_ann_l2_device(const float *d_x, const float *d_y, int xrows, int yrows, int dim, int k, int ncand, int slices,
                      uint64_t *d_idx, float *d_dist, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] {
    return ann_run(d_x, d_y, xrows, yrows, dim, k, ncand, slices, d_idx, d_dist, d_ws, ws_bytes,
                   static_cast<hipStream_t>(stream));
  });
}

int spv_rectify_device(const double *F, const void *d_im0, const void *d_im1, int dtype, int wid, int hgt, int nchan,
                       double sf, void *d_r0, void *d_r1, int32_t *d_ri0, int32_t *d_ri1, void *stream) {
  return api([&] {
    return rectify_run(F, d_im0, d_im1, dtype, wid, hgt, nchan, sf, d_r0, d_r1, d_ri0, d_ri1,
                       static_cast<hipStream_t>(stream));
  });
}

int spv_rectify_batch_bounds_device(const int32_t *sizes, int nimg, int nchan, double sampling_factor,
                                    const int32_t *pairs, int npairs, const double *P0s, const double *P1s,
                                    const int32_t *use, int32_t *d_box, void *stream) {
  return api([&] {
    return rectify_batch_bounds_run(sizes, nimg, nchan, sampling_factor, pairs, npairs, P0s, P1s, use, d_box,
                                    static_cast<hipStream_t>(stream));
  });
}
int spv_rectify_batch_device(const void *d_images, int dtype, const int32_t *sizes, int nimg, int nchan,
                             double sampling_factor, const int32_t *pairs, int npairs, const double *P0s,
                             const double *P1s, const int32_t *use, const int32_t *box, void *d_r0, void *d_r1,
                             int32_t *d_ri0, int32_t *d_ri1, void *stream) {
  return api([&] {
    return rectify_batch_run(d_images, dtype, sizes, nimg, nchan, sampling_factor, pairs, npairs, P0s, P1s, use, box,
                             d_r0, d_r1, d_ri0, d_ri1, static_cast<hipStream_t>(stream));
  });
}

int spv_stereo_batch_plan(const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange,
                          long long out[3], long long *out_off, int32_t *items, long long items_cap) {
  return api([&] {
    if (!out || !out_off || items_cap < 0) return set_error(SPV_ERR_INVALID, "bad arguments");
    StereoBatchPlan pl;
    SPV_TRY(stereo_batch_plan(box, npairs, use, radius, drange, &pl));
    out[0] = pl.used;
    out[1] = (long long)pl.items.size();
    out[2] = pl.out_off[npairs];
    memcpy(out_off, pl.out_off.data(), ((size_t)npairs + 1) * sizeof(long long));
    export_items<4>(pl.items, items, items_cap);
    return (int)SPV_OK;
  });
}
int spv_stereo_batch_device(const uint8_t *d_r0, const uint8_t *d_r1, const int32_t *d_ri0, const int32_t *d_ri1,
                            const int32_t *box, int npairs, const int32_t *use, int radius, const int32_t *drange,
                            int swap, int32_t *d_disp, void *d_cost, void *d_cost2, void *stream) {
  return api([&] {
    return stereo_batch_run(d_r0, d_r1, d_ri0, d_ri1, box, npairs, use, radius, drange, swap, d_disp,
                            static_cast<uint16_t *>(d_cost), static_cast<uint16_t *>(d_cost2),
                            static_cast<hipStream_t>(stream));
  });
}
int spv_stereo_keep_batch_device(const int32_t *box, int npairs, const int32_t *d_disp0, const void *d_cost0,
                                 const void *d_cost20, const int32_t *d_disp1, int lr_tol, int uniqueness,
                                 uint8_t *d_keep, void *stream) {
  return api([&] {
    return stereo_keep_batch_run(box, npairs, d_disp0, static_cast<const uint16_t *>(d_cost0),
                                 static_cast<const uint16_t *>(d_cost20), d_disp1, lr_tol, uniqueness, d_keep,
                                 static_cast<hipStream_t>(stream));
  });
}
int spv_stereo_matches_batch_device(const int32_t *box, int npairs, const int32_t *sizes, int nimg,
                                    const int32_t *pairs, const int32_t *d_disp0, const uint8_t *d_keep,
                                    const int32_t *d_ri0, const int32_t *d_ri1, long long capacity, double *d_x0,
                                    double *d_x1, int32_t *d_rows, long long *d_pair_off, void *stream) {
  return api([&] {
    return stereo_matches_batch_run(box, npairs, sizes, nimg, pairs, d_disp0, d_keep, d_ri0, d_ri1, capacity, d_x0,
                                    d_x1, d_rows, d_pair_off, static_cast<hipStream_t>(stream));
  });
}

size_t spv_sift_workspace_bytes(int wid, int hgt) {
  if (sift_check(wid, hgt) != SPV_OK) {
    clear_error();
    return 0;
  }
  return sift_workspace_bytes(wid, hgt);
}

int spv_sift_device(const float *d_im, int wid, int hgt, void *d_ws, size_t ws_bytes, float *d_table, int capacity,
                    int32_t *d_count, void *stream) {
  return api([&] {
    return sift_run(d_im, wid, hgt, d_ws, ws_bytes, d_table, capacity, d_count, static_cast<hipStream_t>(stream));
  });
}

int spv_sift_batch_plan(const int32_t *sizes, int nimg, size_t ws_bytes, long long out[4], int32_t *groups,
                        long long groups_cap) {
  return api([&] {
    if (!out || (groups && groups_cap < 0)) return set_error(SPV_ERR_INVALID, "null output or negative groups_cap");
    SiftBatchPlan p;
    SPV_TRY(sift_batch_plan(sizes, nimg, ws_bytes, &p));
    const long long n = (long long)p.groups.size();
    out[0] = n;
    out[1] = (long long)p.all_bytes;
    out[2] = (long long)p.min_bytes;
    out[3] = p.pixels;
    export_items<2>(p.groups, groups, groups_cap);
    return (int)SPV_OK;
  });
}

size_t spv_sift_batch_workspace_bytes(const int32_t *sizes, int nimg) {
  return plan_bytes<SiftBatchPlan>(&SiftBatchPlan::all_bytes, [&](SiftBatchPlan *p) { return sift_batch_plan(sizes, nimg, 0, p); });
}

int spv_sift_batch_device(const float *d_images, const int32_t *sizes, int nimg, void *d_ws, size_t ws_bytes,
                          float *d_table, const long long *cap_off, int32_t *d_counts, void *stream) {
  return api([&] {
    return sift_batch_run(d_images, sizes, nimg, d_ws, ws_bytes, d_table, cap_off, d_counts,
                          static_cast<hipStream_t>(stream));
  });
}

int spv_sift_batch_pack_device(const float *d_table, const long long *cap_off, const long long *seg_off, int nimg,
                               float *d_packed, float *d_geom, uint8_t *d_desc, void *stream) {
  return api([&] {
    return sift_batch_pack_run(d_table, cap_off, seg_off, nimg, d_packed, d_geom, d_desc,
                               static_cast<hipStream_t>(stream));
  });
}

size_t spv_cascade_workspace_bytes(int xrows, int yrows, int dim, int m, int n, int g) {
  if (!cascade_shape_ok(xrows, yrows, dim, m, n, g)) return 0;
  return cascade_workspace_bytes(xrows, yrows, dim, m, n, g);
}

int spv_cascade_plan(int xrows, int yrows, int dim, int m, int n, int g, int out[12]) {
  clear_error();
  if (!out) return set_error(SPV_ERR_INVALID, "null output");
  SPV_TRY(check_cascade_args(xrows, yrows, dim, m, n, g));
  if (dim > kCascadeMaxDim)
    return set_error(SPV_ERR_INVALID, "dim=%d > %d is not supported by the cascade refine kernel", dim, kCascadeMaxDim);
  const CascadePlan p = cascade_plan(xrows, yrows, dim, m, n, g);
  const int v[12] = {p.family, p.pa,    p.pb,   p.gmax_q, p.use_group, p.cpl,
                     p.ru,     p.wpe,   p.shift, p.full,  p.sorted,    p.qhist_fused};
  std::copy(v, v + 12, out);
  return SPV_OK;
}

int spv_cascade_batch_plan(const long long *seg_off, int nseg, int dim, int m, int n, int g, const int32_t *pairs,
                           int npairs, long long out[4], int32_t *items, long long items_cap) {
  return api([&] {
    if (!out || (items && items_cap < 0)) return set_error(SPV_ERR_INVALID, "null output or negative items_cap");
    CascadeBatchPlan p;
    SPV_TRY(cascade_batch_plan(seg_off, nseg, dim, m, n, g, pairs, npairs, &p));
    const long long cnt = (long long)p.items.size();
    out[0] = cnt;
    out[1] = p.out_rows;
    out[2] = p.hb;
    out[3] = (long long)p.total_bytes;
    export_items<3>(p.items, items, items_cap);
    return (int)SPV_OK;
  });
}

size_t spv_cascade_batch_workspace_bytes(const long long *seg_off, int nseg, int dim, int m, int n, int g,
                                         const int32_t *pairs, int npairs) {
  return plan_bytes<CascadeBatchPlan>(&CascadeBatchPlan::total_bytes, [&](CascadeBatchPlan *p) {
    return cascade_batch_plan(seg_off, nseg, dim, m, n, g, pairs, npairs, p);
  });
}

int spv_cascade_batch_device(const float *d_rows, const long long *seg_off, int nseg, int dim, int m, int n, int g,
                             const int32_t *pairs, int npairs, const float *d_dict, uint64_t *d_idx, float *d_dist,
                             int32_t *d_ncand, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] {
    return cascade_batch_run(d_rows, seg_off, nseg, dim, m, n, g, pairs, npairs, d_dict, d_idx, d_dist, d_ncand, d_ws,
                             ws_bytes, static_cast<hipStream_t>(stream));
  });
}

int spv_l1k2_gathered_device(int ndev, const int *devices, const uint8_t *const *d_x, const uint8_t *const *d_y,
                             int xrows, long long yrows_total, int dim, uint64_t *d_idx, int32_t *d_dist,
                             int transport) {
  return host_api([&] {
    if (!d_x || !d_y) return set_error(SPV_ERR_INVALID, "bad device list");
    SPV_TRY(check_gathered_devices(ndev, devices, transport));
    if (xrows < 0 || yrows_total < 0 || yrows_total > (long long)INT32_MAX * ndev)
      return set_error(SPV_ERR_INVALID, "bad row count");
    SPV_TRY(check_dim(dim));
    if (yrows_total == 0) return SPV_OK;
    if (!d_idx || !d_dist) return set_error(SPV_ERR_INVALID, "null pointer");
    const int G = (int)std::min<long long>(ndev, yrows_total);
    for (int r = 0; r < G; ++r) {
      if (!d_y[r] || (xrows > 0 && !d_x[r])) return set_error(SPV_ERR_INVALID, "null pointer (rank %d)", r);
      if (((uintptr_t)d_y[r] | (uintptr_t)d_x[r]) & 15)
        return set_error(SPV_ERR_INVALID, "device pointers must be 16-byte aligned (rank %d)", r);
    }
    if (((uintptr_t)d_idx | (uintptr_t)d_dist) & 15) return set_error(SPV_ERR_INVALID, "device pointers must be 16-byte aligned");
    return l1k2_gathered(std::vector<int>(devices, devices + ndev), {nullptr, d_x}, {nullptr, d_y}, xrows, yrows_total,
                         dim, d_idx, d_dist, transport);
  });
}

int spv_cascade_gathered_device(int ndev, const int *devices, const float *const *d_x, const float *const *d_y,
                                int xrows, long long yrows_total, int dim, int m, int n, int g,
                                const float *const *d_dict, uint64_t *d_idx, float *d_dist, int32_t *d_ncand,
                                int transport) {
  return host_api([&] {
    SPV_TRY(check_gathered_devices(ndev, devices, transport));
    if (!d_x || !d_y || !d_dict) return set_error(SPV_ERR_INVALID, "null pointer");
    if (yrows_total < 0 || yrows_total > (long long)INT32_MAX * ndev) return set_error(SPV_ERR_INVALID, "bad row count");
    SPV_TRY(check_cascade_args(xrows, 0, dim, m, n, g));
    if (yrows_total == 0) return SPV_OK;
    if (!d_idx || !d_dist) return set_error(SPV_ERR_INVALID, "null pointer");
    const int G = (int)std::min<long long>(ndev, yrows_total);
    for (int r = 0; r < G; ++r)
      if (!d_y[r] || !d_dict[r] || (xrows > 0 && !d_x[r])) return set_error(SPV_ERR_INVALID, "null pointer (rank %d)", r);
    return cascade_gathered(std::vector<int>(devices, devices + ndev), {nullptr, d_x}, {nullptr, d_y}, {nullptr, d_dict},
                            xrows, yrows_total, dim, m, n, g, d_idx, d_dist, d_ncand, transport);
  });
}

int spv_dlt_gathered_device(int ndev, const int *devices, const double *P0, const double *P1, long long npt_total,
                            const double *const *d_x, const double *const *d_xp, double *d_dst, int want_error,
                            int transport) {
  return host_api([&] {
    SPV_TRY(check_gathered_devices(ndev, devices, transport));
    if (npt_total < 0) return set_error(SPV_ERR_INVALID, "negative point count");
    if (npt_total == 0) return SPV_OK;
    if (!P0 || !P1 || !d_x || !d_xp || !d_dst) return set_error(SPV_ERR_INVALID, "null pointer");
    const int G = (int)std::min<long long>(ndev, npt_total);
    for (int r = 0; r < G; ++r)
      if (!d_x[r] || !d_xp[r]) return set_error(SPV_ERR_INVALID, "null pointer (rank %d)", r);
    return dlt_gathered(std::vector<int>(devices, devices + ndev), P0, P1, {nullptr, d_x}, {nullptr, d_xp}, npt_total,
                        d_dst, want_error != 0, transport);
  });
}

long long spv_shard_lo(long long total, int shards, int r) {
  if (shards < 1 || r < 0) return 0;
  if (r >= shards) return total;
  return shard_lo(total, shards, r);
}

int spv_cascade_device(const float *d_x, const float *d_y, int xrows, int yrows, int dim, int m,
                       int n, int g, const float *d_dict, uint64_t *d_idx, float *d_dist,
                       int32_t *d_ncand, void *d_ws, size_t ws_bytes, void *stream) {
  return api([&] {
    SPV_TRY(check_cascade_args(xrows, yrows, dim, m, n, g));
    return cascade_run(d_x, d_y, xrows, yrows, dim, m, n, g, d_dict, d_idx, d_dist, d_ncand, d_ws,
                       ws_bytes, static_cast<hipStream_t>(stream));
  });
}

int spv_dlt_triangulate_device(const double *P0, const double *P1, long long npt,
                               const double *d_x, const double *d_xp, double *d_dst,
                               void *stream) {
  return api([&] { return dlt_run(P0, P1, npt, d_x, d_xp, d_dst, false, static_cast<hipStream_t>(stream)); });
}
int spv_dlt_reprojection_error_device(const double *P0, const double *P1, long long npt,
                                      const double *d_x, const double *d_xp, double *d_dst,
                                      void *stream) {
  return api([&] { return dlt_run(P0, P1, npt, d_x, d_xp, d_dst, true, static_cast<hipStream_t>(stream)); });
}
int spv_dlt_triangulate_batch_device(const double *d_x0, const double *d_x1, const long long *pair_off, int npairs,
                                     const double *P0s, const double *P1s, const int32_t *use, const uint8_t *d_mask,
                                     double *d_X, double *d_err, int32_t *d_rows, long long capacity,
                                     long long *d_out_off, long long *d_count, void *stream) {
  return api([&] {
    return dlt_batch_run(d_x0, d_x1, pair_off, npairs, P0s, P1s, use, d_mask, d_X, d_err, d_rows, capacity, d_out_off,
                         d_count, static_cast<hipStream_t>(stream));
  });
}

}  // extern "C"
