// shard.h -- the devices the host-pointer entry points run on, and how a call is split over them.
#pragma once

#include "common.h"
#include "records.h"

#include <string>
#include <thread>
#include <vector>

namespace spv {

// Makes `dev` current on this thread; SPV_ERR_HIP when there is no such device.
int use_device(int dev);
// Devices the host-pointer entry points shard over.  One entry unless spv_set_devices() /
// SPECTAVI_DEVICES ("0,1,2,3" or "all") asked for more.
std::vector<int> device_list();
void set_device_list(const int *devices, int count);  // spv_set_device / spv_set_devices
void set_gather_mode(int mode);                       // spv_set_gather_mode
// How the shards of a host-pointer call of `total` rows reach the caller's arrays: SPV_GATHER_DIRECT
// (each shard copied straight into its slice), SPV_GATHER_RCCL or SPV_GATHER_PEERCOPY (gathered on
// the first listed GPU and copied from there).
int gather_transport(const std::vector<int> &devs, long long total = -1);

// Runs fn(r) for every rank r < G on a host thread of its own, each under guard(); returns the first
// failing rank's status as "device %d: <its message>".  A thread that cannot be started
// (std::system_error) must not unwind through joinable threads (std::terminate): that rank runs on
// the calling thread instead.
template <typename Fn>
int run_ranks(const std::vector<int> &devs, int G, Fn fn) {
  std::vector<int> status(G, SPV_OK);
  std::vector<std::string> message(G);
  {
    std::vector<std::thread> threads;
    threads.reserve(G);
    for (int r = 0; r < G; ++r) {
      auto rank = [&, r] {
        status[r] = guard([&] {
          const int st = fn(r);
          if (st != SPV_OK) message[r] = spv_last_error();
          return st;
        });
      };
      try {
        threads.emplace_back(rank);
      } catch (...) {
        rank();
      }
    }
    for (auto &t : threads) t.join();
  }
  for (int r = 0; r < G; ++r)
    if (status[r] != SPV_OK) return set_error(status[r], "device %d: %s", devs[r], message[r].c_str());
  return SPV_OK;
}

// Splits [0, total) into contiguous balanced shards (shard_lo), one per configured device, and runs
// fn(device, lo, hi) on a host thread per shard (every row of the hot path is independent: the
// reference parallelises the same loop with OpenMP, src/BruteForceNnL1K2.h:92).  Each shard writes
// straight into its slice of the caller's output, so no gather is needed inside one process.
template <typename Fn>
int run_sharded(long long total, Fn fn) {
  const std::vector<int> devs = device_list();
  const int G = (int)std::min<long long>((long long)devs.size(), std::max<long long>(total, 1));
  if (G <= 1) return fn(devs[0], 0LL, total);
  return run_ranks(devs, G, [&](int r) { return fn(devs[r], shard_lo(total, G, r), shard_lo(total, G, r + 1)); });
}

// Gathered calls: every rank computes its contiguous balanced shard on its own device, the results are
// gathered on devs[0] (transport: SPV_GATHER_RCCL, SPV_GATHER_PEERCOPY, or SPV_GATHER_AUTO to ask
// gather_transport) and written to the caller's arrays.  An input is either the caller's host array
// (host form: each rank stages its rows on its own stream, and the outputs are host arrays too) or one
// device-resident array per rank (the spv_*_gathered_device forms of include/spectavi_amd.h: the outputs
// are arrays on devs[0]).  The host form's pointers are checked by the caller.
template <typename T>
struct GatherInput {
  const T *host;        // host form
  const T *const *dev;  // device-resident form: dev[r] on devs[r]
};
int l1k2_gathered(const std::vector<int> &devs, GatherInput<uint8_t> x, GatherInput<uint8_t> y, int xrows,
                  long long yrows, int dim, uint64_t *idx, int32_t *dist, int transport);
int cascade_gathered(const std::vector<int> &devs, GatherInput<float> x, GatherInput<float> y, GatherInput<float> dict,
                     int xrows, long long yrows, int dim, int m, int n, int g, uint64_t *idx, float *dist,
                     int32_t *ncand, int transport);
int dlt_gathered(const std::vector<int> &devs, const double *P0, const double *P1, GatherInput<double> x,
                 GatherInput<double> xp, long long npt, double *dst, bool want_error, int transport);

}  // namespace spv
