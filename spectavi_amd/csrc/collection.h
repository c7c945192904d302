// collection.h -- what the many-pairs ops share on the host: the rules of a collection (row sets stored back to
// back, seg_off, and the pairs of sets an op works on), the out rows of a pair list, and the per-pair table an op
// without a workspace keeps on the device between calls.  Host only.  See DESIGN.md 4.1b.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

namespace spv {

// off non-null, off[0] = 0, never decreasing, off[n] < 2^31 (n >= 0 is the caller's rule); SPV_ERR_INVALID with a
// message that names the argument `what` otherwise.
int check_offsets(const long long *off, int n, const char *what);

// The rules of (seg_off, pairs): nseg, npairs >= 0; check_offsets(seg_off, nseg); pairs non-null where npairs > 0;
// every pairs[i] in [0, nseg).  A null seg_off is refused: an entry that takes one for a collection without sets
// passes kNoSets in its place, in one line of its own.
int check_collection(const long long *seg_off, int nseg, const int32_t *pairs, int npairs);
inline constexpr long long kNoSets[1] = {0};
// ... and fewer than 2^31 out rows: the ops whose matches name an out row in an int32 (gather, tracks).
int check_collection_out32(const long long *seg_off, int nseg, const int32_t *pairs, int npairs);

// Of a checked collection.  out_off[npairs + 1]: pair p owns out rows [out_off[p], out_off[p + 1]), one per row of
// its query set.
std::vector<long long> pair_out_off(const long long *seg_off, const int32_t *pairs, int npairs);
// out_off [npairs + 1] | first row of the query set [npairs] | first row of the database set [npairs] | rows of the
// database set [npairs] | seg_off [nseg + 1].  The batch gather reads the first 3 npairs + 1 entries.
std::vector<long long> pair_table(const long long *seg_off, int nseg, const int32_t *pairs, int npairs);

// A table that lives with the calling thread between the calls of an op that has no workspace argument and does
// not wait for its kernels: a grow-only device buffer and the event of the launch that read it last, which the
// thread's next call waits for before it overwrites the table.  One thread_local instance per op.
struct DeviceTable {
  void *p = nullptr;
  size_t cap = 0;
  int dev = -1;
  hipEvent_t ev = nullptr;
  // waits for the last reader, grows, copies on `stream` (pageable source: the copy has left src on return)
  int upload(const void *src, size_t bytes, hipStream_t stream);
  int record(hipStream_t stream);  // after the last launch that reads the table
  void drop();
  ~DeviceTable() { drop(); }
};

}  // namespace spv
