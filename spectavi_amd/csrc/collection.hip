// collection.hip -- the host code of collection.h.

#include "collection.h"

#include "common.h"

namespace spv {

int check_offsets(const long long *off, int n, const char *what) {
  if (!off) return set_error(SPV_ERR_INVALID, "null %s", what);
  if (off[0] != 0) return set_error(SPV_ERR_INVALID, "%s[0] = %lld, must be 0", what, off[0]);
  for (int i = 0; i < n; ++i)
    if (off[i + 1] < off[i]) return set_error(SPV_ERR_INVALID, "%s decreases at %d", what, i);
  if (off[n] >= (1ll << 31)) return set_error(SPV_ERR_INVALID, "%s ends at %lld rows, must be below 2^31", what, off[n]);
  return SPV_OK;
}

int check_collection(const long long *seg_off, int nseg, const int32_t *pairs, int npairs) {
  if (nseg < 0 || npairs < 0) return set_error(SPV_ERR_INVALID, "negative count (nseg=%d, npairs=%d)", nseg, npairs);
  SPV_TRY(check_offsets(seg_off, nseg, "seg_off"));
  if (npairs > 0 && !pairs) return set_error(SPV_ERR_INVALID, "null pairs");
  for (int i = 0; i < 2 * npairs; ++i)
    if (pairs[i] < 0 || pairs[i] >= nseg)
      return set_error(SPV_ERR_INVALID, "pair %d names set %d of %d", i / 2, (int)pairs[i], nseg);
  return SPV_OK;
}

int check_collection_out32(const long long *seg_off, int nseg, const int32_t *pairs, int npairs) {
  SPV_TRY(check_collection(seg_off, nseg, pairs, npairs));
  const long long out_rows = pair_out_off(seg_off, pairs, npairs)[npairs];
  if (out_rows >= (1ll << 31)) return set_error(SPV_ERR_INVALID, "%lld out rows, must be below 2^31", out_rows);
  return SPV_OK;
}

std::vector<long long> pair_out_off(const long long *seg_off, const int32_t *pairs, int npairs) {
  std::vector<long long> off((size_t)npairs + 1, 0);
  for (int p = 0; p < npairs; ++p) off[(size_t)p + 1] = off[p] + (seg_off[pairs[2 * p] + 1] - seg_off[pairs[2 * p]]);
  return off;
}

std::vector<long long> pair_table(const long long *seg_off, int nseg, const int32_t *pairs, int npairs) {
  std::vector<long long> tab = pair_out_off(seg_off, pairs, npairs);
  tab.resize((size_t)4 * npairs + 1 + nseg + 1, 0);
  for (int p = 0; p < npairs; ++p) {
    const int q = pairs[2 * p], d = pairs[2 * p + 1];
    tab[(size_t)npairs + 1 + p] = seg_off[q];
    tab[(size_t)2 * npairs + 1 + p] = seg_off[d];
    tab[(size_t)3 * npairs + 1 + p] = seg_off[d + 1] - seg_off[d];
  }
  std::copy(seg_off, seg_off + nseg + 1, tab.begin() + (size_t)4 * npairs + 1);
  return tab;
}

int DeviceTable::upload(const void *src, size_t bytes, hipStream_t stream) {
  int now = 0;
  SPV_HIP_CHECK(hipGetDevice(&now));
  if (ev) SPV_HIP_CHECK(hipEventSynchronize(ev));
  if (dev != now || cap < bytes) {
    drop();
    SPV_HIP_CHECK(hipMalloc(&p, bytes));
    cap = bytes;
    dev = now;
  }
  if (!ev) SPV_HIP_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  SPV_HIP_CHECK(hipMemcpyAsync(p, src, bytes, hipMemcpyHostToDevice, stream));
  return SPV_OK;
}

int DeviceTable::record(hipStream_t stream) {
  SPV_HIP_CHECK(hipEventRecord(ev, stream));
  return SPV_OK;
}

void DeviceTable::drop() {
  if (ev) {
    (void)hipEventSynchronize(ev);
    (void)hipEventDestroy(ev);
    ev = nullptr;
  }
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
}

}  // namespace spv
