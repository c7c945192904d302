// fit_rounds.hip -- the host side that the many-sets RANSAC fits share (fit_rounds.h): ransac_batch.hip fits an
// essential matrix to every set of a collection, resect_batch.hip a camera, and both advance their sets together
// in rounds.  A round is the same for both:
//
//   every set that is still running contributes its next block of tries (its step: small first, fourfold after a
//   round that gave it the whole step, up to the op's ceiling), in order, as long as the round has room: the op's
//   tries cap and work cap (fill_round);
//   the work items of the round are ransac_batch_items' (ransac_batch.hip);
//   one upload brings the round's tables: the subsets as row numbers of the CONCATENATED arrays, copied from the
//   caller's samples or drawn from the set's own generator, (each try's set size,) the slots and the items;
//   the op's kernels run over all tries of the round and leave one four-int head per slot;
//   one read-back of the heads and one stream synchronisation; sets that succeeded or ran out of tries leave.
//
// Nothing here depends on what a try computes.  A set's results do not depend on how its tries are cut into rounds
// (the ops say why); only tries_run does.
#include "fit_rounds.h"

#include "collection.h"

#include <string.h>

namespace spv {

int fit_sets_check(const long long *off, int nsets, int max_tries, const int32_t *samples, int width, int min_rows,
                   const char *what, const char *tries_message) {
  if (nsets < 0) return set_error(SPV_ERR_INVALID, "negative set count");
  if (nsets > (1 << 20)) return set_error(SPV_ERR_INVALID, "more than 2^20 sets per call");
  if (max_tries < 0) return set_error(SPV_ERR_INVALID, "negative maximum_tries");
  if (max_tries > 700000000) return set_error(SPV_ERR_INVALID, "%s", tries_message);
  SPV_TRY(check_offsets(off, nsets, what));
  if (!samples) return SPV_OK;
  for (int p = 0; p < nsets; ++p) {
    const long long npt = off[p + 1] - off[p];
    if (npt < min_rows) continue;  // a skipped set's subsets are not read
    const int32_t *s = samples + (size_t)p * max_tries * width;
    for (size_t i = 0; i < (size_t)max_tries * width; ++i)
      if (s[i] < 0 || s[i] >= npt)
        return set_error(SPV_ERR_INVALID, "set %d: sample index %d outside [0, %lld)", p, s[i], npt);
  }
  return SPV_OK;
}

FitRounds::FitRounds(const FitRoundsOp &op, const long long *off, int nsets, int max_tries)
    : op_(op), off_(off), nsets_(nsets), max_tries_(max_tries), last_((size_t)std::max(nsets, 0), FitHead{0, 0, 0, -1}) {
  if (max_tries <= 0) return;
  for (int p = 0; p < nsets; ++p) {
    const long long npt = off[p + 1] - off[p];
    if (npt < op.min_rows) continue;
    int first, top;
    op.steps(npt, max_tries, &first, &top);
    run_.push_back(FitSetRun{p, (int)npt, 0, first, top});
  }
}

// A running set brings its next min(step, what is left of max_tries) tries while the round holds fewer than
// round_tries tries and less than round_work units of work, a try of a set costing work_per_row x npt; the first set
// of a round always runs, and a set of which not one more try fits waits with the sets behind it.  A slot counts
// candidates: per_try of them a try.
void FitRounds::fill_round(std::vector<RansacBatchSlot> *slots, std::vector<int> *who) const {
  slots->clear();
  if (who) who->clear();
  int tries = 0;
  long long work = 0;
  for (size_t i = 0; i < run_.size(); ++i) {
    const FitSetRun &r = run_[i];
    if (tries >= op_.round_tries || (tries > 0 && work >= op_.round_work)) break;
    const long long per = op_.work_per_row * r.npt;
    const long long by_work = tries == 0 ? 2147483647 : (op_.round_work - work) / per;  // the first set always runs
    if (by_work < 1) break;  // not one more try of this set fits: it waits, and so do the sets behind it
    const int n = (int)std::min<long long>({(long long)r.step, (long long)(max_tries_ - r.done), (long long)(op_.round_tries - tries), by_work});
    if (n <= 0) continue;
    slots->push_back(RansacBatchSlot{r.set, r.npt, op_.per_try * tries, op_.per_try * n, op_.per_try * r.done});
    if (who) who->push_back((int)i);
    tries += n;
    work += per * n;
  }
}

void FitRounds::size_scratch(int cus) {
  cus_ = cus;
  // no set brings more than its ceiling, the round no more than round_tries
  long long cap_tries = 0;
  for (const FitSetRun &r : run_) cap_tries += std::min(r.top, max_tries_);
  round_cap_ = (int)std::min<long long>(cap_tries, op_.round_tries);
  // (ransac_batch_items cuts a set's candidates at most ceil(4 cus / blocks) ways)
  size_t all_blocks = 0;
  for (int p = 0; p < nsets_; ++p) all_blocks += batch_row_blocks(off_[p + 1] - off_[p]);
  items_cap_ = all_blocks + 4 * (size_t)cus + (size_t)nsets_;
  tables_bytes_ = (size_t)round_cap_ * (op_.width + (op_.with_try_npt ? 1 : 0)) * sizeof(int) +
                  (size_t)nsets_ * sizeof(RansacBatchSlot) + items_cap_ * sizeof(RansacBatchItem) + 64;
}

int FitRounds::run(const int32_t *samples, const unsigned long long *seeds, bool stay_after_success,
                   unsigned char *d_tables, FitHead *d_heads, hipStream_t stream,
                   const std::function<int(const FitRoundTables &)> &enqueue, int32_t *tries_run) {
  const int width = op_.width, per = op_.per_try;
  std::vector<std::mt19937> gens;  // one per running set; gen_of survives the compaction of run_
  if (!samples) {
    gens.reserve(run_.size());
    for (const FitSetRun &r : run_) gens.emplace_back(ransac_seed(seeds[r.set]));
  }
  std::vector<int> gen_of(run_.size());
  for (size_t i = 0; i < run_.size(); ++i) gen_of[i] = (int)i;

  std::vector<RansacBatchSlot> slots;
  std::vector<RansacBatchItem> items;
  std::vector<int> who;
  std::vector<unsigned char> host;
  std::vector<FitHead> heads((size_t)nsets_);
  while (!run_.empty()) {
    fill_round(&slots, &who);
    ransac_batch_items(slots, off_, cus_, &items);
    int ntries = 0;
    for (const RansacBatchSlot &s : slots) ntries += s.ncand / per;
    const size_t off_npt = (size_t)ntries * width * sizeof(int);
    const size_t off_slots = off_npt + (op_.with_try_npt ? (size_t)ntries * sizeof(int) : 0);
    const size_t off_items = round_up(off_slots + slots.size() * sizeof(RansacBatchSlot), 16);
    const size_t bytes = off_items + items.size() * sizeof(RansacBatchItem);
    if (ntries > round_cap_ || bytes > tables_bytes_)
      return set_error(SPV_ERR_INTERNAL, "round of %d tries, %zu items outgrew its scratch", ntries, items.size());
    host.resize(bytes);
    int *h_samples = reinterpret_cast<int *>(host.data());
    int *h_npt = reinterpret_cast<int *>(host.data() + off_npt);
    for (size_t k = 0; k < slots.size(); ++k) {
      const RansacBatchSlot &s = slots[k];
      const int n = s.ncand / per, t0 = s.cand0 / per;
      int *dst = h_samples + (size_t)t0 * width;
      if (samples) {
        memcpy(dst, samples + ((size_t)s.set * max_tries_ + run_[who[k]].done) * width, (size_t)n * width * sizeof(int));
      } else {
        std::mt19937 &gen = gens[gen_of[who[k]]];
        for (int t = 0; t < n; ++t) op_.draw(gen, s.npt, dst + (size_t)width * t);
      }
      const int row0 = (int)off_[s.set];
      for (size_t i = 0; i < (size_t)n * width; ++i) dst[i] += row0;  // rows of the concatenated arrays
      if (op_.with_try_npt)
        for (int t = 0; t < n; ++t) h_npt[t0 + t] = s.npt;
    }
    if (!slots.empty()) memcpy(host.data() + off_slots, slots.data(), slots.size() * sizeof(RansacBatchSlot));
    if (!items.empty()) memcpy(host.data() + off_items, items.data(), items.size() * sizeof(RansacBatchItem));
    // (pageable source: the copy has left `host` when the call returns)
    SPV_HIP_CHECK(hipMemcpyAsync(d_tables, host.data(), bytes, hipMemcpyHostToDevice, stream));
    SPV_TRY(enqueue(FitRoundTables{reinterpret_cast<const int *>(d_tables),
                                   op_.with_try_npt ? reinterpret_cast<const int *>(d_tables + off_npt) : nullptr,
                                   reinterpret_cast<const RansacBatchSlot *>(d_tables + off_slots),
                                   reinterpret_cast<const RansacBatchItem *>(d_tables + off_items), ntries,
                                   (int)slots.size(), (int)items.size()}));
    SPV_HIP_CHECK(hipMemcpyAsync(heads.data(), d_heads, slots.size() * sizeof(FitHead), hipMemcpyDeviceToHost, stream));
    SPV_HIP_CHECK(hipStreamSynchronize(stream));
    // sets that succeeded or ran out of tries leave
    std::vector<char> leaves(run_.size(), 0);
    for (size_t k = 0; k < slots.size(); ++k) {
      FitSetRun &r = run_[who[k]];
      const int n = slots[k].ncand / per;
      if (n == r.step) r.step = std::min(r.top, r.step * 4);
      r.done += n;
      last_[r.set] = heads[k];
      if (tries_run) tries_run[r.set] = r.done;
      if ((heads[k].success && !stay_after_success) || r.done >= max_tries_) leaves[who[k]] = 1;
    }
    size_t keep = 0;
    for (size_t i = 0; i < run_.size(); ++i)
      if (!leaves[i]) {
        run_[keep] = run_[i];
        gen_of[keep] = gen_of[i];
        ++keep;
      }
    run_.resize(keep);
  }
  return SPV_OK;
}

void fit_outputs_clear(const FitOutputs &o, int nsets) {
  for (int p = 0; p < nsets; ++p) {
    o.success[p] = 0;
    o.inlier_percent[p] = 0.0;
    o.n_inliers[p] = 0;
    if (o.best_try) o.best_try[p] = -1;
    if (o.tries_run) o.tries_run[p] = 0;
  }
}

void fit_outputs_set(const FitOutputs &o, const FitRoundsOp &op, const long long *off, const std::vector<FitHead> &last) {
  for (size_t p = 0; p < last.size(); ++p) {
    const FitHead &h = last[p];
    o.success[p] = h.success;
    o.n_inliers[p] = h.found ? h.count : 0;
    const long long npt = off[p + 1] - off[p];
    o.inlier_percent[p] = npt >= op.min_rows ? (double)o.n_inliers[p] / (double)npt : 0.0;
    if (o.best_try) o.best_try[p] = h.found ? h.cand / op.per_try : -1;
  }
}

}  // namespace spv
