// fit_rounds.h -- what the many-sets RANSAC fits share on the host (fit_rounds.hip): the argument check, the rule
// that fills a round, and the round driver.  ransac_batch.hip (two-view) and resect_batch.hip (resection) each
// describe themselves in a FitRoundsOp and enqueue their own kernels; the work items are ransac_batch_items'.
#pragma once
#include "common.h"

#include <functional>
#include <random>
#include <vector>

namespace spv {

// What a reduce kernel leaves for every slot of a round, and all the host reads back: the set's kept model so far.
struct FitHead {
  int found;    // a model has been kept
  int success;  // ... and it meets the required share
  int count;    // its inliers
  int cand;     // its candidate: per_try x try + its place in the try
};

// A set that is still running.
struct FitSetRun {
  int set, npt, done;  // done: tries evaluated so far
  int step, top;       // the tries it asks for next; fourfold after a round that gave it all of them, up to top
};

struct FitRoundsOp {
  int width;                                       // rows of a sample
  int per_try;                                     // candidates a try
  int min_rows;                                    // smaller sets are skipped
  int round_tries;                                 // the round rule: tries of all sets in a round,
  long long round_work, work_per_row;              //   its work, and the work of one try per row of its set
  void (*steps)(long long npt, int max_tries, int *first, int *top);  // a set's first step and its ceiling
  void (*draw)(std::mt19937 &gen, int npt, int *out);                 // one sample of a set of npt rows
  bool with_try_npt;                               // the round's tables also hold every try's set size
};

// SPV_ERR_INVALID (message set) for the counts, the offsets (`what` names them) and, where samples are given, a
// sample row outside its set; touches no device, no output.  With max_tries 0 and no samples: the rules of the
// offsets alone.
int fit_sets_check(const long long *off, int nsets, int max_tries, const int32_t *samples, int width, int min_rows,
                   const char *what, const char *tries_message);

// The device side of a round's tables, one upload: samples int[ntries, width] as rows of the concatenated arrays |
// try_npt int[ntries] (with_try_npt) | slots | items (16-byte aligned).
struct FitRoundTables {
  const int *samples, *try_npt;
  const RansacBatchSlot *slots;
  const RansacBatchItem *items;
  int ntries, nslots, nitems;
};

// The rounds of one call.  Every running set brings its next step of tries while the round has room
// (fit_fill_round); one upload brings the round's tables; `enqueue` puts the op's kernels on the stream, which must
// leave one FitHead per slot in d_heads; one read-back of the heads and one stream synchronisation; then a set that
// succeeded (unless stay_after_success) or ran out of tries leaves.
class FitRounds {
 public:
  FitRounds(const FitRoundsOp &op, const long long *off, int nsets, int max_tries);
  bool empty() const { return run_.empty(); }
  // The slots of the next round (host only); who (may be null): the slots' places among the running sets.
  void fill_round(std::vector<RansacBatchSlot> *slots, std::vector<int> *who) const;
  // The largest round: its tries, its work items (and those of a last pass over every row block) and its tables.
  void size_scratch(int cus);
  int round_cap() const { return round_cap_; }
  size_t items_cap() const { return items_cap_; }
  size_t tables_bytes() const { return tables_bytes_; }
  // Runs every round.  d_tables holds tables_bytes(), d_heads one FitHead per set; tries_run (may be null) per set.
  int run(const int32_t *samples, const unsigned long long *seeds, bool stay_after_success, unsigned char *d_tables,
          FitHead *d_heads, hipStream_t stream, const std::function<int(const FitRoundTables &)> &enqueue,
          int32_t *tries_run);
  const std::vector<FitHead> &last() const { return last_; }  // the last head of every set; cand -1: never ran

 private:
  const FitRoundsOp &op_;
  const long long *off_;
  int nsets_, max_tries_, cus_ = 0, round_cap_ = 0;
  size_t items_cap_ = 0, tables_bytes_ = 0;
  std::vector<FitSetRun> run_;
  std::vector<FitHead> last_;
};

// The host outputs the fits share.  Before the first round every set reports what a skipped set reports; after the
// last, what its head says: best_try = cand / per_try.
struct FitOutputs {
  int32_t *success;
  double *inlier_percent;
  int32_t *n_inliers, *best_try, *tries_run;  // best_try, tries_run may be null
};
void fit_outputs_clear(const FitOutputs &o, int nsets);
void fit_outputs_set(const FitOutputs &o, const FitRoundsOp &op, const long long *off, const std::vector<FitHead> &last);

// (error paths of a fit: nothing may still be queued on a caller's stream when the scratch goes back to the pool)
struct StreamDrain {
  hipStream_t st;
  ~StreamDrain() { (void)hipStreamSynchronize(st); }
};

}  // namespace spv
