"""Collections of correspondence sets for the many-sets RANSAC tests (tests/test_ransac_batch_args.py,
tests/test_ransac_batch_gpu.py, tests/test_ransac_batch_schedule.py, tests/test_ransac_batch_rounds_gpu.py): scenes
from tests/mvg_checks.two_view_scene with fixed seeds, as the single-fit tests draw them, the comparison of a batch
row with a single fit, and a host model of the round schedule (`schedule`) with the two collections that make a
round fill up."""
import numpy as np

from tests import mvg_checks as mc

THRESHOLD = 1e-3  # noise-free scenes: the reprojection error that separates planted inliers from outliers

# (required share, find_best) of test_ransac_fit_matches_oracle_given_the_same_subsets, with `clean` the clean
# share of the most contaminated set (0.65): success, best-on-failure and no model at all
SETTINGS = [(0.55, False), (0.55, True), (0.995, False), (0.995, True)]

# the sizes every collection of the edge test holds: empty, skipped, the minimum, the row-block edge, many row blocks
EDGE_SIZES = [0, 9, 10, 255, 256, 257, 2500]
EDGE_OUTLIERS = [0.0, 0.0, 0.1, 0.15, 0.2, 0.3, 0.35]


def scene(seed, npt, outliers):
    """x0, x1 float64 [npt,3] and the planted inlier rows."""
    if npt == 0:
        return np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int64)
    x0, x1, _, out_idx = mc.two_view_scene(np.random.default_rng(seed), npt=npt, outlier_fraction=outliers)
    return x0, x1, np.setdiff1d(np.arange(npt), out_idx)


def subsets(seed, npt, ntries):
    """int32 [ntries,7] as spv_ransac_sample draws them; a set too small to run gets rows no set holds (its
    subsets must not be read)."""
    from spectavi_amd import mvg
    if npt < 10:
        return np.full((ntries, 7), -7, np.int32)
    return mvg.ransac_sample(seed, npt, ntries)


def collection(sizes, outliers, ntries, seed0):
    """Lists x0s, x1s, samples, planted inliers: set p from seed seed0 + p."""
    x0s, x1s, smp, inl = [], [], [], []
    for p, (n, f) in enumerate(zip(sizes, outliers)):
        a, b, keep = scene(seed0 + p, n, f)
        x0s.append(a)
        x1s.append(b)
        inl.append(keep)
        smp.append(subsets(1000 + seed0 + p, n, ntries))
    return x0s, x1s, smp, inl


def offsets(x0s):
    return np.concatenate([[0], np.cumsum([len(x) for x in x0s])]).astype(np.int64)


def skipped_row():
    return {'success': False, 'essential': None, 'camera': None, 'inlier_percent': 0.0, 'n_inliers': 0,
            'best_try': -1, 'best_root': -1, 'tries_run': 0}


def assert_same_fit(row, single, ntries, what):
    """A batch row against the single fit of the same set with the same subsets: bit for bit on everything but
    tries_run, which stays within its bounds."""
    for k in ('success', 'best_try', 'best_root', 'inlier_percent'):
        assert row[k] == single[k], (what, k, row[k], single[k])
    assert np.array_equal(row['inlier_idx'], single['inlier_idx']), what
    assert row['inlier_idx'].dtype == np.int32
    for k in ('essential', 'camera'):
        if single[k] is None:
            assert row[k] is None, (what, k)
        else:
            assert row[k] is not None and row[k].tobytes() == single[k].tobytes(), (what, k)
    if row['success']:
        assert row['best_try'] < row['tries_run'] <= ntries, (what, row['tries_run'])
    else:
        assert row['tries_run'] == ntries, (what, row['tries_run'])


def assert_skipped(row, what):
    want = skipped_row()
    for k in ('success', 'essential', 'camera', 'inlier_percent', 'best_try', 'best_root', 'tries_run'):
        assert row[k] == want[k] or (row[k] is None and want[k] is None), (what, k, row[k])
    assert len(row['inlier_idx']) == 0, what


# ---- the round schedule, restated -----------------------------------------------------------------------------
#
# The rule as DESIGN.md A.1b and the header of ransac_batch.hip state it:
#   * a set of fewer than 10 rows never runs; every other set runs until its first success or until its tries
#     run out;
#   * a set asks for its step: first min(batch, max(8, min(256, 1e8 // (12 npt)))) tries, with
#     batch = min(max(1, min(5461, 2e9 // (12 npt))), maximum_tries), then fourfold up to batch -- but the step
#     grows only after a round that gave the set its whole step;
#   * a round takes the running sets in order while it has room: ROUND_TRIES tries, and ROUND_SOLVES (camera,
#     correspondence) solves at 12 npt a try once it holds anything (the first set of a round always runs).  A set
#     gets what fits of its step; when not one more try of it fits, the round is over;
#   * a set that found no room waits, unchanged.

ROUND_TRIES = 32768
ROUND_SOLVES = 2000000000
MIN_SET_ROWS = 10


def schedule(sizes, max_tries, leaves_after, detail=False, without=None):
    """The rounds of one call: sizes[p] rows per set, leaves_after[p] the try of set p's first success (the
    single fit's best_try where it succeeded) or None for a set that runs all its tries.  Returns (rounds,
    tries_run): rounds as lists of (set, tries) in slot order, tries_run per set (0 = skipped).  With detail a slot
    is (set, tries, step, left, cut): the step the set asked with, the tries it had left, and what cut the slot
    below both -- None, 'tries' or 'work'.

    `without` names a part of the rule to leave out, for the tests that show that a collection can tell: 'work
    clip' (a slot is not cut to the solves that are left; the round still ends once they are used up) or 'whole
    step' (the step grows after every slot)."""
    assert without in (None, 'work clip', 'whole step')
    running = []
    for p, npt in enumerate(sizes):
        if npt < MIN_SET_ROWS or max_tries <= 0:
            continue
        batch = min(max(1, min(5461, ROUND_SOLVES // (12 * npt))), max_tries)
        running.append(dict(set=p, cost=12 * int(npt), done=0, batch=batch,
                            step=min(batch, max(8, min(256, 100000000 // (12 * npt))))))
    rounds, tries_run = [], [0] * len(sizes)
    while running:
        tries_left, solves_left, slots = ROUND_TRIES, ROUND_SOLVES, []
        for s in running:
            by_tries = tries_left
            by_work = solves_left // s['cost'] if slots else by_tries  # an empty round takes its first set anyway
            if without == 'work clip':
                by_work = by_tries if solves_left > 0 or not slots else 0
            if min(by_tries, by_work) < 1:
                break  # the round is over: this set and all after it wait
            left = max_tries - s['done']
            want = min(s['step'], left)
            n = min(want, by_tries, by_work)
            cut = None if n == want else ('tries' if by_tries <= by_work else 'work')
            slots.append((s['set'], n, s['step'], left, cut))
            tries_left -= n
            solves_left -= n * s['cost']
        for p, n, step, _, _ in slots:
            s = next(r for r in running if r['set'] == p)
            if n == step or without == 'whole step':
                s['step'] = min(s['batch'], 4 * step)
            s['done'] += n
            tries_run[p] = s['done']
            after = leaves_after[p]
            if s['done'] >= max_tries or (after is not None and s['done'] > after):
                running.remove(s)
        rounds.append(slots if detail else [(p, n) for p, n, _, _, _ in slots])
    return rounds, tries_run


# Collection A, the tries cap: tiny sets, so that 32 768 tries are the only bound.  Clean sets of 10 and 12 rows
# (no outliers: a clean 7-subset on the first try, 100 % inliers) at every fourth place among all-outlier sets of 17
# and 40 rows, which cannot reach 90 %: 7 rows of a subset fit its model, 16 of 17 would have to.  218 sets: the
# third round is full when it reaches the last set, whose first step of 256 is cut to 128 -- a cut slot of a set
# whose step could still grow, so growing it regardless costs the call a round (200 sets cut only a step of 700,
# which is already the set's batch).
A_SETS = 218
A_TRIES = 700
A_SETTINGS = dict(required_percent_inliers=0.9, reprojection_error_allowed=THRESHOLD, find_best_even_in_failure=True,
                  singular_value_ratio_allowed=3e-2)


def collection_a_shape():
    """(sizes, clean flags) of collection A."""
    clean = [p % 4 == 3 for p in range(A_SETS)]
    sizes = [(10, 12)[(p // 4) % 2] if c else (17, 40)[p % 2] for p, c in enumerate(clean)]
    return sizes, clean


def collection_a():
    """x0s, x1s, samples, seeds (non-zero, one above 2^32) of collection A."""
    sizes, clean = collection_a_shape()
    x0s, x1s, smp, _ = collection(sizes, [0.0 if c else 1.0 for c in clean], A_TRIES, 7000)
    seeds = [9000 + 13 * p for p in range(A_SETS)]
    seeds[5] += 2 ** 40
    return x0s, x1s, smp, seeds


# Collection B, the work cap: 12 x 10 000 solves a try, so the second round's 1 024 tries a set are 1.2288e8 solves
# and sixteen sets fill 2e9 but for 282 tries of the seventeenth; not one try of the eighteenth fits.  Below about
# 5 100 rows a set the tries cap binds first (32 768 tries x 12 npt < 2e9).  The sets have 30 % outliers and never
# reach 99.5 %, but for two late sets (B_LATE: set -> first try with a clean subset): 0.4 % outliers, every subset
# before that try holds an outlier row, the subsets from there on hold none.  The seventeenth set's first success
# lies inside its cut slot (tries 256 .. 537): it leaves after 538 tries, and would after 1 280 were the slot not
# cut.  The eighteenth's is try 256, the first it has not run: it waits in round two and leaves after 1 280 tries,
# and would after 257 if the round gave it a try that does not fit.
B_SIZES = [10000] * 20
B_TRIES = 1300
B_LATE = {16: 400, 17: 256}
B_SETTINGS = dict(required_percent_inliers=0.995, reprojection_error_allowed=THRESHOLD, find_best_even_in_failure=True,
                  singular_value_ratio_allowed=3e-2)


def collection_b_firsts():
    """leaves_after of collection B as it is built."""
    return [B_LATE.get(p) for p in range(len(B_SIZES))]


def collection_b():
    outliers = [0.004 if p in B_LATE else 0.3 for p in range(len(B_SIZES))]
    x0s, x1s, smp, inl = collection(B_SIZES, outliers, B_TRIES, 8000)
    for p, first in B_LATE.items():
        good = inl[p]
        bad = np.setdiff1d(np.arange(B_SIZES[p]), good)
        assert len(bad) == 40
        s = smp[p].copy()
        for t in range(B_TRIES):
            if t < first:  # contaminated: one outlier row that the subset does not hold yet
                s[t, 0] = next(b for b in np.roll(bad, -t) if b not in s[t, 1:])
            else:          # clean: planted inliers for whatever outlier rows were drawn
                for k in np.flatnonzero(np.isin(s[t], bad)):
                    s[t, k] = next(g for g in np.roll(good, -97 * t) if g not in s[t])
        smp[p] = s
    return x0s, x1s, smp
