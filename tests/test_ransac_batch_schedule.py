"""The round schedule of the many-sets RANSAC without a GPU: the host model (tests/ransac_batch_cases.schedule,
written from the stated rule) against the first round that spv_ransac_fit_batch_plan shows, and the properties
the two collections of tests/test_ransac_batch_rounds_gpu.py exist for -- asserted on the model here, so that the
GPU tests that hold the call to the model are known to reach the cuts."""
import numpy as np
import pytest

from tests import ransac_batch_cases as rc


def _sizes(off):
    return [int(n) for n in np.diff(np.asarray(off, np.int64))]


A_SIZES = rc.collection_a_shape()[0]

# (sizes, maximum_tries, compute units): A, B and the four of test_plan_cuts_candidates_when_row_blocks_are_few
PLANNED = [(A_SIZES, rc.A_TRIES, 256), (rc.B_SIZES, rc.B_TRIES, 256),
           ([500] * 64, 500, 256), ([50000] * 8, 500, 256),
           (_sizes(np.cumsum([0, 0, 9, 10, 255, 256, 257, 2500])), 60, 256), ([100] * 300, 1000, 64)]


@pytest.mark.parametrize("sizes,tries,cus", PLANNED, ids=["A", "B", "64x500", "8x50000", "edges", "300x100"])
def test_model_and_plan_agree_on_the_first_round(sizes, tries, cus):
    from spectavi_amd import device as spv
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    plan, items = spv.ransac_fit_batch_plan(off, tries, cus, want_items=True)
    first = rc.schedule(sizes, tries, [None] * len(sizes))[0][0]
    assert plan['sets'] == len(first) and plan['tries'] == sum(n for _, n in first)
    want, at = {}, 0
    for p, n in first:  # a slot's candidates follow those of the slot before: three a try
        want[p] = (3 * at, 3 * (at + n))
        at += n
    got = {}
    for s, _, _, c0, nc in items:
        lo, hi = got.get(int(s), (c0, c0 + nc))
        got[int(s)] = (min(lo, c0), max(hi, c0 + nc))
    assert got == want


def _a_model():
    sizes, clean = rc.collection_a_shape()
    return sizes, clean, rc.schedule(sizes, rc.A_TRIES, [0 if c else None for c in clean], detail=True)


def test_collection_a_fills_rounds_to_the_tries_cap():
    sizes, clean, (rounds, tries_run) = _a_model()
    held = [sum(s[1] for s in r) for r in rounds]
    assert rc.ROUND_TRIES in held and max(held) == rc.ROUND_TRIES
    # a slot below its set's step and below what the set had left, because the round was full
    assert any(n < step and n < left and cut == 'tries' for r in rounds for _, n, step, left, cut in r)
    assert not any(cut == 'work' for r in rounds for s in r for cut in s[4:])
    # ... one of them while the set's step could still grow: whether a cut slot grows the step shows in the rounds
    assert any(n < step < rc.A_TRIES and n < left and cut == 'tries' for r in rounds for _, n, step, left, cut in r)
    running = [p for p, n in enumerate(sizes) if n >= rc.MIN_SET_ROWS]
    assert len(running) == len(sizes) and set(running) - {s[0] for s in rounds[0]}  # a set without a slot in round one
    slots_of = {p: [k for k, r in enumerate(rounds) if any(s[0] == p for s in r)] for p in running}
    assert any(b - a > 1 for ks in slots_of.values() for a, b in zip(ks, ks[1:]))  # a round sat out between two slots
    # clean sets leave in different rounds, each between sets that go on
    last = {p: ks[-1] for p, ks in slots_of.items()}
    between = [p for p in running if clean[p] and 0 < p < len(sizes) - 1 and last[p - 1] > last[p] < last[p + 1]]
    assert len({last[p] for p in between}) >= 2
    assert all(tries_run[p] <= 256 for p in running if clean[p])
    assert all(tries_run[p] == rc.A_TRIES for p in running if not clean[p])
    alone = rc.schedule([17], rc.A_TRIES, [None])[0]
    assert [n for r in alone for _, n in r] == [256, 444] and len(rounds) > len(alone)


def test_collection_b_fills_a_round_to_the_work_cap():
    late = rc.collection_b_firsts()
    rounds, tries_run = rc.schedule(rc.B_SIZES, rc.B_TRIES, late, detail=True)
    capped = [r for r in rounds if any(s[4] == 'work' for s in r)]
    assert capped and all(sum(s[1] for s in r) < rc.ROUND_TRIES for r in capped)
    # sixteen whole steps are 1.966e9 solves; 282 tries of the next set fit, and not one of the set after it
    assert [s[:2] for s in capped[0]] == [(p, 1024) for p in range(16)] + [(16, 282)]
    # sets wait for that reason: running, served in round one, without a slot in the capped round
    assert {s[0] for s in rounds[0]} - {s[0] for s in capped[0]} == {17, 18, 19}
    assert len(rounds) > 3 and not any(s[4] == 'tries' for r in rounds for s in r)
    # what the call shows of the cut: set 16's first success lies inside its cut slot, set 17's is the first try it
    # would run if the capped round gave it any
    want = [rc.B_TRIES] * len(rc.B_SIZES)
    want[16], want[17] = 256 + 282, 256 + 1024
    assert tries_run == want and 256 <= late[16] < 256 + 282 and late[17] == 256
    assert rc.schedule(rc.B_SIZES, rc.B_TRIES, late, without='work clip')[1][16] == 256 + 1024


def test_the_collections_tell_a_rule_with_a_part_left_out():
    """The GPU tests hold tries_run and the number of rounds to the model; both collections are shaped so that a
    schedule without the work clip, or one that grows a step after a cut slot, differs in one of the two."""
    sizes, clean, _ = _a_model()
    shown = []
    for sz, tries, late in ((sizes, rc.A_TRIES, [0 if c else None for c in clean]),
                            (rc.B_SIZES, rc.B_TRIES, rc.collection_b_firsts())):
        full = rc.schedule(sz, tries, late)
        shown.append({w for w in ('work clip', 'whole step')
                      if (lambda m: (len(m[0]), m[1]))(rc.schedule(sz, tries, late, without=w)) != (len(full[0]), full[1])})
    assert shown == [{'whole step'}, {'work clip'}]
