"""The first round of resect_fit_batch and its work items (spv_resect_fit_batch_plan, host only) against a Python
restatement of the stated rule: every set of 6 rows or more brings its first 256 tries while the round has room
(32768 tries, 4e9 verdicts); rows are cut in blocks of 256; with B row blocks in the round a set's tries are cut into
at most ceil(4 compute units / B) ranges of at least 48 tries."""
import numpy as np
import pytest

from spectavi_amd import device

ROUND_TRIES, ROUND_VERDICTS, FIRST_STEP, MIN_PIECE, BLOCK = 32768, 4000000000, 256, 48, 256


def restated(off, max_tries, cus):
    off = np.asarray(off, np.int64)
    slots, tries, verdicts = [], 0, 0
    if max_tries > 0:
        for p in range(len(off) - 1):
            n = int(off[p + 1] - off[p])
            if n < 6:
                continue
            if tries >= ROUND_TRIES or (tries > 0 and verdicts >= ROUND_VERDICTS):
                break
            by_work = (ROUND_VERDICTS - verdicts) // n if tries > 0 else 2 ** 31
            if by_work < 1:
                break
            k = min(FIRST_STEP, max_tries, ROUND_TRIES - tries, by_work)
            slots.append((p, n, tries, k))
            tries += k
            verdicts += n * k
    blocks = sum(-(-n // BLOCK) for _, n, _, _ in slots)
    items = []
    if blocks:
        pieces = min(-(-4 * cus // blocks), 1 << 16)
        for p, n, t0, k in slots:
            cut = max(1, min(pieces, k // MIN_PIECE))
            chunk = -(-k // cut)
            for r in range(0, n, BLOCK):
                for c in range(0, k, chunk):
                    items.append((p, int(off[p]) + r, min(BLOCK, n - r), t0 + c, min(chunk, k - c)))
    return dict(sets=len(slots), tries=tries, items=len(items), row_blocks=blocks), np.array(items, np.int32).reshape(-1, 5)


COLLECTIONS = {
    "the per-try cases": ([0, 5, 6, 255, 256, 257, 2500], 60, 256),
    "few row blocks, cut tries": ([300, 40, 6], 200, 256),
    "one small set": ([7], 500, 256),
    "one set, one compute unit": ([1000], 500, 1),
    "many sets fill the chip": ([500] * 600, 512, 256),
    "the round's try cap": ([10] * 200, 500, 304),
    "nothing runs": ([0, 5, 3], 500, 256),
    "no tries": ([100, 200], 0, 256),
    "64 views of 2000": ([2000] * 64, 512, 256),
}


@pytest.mark.parametrize("name", sorted(COLLECTIONS))
def test_plan_is_the_restated_rule(name):
    sizes, tries, cus = COLLECTIONS[name]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    want, want_items = restated(off, tries, cus)
    plan, items = device.resect_fit_batch_plan(off, tries, cus, want_items=True)
    assert plan == want, (name, plan, want)
    assert np.array_equal(items, want_items), name
    assert device.resect_fit_batch_plan(off, tries, cus) == want
    # every (row, try) of the round once, never across two sets
    for p, r0, rows, t0, n in items:
        assert off[p] <= r0 and r0 + rows <= off[p + 1] and 0 < rows <= BLOCK and n > 0
    cover = {}
    for p, r0, rows, t0, n in items:
        for r in range(r0, r0 + rows, BLOCK):
            cover.setdefault((int(p), int(r)), []).append((int(t0), int(n)))
    for key, ranges in cover.items():
        ranges.sort()
        assert all(a[0] + a[1] == b[0] for a, b in zip(ranges, ranges[1:])), key


def test_plan_properties():
    # the cut: 3 row blocks on 256 compute units, 200 tries -> 4 ranges of 50 for every set
    plan, items = device.resect_fit_batch_plan([0, 300, 340, 346], 200, 256, want_items=True)
    assert plan == dict(sets=3, tries=600, items=16, row_blocks=4)
    assert sorted(set(items[:, 4].tolist())) == [50]
    # a full chip is not cut
    plan = device.resect_fit_batch_plan(np.arange(0, 2100 * 201, 2100), 512, 256)
    assert plan["items"] == plan["row_blocks"] == 128 * 9 and plan["tries"] == ROUND_TRIES and plan["sets"] == 128
    # the items handed out are capped by items_cap
    from spectavi_amd._lib import clib
    import ctypes as ct
    out = (ct.c_longlong * 4)()
    off = np.array([0, 300, 340, 346], np.int64)
    few = np.full((3, 5), -1, np.int32)
    assert clib.spv_resect_fit_batch_plan(off.ctypes.data, 3, 200, 256, out, few.ctypes.data, 2) == 0
    assert out[2] == 16 and np.all(few[:2] >= 0) and np.all(few[2] == -1)
    for bad in ([], [1, 2], [0, 3, 2], [0, 2 ** 31]):
        with pytest.raises(ValueError):
            device.resect_fit_batch_plan(bad)
