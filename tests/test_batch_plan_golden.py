"""CPU-only: the three many-pairs plans answer, item for item, what tests/golden/batch_plans.json records, and the six
entries that take a collection refuse the same bad collections with the same status.

The plans of spv_l1k2_batch_plan, spv_l1k2_guided_batch_plan and spv_cascade_batch_plan are pinned by their whole
out[], their item count, the SHA-256 of the int32 item array (the array itself where it has at most 64 items) and the
answer of the matching *_workspace_bytes query.  The status matrix records the return status alone, never the message,
of a list of bad collections through the three plans and, with null device pointers so that nothing reaches a device,
through spv_epipolar_lines_batch_device, spv_gather_match_coords_batch_device and spv_tracks_batch_device.
`python -m tests.test_batch_plan_golden` rewrites the fixture from the library as built; that is done before a change
to the planners or the collection rules, never after it."""
import ctypes as ct
import hashlib
import json
import os

import numpy as np
import pytest

from tests import cascade_batch_cases as cc
from tests import l1k2_batch_cases as lc

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_plans.json")
PLAN_KNOBS = ("SPECTAVI_L1K2_", "SPECTAVI_CASCADE_")   # the plans read these
DIMS = (16, 64, 128, 176, 256)
FULL_ITEMS = 64   # item arrays up to this long are recorded in full


def random_collection(seed):
    """2..12 sets of 0..3000 rows, now and then one of 20000, and 1..40 pairs, repeats and self pairs included."""
    rng = np.random.default_rng([seed, 0xC011])
    nseg = int(rng.integers(2, 13))
    rows = rng.choice([0, 1, 63, 64, 65, 255, 256, 257, 700, 3000], nseg).tolist()
    if seed % 2:
        rows[int(rng.integers(0, nseg))] = 20000
    pairs = rng.integers(0, nseg, (int(rng.integers(1, 41)), 2)).tolist()
    return rows, [tuple(p) for p in pairs]


def collections():
    """(name, set rows, pairs, dims of the l1k2_batch plan)."""
    out = [("nine-all81", lc.NINE, lc.ALL81, DIMS), ("nine-few", lc.NINE, lc.FEW, DIMS)]
    for prefix in ("mid-", "long-", "tiles-", "maxslice-"):
        named = [c for c in lc.Q_CASES if c[0].startswith(prefix) and c[3] in DIMS]
        out.append((prefix.rstrip("-"), named[0][1], named[0][2], tuple(c[3] for c in named)))
    out += [("no-sets", [], [], DIMS), ("no-pairs", lc.NINE, [], DIMS), ("all-empty", [0, 0, 0], [(0, 1), (2, 2)], DIMS),
            ("empty-database", [100, 0], [(0, 1)], DIMS), ("empty-query", [0, 100], [(0, 1)], DIMS)]
    out += [("random-%d" % s,) + random_collection(s) + (DIMS,) for s in range(6)]
    return out


def plan_cases():
    """(entry, size query, case name, set rows, pairs, the int arguments between nseg and pairs, out[] length, columns)."""
    cases = []
    for name, rows, pairs, dims in collections():
        for d in dims:
            cases.append(("spv_l1k2_batch_plan", "spv_l1k2_batch_workspace_bytes", "%s/%d" % (name, d), rows, pairs, (d,), 6, 5))
        if 128 in dims:
            cases.append(("spv_l1k2_guided_batch_plan", "spv_l1k2_guided_batch_workspace_bytes", "%s/128" % name, rows,
                          pairs, (128,), 4, 5))
            cases.append(("spv_cascade_batch_plan", "spv_cascade_batch_workspace_bytes", "%s/%s" % (name, list(cc.NINE_SHAPE)),
                          rows, pairs, cc.NINE_SHAPE, 4, 3))
    for shape in cc.EDGES:
        cases.append(("spv_cascade_batch_plan", "spv_cascade_batch_workspace_bytes", "few/%s" % list(shape), cc.FEW_ROWS,
                      cc.FEW, shape, 4, 3))
    return cases


def plan_answers():
    from spectavi_amd._lib import clib
    got = {}
    for entry, size_query, name, rows, pairs, ints, nout, cols in plan_cases():
        seg = lc.seg_of(rows)
        prs = np.ascontiguousarray(np.asarray(pairs, np.int32).reshape(-1, 2))
        args = (seg.ctypes.data, len(rows)) + tuple(int(v) for v in ints) + (prs.ctypes.data if len(prs) else None, len(prs))
        out = (ct.c_longlong * nout)()
        fn = getattr(clib, entry)
        assert fn(*args, out, None, 0) == 0, (entry, name)
        first = list(out)
        count = first[2] if nout == 6 else first[0]
        items = np.full((count, cols), -1, np.int32)
        assert fn(*args, out, items.ctypes.data, count) == 0, (entry, name)
        assert list(out) == first
        rec = dict(out=first, items=count, sha256=hashlib.sha256(items.tobytes()).hexdigest(),
                   workspace_bytes=int(getattr(clib, size_query)(*args)))
        if count <= FULL_ITEMS:
            rec["rows"] = items.tolist()
        got.setdefault(entry, {})[name] = rec
    return got


# (name, seg_off or None, nseg, pairs or None, npairs)
GOOD = [0, 5, 9]
BAD = [
    ("null-seg-off/nseg-0/npairs-0", None, 0, None, 0),
    ("null-seg-off/nseg-0/npairs-1", None, 0, [(0, 0)], 1),
    ("null-seg-off/nseg-2", None, 2, [(0, 1)], 1),
    ("null-pairs", GOOD, 2, None, 1),
    ("seg-off-0-not-0", [1, 5, 9], 2, [(0, 1)], 1),
    ("decrease", [0, 5, 3], 2, [(0, 1)], 1),
    ("total-2^31", [0, 2 ** 31], 1, [(0, 0)], 1),
    ("pair-names-minus-1", GOOD, 2, [(0, -1)], 1),
    ("pair-names-nseg", GOOD, 2, [(2, 0)], 1),
    ("negative-nseg", GOOD, -1, [(0, 1)], 1),
    ("negative-npairs", GOOD, 2, [(0, 1)], -1),
    # controls: collections every entry accepts (the device entries then refuse their null device pointers)
    ("control/nseg-0", [0], 0, None, 0),
    ("control/valid", GOOD, 2, [(0, 1), (1, 1)], 2),
]
ENTRIES = ("spv_l1k2_batch_plan", "spv_l1k2_guided_batch_plan", "spv_cascade_batch_plan", "spv_epipolar_lines_batch_device",
           "spv_gather_match_coords_batch_device", "spv_tracks_batch_device")


def status_answers():
    from spectavi_amd._lib import clib
    got = {}
    for name, seg, nseg, pairs, npairs in BAD:
        seg_a = None if seg is None else np.asarray(seg, np.int64)
        prs_a = None if pairs is None else np.ascontiguousarray(np.asarray(pairs, np.int32))
        s = None if seg_a is None else seg_a.ctypes.data
        p = None if prs_a is None else prs_a.ctypes.data
        out = (ct.c_longlong * 6)()
        got[name] = [
            clib.spv_l1k2_batch_plan(s, nseg, 128, p, npairs, out, None, 0),
            clib.spv_l1k2_guided_batch_plan(s, nseg, 128, p, npairs, out, None, 0),
            clib.spv_cascade_batch_plan(s, nseg, *cc.NINE_SHAPE, p, npairs, out, None, 0),
            clib.spv_epipolar_lines_batch_device(None, s, nseg, p, npairs, None, None, None, None),
            clib.spv_gather_match_coords_batch_device(None, s, nseg, p, npairs, None, None, 0, None, None, None, None),
            clib.spv_tracks_batch_device(s, nseg, p, npairs, None, None, 0, None, 2, 0, None, None, None, None, None, None,
                                         None, 0, None),
        ]
    return got


def skip_under_knobs():
    knobs = sorted(k for k in os.environ if k.startswith(PLAN_KNOBS))
    if knobs:
        pytest.skip("the plans read %s" % ", ".join(knobs))


def recorded():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def plans_now():
    skip_under_knobs()
    return plan_answers()


@pytest.mark.parametrize("entry", ENTRIES[:3])
def test_plan_answers_the_recorded_items(entry, plans_now):
    want, got = recorded()["plans"][entry], plans_now[entry]
    assert sorted(want) == sorted(got), "the fixture records other cases than this module lists"
    wrong = [(n, want[n], got[n]) for n in sorted(want) if want[n] != got[n]]
    assert not wrong, "%d of %d plans differ (case, recorded, now): %s" % (len(wrong), len(want), wrong[:2])
    assert any(r["items"] > FULL_ITEMS for r in want.values()) and any("rows" in r for r in want.values())


def test_bad_collections_get_the_recorded_status():
    skip_under_knobs()
    rec = recorded()
    assert rec["status_entries"] == list(ENTRIES)
    want, got = rec["status"], status_answers()
    assert sorted(want) == sorted(got), "the fixture records other collections than this module lists"
    wrong = [(n, want[n], got[n]) for n in sorted(want) if want[n] != got[n]]
    assert not wrong, "statuses differ (collection, recorded, now), entries %s: %s" % (list(ENTRIES), wrong)
    assert {0} < {s for row in want.values() for s in row}, "the matrix holds both SPV_OK and refusals"


if __name__ == "__main__":
    assert not [k for k in os.environ if k.startswith(PLAN_KNOBS)]
    with open(FIXTURE, "w") as f:
        json.dump(dict(plans=plan_answers(), status_entries=list(ENTRIES), status=status_answers()), f, sort_keys=True,
                  separators=(",", ":"))
        f.write("\n")
    print("wrote %s: %d bytes" % (FIXTURE, os.path.getsize(FIXTURE)))
