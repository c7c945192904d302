"""The helpers of tests/test_l1k2_batch_gpu.py, and a child process for what cannot run inside pytest's: the planner
gives a collection that fills the chip the largest q its width allows, so items of more than one LDS tile meet the
Q = 1 instantiations (and Q = 2 at widths <= 64) only under SPECTAVI_L1K2_Q, which the library reads once per process.
The parent puts the variable in this process's environment; the child asserts from the plan that it took effect and
that the items are the 4096-row ones, then checks every tiles-* case of tests/l1k2_batch_cases.py against the oracle.
Exits 1 on the first mismatch, printing the case.

    SPECTAVI_L1K2_Q=<q> python tests/l1k2_batch_child.py <q> [--plan-only]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from tests import l1k2_batch_cases as bc  # noqa: E402


def sets_u8(seed, rows, dim, hi=256):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, hi, (r, dim), dtype=np.uint8) for r in rows]


def case_tables(case):
    """The sets of a case of bc.Q_CASES: few distinct byte values at the narrow widths, so that distances tie and the
    (dist, idx) order is exercised across tiles, slices and items."""
    name, rows, _, dim = case[:4]
    return sets_u8(len(name) + dim, rows, dim, hi=4 if dim <= 32 else 256)


def run_device(tables, pairs, workspace=None):
    """device.l1k2_batch on the concatenated tables -> (idx uint64, dist int32, out_off) on the host."""
    import torch
    from spectavi_amd import device
    dim = tables[0].shape[1]
    desc = torch.from_numpy(np.concatenate(tables).reshape(-1, dim)).cuda()
    idx, dist, off = device.l1k2_batch(desc, bc.seg_of([len(t) for t in tables]), pairs, workspace=workspace)
    torch.cuda.synchronize()
    return idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), off


def check_pairs(oracle, tables, pairs, idx, dist, off, which=None):
    assert idx.shape == dist.shape == (off[-1], 2) and len(off) == len(pairs) + 1
    memo = {}
    for p in (range(len(pairs)) if which is None else which):
        a, b = pairs[p]
        if (a, b) not in memo:
            memo[(a, b)] = oracle.nn_bruteforcel1k2(tables[b], tables[a], nthreads=8)
        oi, od = memo[(a, b)]
        assert off[p + 1] - off[p] == len(tables[a])
        assert np.array_equal(idx[off[p]:off[p + 1]], oi), ("idx of pair %d = %s" % (p, (a, b)))
        assert np.array_equal(dist[off[p]:off[p + 1]], od), ("dist of pair %d = %s" % (p, (a, b)))


def longest_item(rows, pairs, dim):
    """(q, database rows of the longest item) of the plan in force."""
    from spectavi_amd import device
    plan, items = device.l1k2_batch_plan(bc.seg_of(rows), pairs, dim, want_items=True)
    return plan["q"], int(items[:, 4].max())


def main(q, plan_only):
    assert os.environ.get("SPECTAVI_L1K2_Q") == str(q), "the parent must set SPECTAVI_L1K2_Q"
    if not plan_only:
        from oracle import oracle
    for case in bc.TILE_CASES:
        name, rows, pairs, dim, qmax, xrows = case
        if q >= qmax:   # the planner's own choice: runs inside pytest
            continue
        if longest_item(rows, pairs, dim) != (q, xrows):
            print("MISMATCH: plan of %s under SPECTAVI_L1K2_Q=%d: %s" % (name, q, longest_item(rows, pairs, dim)), flush=True)
            return 1
        if plan_only:
            continue
        tables = case_tables(case)
        try:
            check_pairs(oracle, tables, pairs, *run_device(tables, pairs))
        except AssertionError as e:
            print("MISMATCH: %s under SPECTAVI_L1K2_Q=%d: %s" % (name, q, e), flush=True)
            return 1
    print("ok q=%d" % q, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(int(sys.argv[1]), "--plan-only" in sys.argv[2:]))
