"""The dim-128 bound path of the L1 2-NN (l1k2_prune.hip) run with the tuned table (spv_l1k2_set_bound(1)) and forced
on: every case bit for bit against the CPU oracle with prune on (twice) and off, `bounded` equal to the numpy model's
(tests/l1k2_prune_model.py, run with the tuned table) and, where one slice makes them independent of timing, the
survivors too.  The shapes are the smallest at which the path can go wrong with another table: one tile against
1, 64, 65 and 257 queries, ragged tiles of 1 and 31 live rows, a last slice of one row, everything surviving (the
full queue), and, in a child process whose plan cuts two long slices (SPECTAVI_L1K2_BLOCKS is read once), two slices
of four tiles and the keep rule at equality on the tuned table's own tight byte pairs."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_two_slices_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import l1k2_prune_cases as pc  # noqa: E402
from tests import l1k2_prune_model as pm  # noqa: E402
from tests.test_l1k2_bound_tuned import TUNED, table_of  # noqa: E402
from tests.test_l1k2_prune_gpu import _run  # noqa: E402

pytestmark = pytest.mark.gpu

CHILD_TIMEOUT = 120

# (rows, queries, kind) in the test process: 64-row slices, so all but 65 x 65 are a single slice
DEFAULT_CASES = [(32, 1, "uniform"), (32, 64, "uniform"), (32, 65, "uniform"), (32, 257, "uniform"),
                 (33, 65, "uniform"), (63, 65, "uniform"), (65, 65, "uniform"), (64, 300, "constant")]


def run_tuned(x, y, mode):
    from spectavi_amd import device
    before = device.l1k2_get_bound()
    device.l1k2_set_bound(TUNED)
    try:
        return _run(x, y, mode)
    finally:
        device.l1k2_set_bound(before)


def tight_case(table, slice_rows, xrows, yrows):
    """The "tight" recipe of tests/l1k2_prune_cases.py on this table's tight pair: constant queries of byte q_b, rows
    of byte far_b whose bound equals their distance.  Slice 0 has two rows one unit per byte farther at its head (its
    own threshold) and the tight rows in its last two tiles; slice 1 begins with tight rows and publishes the tight
    distance early, so slice 0 meets its tight rows at sum == 128 m - p thr and must keep them: they are the result."""
    far_b, q_b = min(ab for ab in pc.tight_pairs(table) if ab[0] >= 4)
    rng = np.random.default_rng(5)
    y = np.full((yrows, 128), q_b, np.uint8)
    x = rng.integers(0, 2, (xrows, 128)).astype(np.uint8)          # bytes 0 / 1 < far_b - 1: farther than every row below
    x[0:2] = far_b - 1
    rows = [slice_rows - 2 * pc.TILE + 7, slice_rows - 2 * pc.TILE + 30, slice_rows - pc.TILE + 4, slice_rows - pc.TILE + 5,
            slice_rows - 1]
    x[rows] = far_b
    x[slice_rows:slice_rows + 4] = far_b
    return x, y, {k: (rows[0], rows[1]) for k in (0, yrows // 2, yrows - 1)}


def check(name, x, y, expect, oracle_fn, blocks):
    from spectavi_amd import device
    table = table_of(TUNED)
    plan = device.l1k2_plan(len(x), len(y), 128)
    slices, slice_rows, _ = pc.plan_of(len(x), len(y), blocks)
    assert (plan["slices"], plan["slice_rows"]) == (slices, slice_rows), (name, plan)
    oidx, odist = oracle_fn(x, y)
    pre = pm.prepare(x, y, table)
    model = [pm.run(x, y, table, blocks, pc.BREAK_EVEN_SHARE, s, None, pre) for s in pm.SCHEDULES]
    for idx, dist, _ in model:
        assert np.array_equal(idx[:len(y)], oidx) and np.array_equal(dist[:len(y)], odist), name
    assert len({(m[2][0], m[2][2]) for m in model}) == 1, name      # the case was chosen so that no schedule moves these
    want = model[0][2]
    runs = [run_tuned(x, y, 1), run_tuned(x, y, 1), run_tuned(x, y, 0)]
    for what, (idx, dist, stats) in zip(("prune on", "prune on, second run", "prune off"), runs):
        print("%s, %s: statistics %r, model %r" % (name, what, stats, want), flush=True)
        assert idx.tobytes() == oidx.tobytes() and dist.tobytes() == odist.tobytes(), (name, what)
    for k, rows in expect.items():
        assert tuple(int(v) for v in runs[0][0][k]) == rows, (name, k)
    for _, _, stats in runs[:2]:
        assert (stats[0], stats[2]) == (want[0], want[2]), (name, stats, want)
        assert 0 < stats[1] <= stats[0], (name, stats)
        if slices == 1:
            assert stats[1] == want[1], (name, stats, want)
    assert runs[2][2] == (0, 0, 0), (name, runs[2][2])


@pytest.mark.parametrize("xrows,yrows,kind", DEFAULT_CASES, ids=lambda v: str(v))
def test_small_shapes_in_this_process(oracle, xrows, yrows, kind):
    c = pc._case("default", xrows, yrows, kind)
    x, y, expect = pc.make_case(c, table_of(TUNED))
    check(c.id, x, y, expect, oracle.nn_bruteforcel1k2, pc.blocks_of("default"))


def run_child_cases(oracle_fn):
    blocks = pc.blocks_of("two")
    table = table_of(TUNED)
    c = next(c for c in pc.cases_of("two") if c.id == "two-237x200-cluster")       # slices of 4 and 4 tiles, 13 live rows
    x, y, expect = pc.make_case(c, table)
    check(c.id, x, y, expect, oracle_fn, blocks)
    xrows, yrows = 2 * 64 * pc.TILE, 40                                            # two slices of 64 tiles
    x, y, expect = tight_case(table, pc.plan_of(xrows, yrows, blocks)[1], xrows, yrows)
    check("two-%dx%d-tight-tuned" % (xrows, yrows), x, y, expect, oracle_fn, blocks)


def test_two_slices_in_a_child_process():
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env.update(pc.SETTINGS["two"])
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__)]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=CHILD_TIMEOUT)
    print(r.stdout)
    assert r.returncode == 0 and "two slices ok" in r.stdout, r.stdout


if __name__ == "__main__":
    from oracle import oracle as _oracle
    run_child_cases(_oracle.nn_bruteforcel1k2)
    print("two slices ok")
