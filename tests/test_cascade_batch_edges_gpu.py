"""GPU parity of cascade_batch.hip on the paths tests/test_cascade_batch_gpu.py never runs: bucket bits above 12 and
below it (the memory cap), the full-code filter over a bucket of several 64-entry steps and two codes, probes whose
buckets fit the LDS list one by one but not together, the second trip of the rank / fill loops, and every
projection form.  Every comparison is check_collection's: array_equal on ncand, dist and idx against the CPU
oracle of each pair.  tests/test_cascade_batch_edge_cases.py shows, without a GPU, that each collection reaches
the path it is named after."""
import numpy as np
import pytest

from tests import cascade_batch_cases as cb
from tests import cascade_variant_cases as cv
from tests.test_cascade_batch_edge_cases import plan_of
from tests.test_cascade_batch_gpu import check_collection

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("big,m,hb", cb.BITS_EDGE, ids=lambda v: str(v))
def test_bucket_bits_at_the_4096_rows_edge(big, m, hb):
    case = cb.bits_edge(big, m)
    assert plan_of(case)["hb"] == hb
    check_collection(*case)


def test_results_do_not_depend_on_the_bucket_bits():
    """One pair of small sets alone (hb = 12), beside a set of 4097 rows (13) and beside one of 70000 (17): the
    pair's slices are the same bytes, and the oracle's."""
    slices = []
    for rows, hb in cb.BYSTANDERS:
        case = cb.invariance(rows)
        assert plan_of(case)["hb"] == hb
        got, _ = check_collection(*case)
        slices.append(tuple(a.tobytes() for a in got[:3]) + (got[3].tolist(),))
    assert slices[1] == slices[0], "hb = 13 differs from hb = 12"
    assert slices[2] == slices[0], "hb = 17 differs from hb = 12"


def test_the_memory_cap_32767_sets_of_two_tables():
    """hb = 11: 65534 bucket tables, the largest blockIdx.y of the scan kernels, a bisection over 32767 sets (most of
    them of 0, 1 or 2 rows) and bucket offsets half a GiB into the workspace.  Out of memory is a failure."""
    case = cb.cap()
    plan = plan_of(case)
    assert plan["hb"] == 11 and plan["workspace_bytes"] < 2 ** 30
    check_collection(*case)


@pytest.mark.parametrize("n", cb.FILTER_TABLES, ids=["two-tables", "one-table"])
def test_full_code_filter_over_a_bucket_of_two_interleaved_codes(n):
    """With one table the kept half of the mixed bucket is all a query sees: entries lost or misplaced by the
    compaction change its neighbours.  With two, the second table's bucket holds the same rows under one code."""
    case = cb.mixed_bucket(n)
    (idx, dist, ncand, out_off), _ = check_collection(*case)
    assert (ncand[:40] == 150 * n).all() and (ncand[40:] == 20 * n).all()   # half of each mixed bucket, all of table 1's


def test_full_code_filter_over_a_long_bucket_of_one_code():
    case = cb.long_bucket(cb.FILTER_SHAPE)
    assert plan_of(case)["hb"] == 12
    (idx, dist, ncand, out_off), _ = check_collection(*case)
    assert np.array_equal(idx[cb.LONG_HIT], np.tile(np.array([0, 1], np.uint64), (10, 1)))
    assert (dist[cb.LONG_HIT] == 0).all() and (ncand[cb.LONG_HIT] == 3000).all()


def test_buckets_that_fit_the_list_one_by_one_but_not_together():
    case = cb.bucket_sum()
    (idx, dist, ncand, out_off), _ = check_collection(*case)
    assert ncand[:100].min() > cb.LIST_CAP >= ncand[100:].max()


def test_rows_past_one_grid_of_the_rank_and_fill_loops():
    case = cb.stride()
    assert case[1][-1] > cb.GRID_ROWS
    (idx, dist, ncand, out_off), _ = check_collection(*case)
    assert (ncand[:300] >= 1).all() and (idx[:300, 0] >= 50).mean() >= 0.9


FORM_CASES = [c for c in cv.CASES if c[0] <= 256 and tuple(c[:4]) not in cb.EDGES]


@pytest.mark.parametrize("case", FORM_CASES, ids=cv.case_id)
def test_every_projection_form(case):
    from spectavi_amd import device
    dim, m, n, g, form = case
    assert device.cascade_plan(0, sum(cb.FORMS_ROWS), dim, m, n, g)["project_query"] == form
    x, seg, d = cb.collection(cb.FORMS_ROWS, dim, m, n, g)
    check_collection(x, seg, d, cb.FORMS_PAIRS, g)
