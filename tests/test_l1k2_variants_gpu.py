"""GPU parity of every L1 2-NN kernel instantiation: each case of tests/l1k2_variant_cases.py (every
(width, queries per lane) of l1k2_tile_kernel, both l1k2_wide_kernel forms, the three merge forms),
selected by the library's own plan, bit-equal to the oracle through the host ABI and the device path.
Every case has a ragged last slice, a last query block with a single live query at Q > 1, and exact
copies of queries in two slices; many use 2- or 3-letter alphabets so that ties decide the order."""
import numpy as np
import pytest

from tests import l1k2_variant_cases as lc
from tests.test_l1k2_gpu import _raw

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", lc.CASES, ids=[lc.case_id(c) for c in lc.CASES])
def test_variant_matches_oracle(oracle, case):
    import torch
    from spectavi_amd import device
    xrows, yrows, dim = case[:3]
    plan = device.l1k2_plan(xrows, yrows, dim)
    assert lc.plan_key(plan)[:2] == case[5], plan
    x, y, dups = lc.make_case(case)
    oidx, odist = oracle.nn_bruteforcel1k2(x, y, nthreads=oracle.max_threads())
    for k in dups:   # the fixture itself: both planted copies are the two nearest, lower index first
        rows = lc.expected_dup_rows(x, y, k)
        assert oidx[k].tolist() == rows.tolist() and odist[k].tolist() == [0, 0]
    # device path: one device, exactly the plan above
    didx, ddist = device.l1k2(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    torch.cuda.synchronize()
    assert np.array_equal(ddist.cpu().numpy(), odist)
    assert np.array_equal(didx.cpu().numpy().view(np.uint64), oidx)
    # host ABI (spv_nn_bruteforcel1k2: the queries are sharded when several devices are visible)
    idx, dist = _raw(x, y)
    assert np.array_equal(dist, odist)
    assert np.array_equal(idx, oidx)
