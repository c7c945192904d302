"""GPU parity of every projection kernel instantiation the cascade's default selection can pick
(cascade_plan in spectavi_amd/csrc/cascade.hip), one (dim, m, n, g) per query-side instantiation --
the database side of the same case runs the matching <.., false, 1> form -- plus the non-shift
probe form at widths that are not a power of two.  Each test first asks the library's own plan
that it launches what the case is written for.  Candidate counts, indices and distances bit-exact
vs the oracle."""
import numpy as np
import pytest

from tests.cascade_variant_cases import CASES, cascade_data, case_id

pytestmark = pytest.mark.gpu


def _check(oracle, x, y, d, m, n, g):
    from spectavi_amd import feature
    idx, dist, ncand = feature.nn_cascading_hash_with_dict(x, y, d, g=g, return_ncand=True)
    oidx, odist, oncand, _ = oracle.nn_cascading_hash(x, y, m, n, g, d)
    assert np.array_equal(ncand, oncand)
    assert np.array_equal(dist, odist)
    assert np.array_equal(idx, oidx)


@pytest.mark.parametrize("dim,m,n,g,target", CASES, ids=[case_id(c) for c in CASES])
def test_projection_variant_matches_oracle(oracle, dim, m, n, g, target):
    from spectavi_amd import device
    x, y, d = cascade_data(dim, m, n, g)
    assert device.cascade_plan(len(x), len(y), dim, m, n, g)["project_query"] == target
    _check(oracle, x, y, d, m, n, g)


@pytest.mark.parametrize("dim", [48, 80, 96, 112])
def test_probe_forms_at_non_power_of_two_widths(oracle, monkeypatch, dim):
    """Rows of at most 128 bytes whose width is not a power of two take the non-shift probe form,
    probe_table_kernel<1, 8, 7, false, false>, in the one-pass and the sorted (per-table) form
    (SPECTAVI_CASCADE_SORT, read per call)."""
    from spectavi_amd import device
    m, n, g = 9, 2, 3
    x, y, d = cascade_data(dim, m, n, g)
    for sort in ("0", "1"):
        monkeypatch.setenv("SPECTAVI_CASCADE_SORT", sort)
        plan = device.cascade_plan(len(x), len(y), dim, m, n, g)
        assert plan["probe"] == "probe_table_kernel<1, 8, 7, false, false>" and plan["sorted"] == (sort == "1")
        _check(oracle, x, y, d, m, n, g)
