"""GPU parity of every projection kernel instantiation the cascade's default selection can pick
(launch_project / launch_project_mfma in spectavi_amd/csrc/cascade.hip), one (dim, m, n, g) per
query-side instantiation -- the database side of the same case runs the matching <.., false, 1>
form -- plus the probe forms that only the per-call SPECTAVI_CASCADE_RU8 switch reaches at widths
that are not a power of two.  Candidate counts, indices and distances bit-exact vs the oracle."""
import numpy as np
import pytest

from tests.cascade_variant_cases import CASES, cascade_data, projection_kernels

pytestmark = pytest.mark.gpu


def _check(oracle, x, y, d, m, n, g):
    from spectavi_amd import feature
    idx, dist, ncand = feature.nn_cascading_hash_with_dict(x, y, d, g=g, return_ncand=True)
    oidx, odist, oncand, _ = oracle.nn_cascading_hash(x, y, m, n, g, d)
    assert np.array_equal(ncand, oncand)
    assert np.array_equal(dist, odist)
    assert np.array_equal(idx, oidx)


@pytest.mark.parametrize("dim,m,n,g", CASES, ids=["%s-%dd-m%dn%dg%d" % ((projection_kernels(*c)[1],) + c)
                                                  for c in CASES])
def test_projection_variant_matches_oracle(oracle, dim, m, n, g):
    x, y, d = cascade_data(dim, m, n, g)
    _check(oracle, x, y, d, m, n, g)


@pytest.mark.parametrize("dim", [48, 80, 96, 112])
def test_probe_forms_at_non_power_of_two_widths(oracle, monkeypatch, dim):
    """Rows of at most 128 bytes whose width is not a power of two take the non-shift probe forms:
    probe_table_kernel<1, 8, 7, false, false> by default and <1, 4, 8, false, false> with
    SPECTAVI_CASCADE_RU8=0 (read per call), each in the one-pass and the sorted (per-table) form."""
    m, n, g = 9, 2, 3
    x, y, d = cascade_data(dim, m, n, g)
    for sort in ("0", "1"):
        monkeypatch.setenv("SPECTAVI_CASCADE_SORT", sort)
        for ru8 in ("1", "0"):
            monkeypatch.setenv("SPECTAVI_CASCADE_RU8", ru8)
            _check(oracle, x, y, d, m, n, g)
