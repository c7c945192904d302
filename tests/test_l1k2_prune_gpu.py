"""The dim-128 bound path of the L1 2-NN (l1k2_prune.hip) forced on through spv_l1k2_set_prune(1), and
the plain tile kernel (0), against the CPU oracle and each other, bit for bit: more than two database
slices' worth of rows with a ragged tail, a query count that fills no whole block, and the inputs on
which a pruning kernel goes wrong (ties, the extreme distances, nothing to prune, duplicates in
different slices, real descriptors, a database shorter than a slice).

What these shapes reach, read against l1k2_plan(): with 8193 queries and the default 16384 wanted blocks
the 131109 rows fall into 683 slices of 192 rows, six 32-row tiles of the bound kernel each, the last
slice 165 rows (six tiles, 5 live rows in the last); "short" into 64-row slices of two tiles and a last
slice of one tile with 21 rows; "oneslice" is a single slice of two tiles, the second with 8 rows.  The
children with SPECTAVI_L1K2_BLOCKS=64 add four slices of 1026 tiles (the last 1020, again 5 live rows).
All of it with one query count, whose last block holds one live query.  The slice lengths in between, every ragged count, the query tails at
the edges of the MFMA column blocks, the hand-over placed on purpose and the keep rule at equality are
the business of tests/test_l1k2_prune_shapes_gpu.py and its case table tests/l1k2_prune_cases.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":   # run as the child of test_long_slices_in_a_child_process
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests.l1k2_variant_cases import GOLDEN, expected_dup_rows  # noqa: E402

pytestmark = pytest.mark.gpu

M, N = 131072 + 37, 8193


def _sift128(rows, rng):
    """The golden SIFT table's last 128 columns (the descriptor), tiled and perturbed as
    l1k2_variant_cases._sift_u8 does with the 144-column form."""
    import os
    t = np.load(os.path.join(GOLDEN, "sift_sur_ogre_table.npz"))["table"][:, -128:]
    u = np.clip(np.rint(t), 0, 255).astype(np.int16)
    out = u[rng.permutation(len(u))][np.arange(rows) % len(u)]
    noisy = rng.random(rows) < 0.5
    out[noisy] += rng.integers(-3, 4, (int(noisy.sum()), 128)).astype(np.int16)
    return np.clip(out, 0, 255).astype(np.uint8)


def _data(kind):
    rng = np.random.default_rng([len(kind), ord(kind[0]), ord(kind[-1])])
    m = {"short": 40000 + 21, "oneslice": 40}.get(kind, M)   # "oneslice": 32 <= rows < 64, a single slice
    if kind in ("uniform", "short", "dups", "oneslice"):
        x = rng.integers(0, 256, (m, 128), dtype=np.uint8)
        y = rng.integers(0, 256, (N, 128), dtype=np.uint8)
    elif kind == "bits01":
        x = rng.integers(0, 2, (m, 128), dtype=np.uint8)
        y = rng.integers(0, 2, (N, 128), dtype=np.uint8)
    elif kind == "bits0255":
        x = rng.integers(0, 2, (m, 128), dtype=np.uint8) * 255
        y = rng.integers(0, 2, (N, 128), dtype=np.uint8) * 255
        x[5], x[m - 2] = 0, 0
        y[3], y[N - 1] = 255, 255   # distance 32640 to the zero rows
        y[4] = 0                    # distance 0
    elif kind == "constant":
        x = np.full((m, 128), 93, np.uint8)
        y = np.full((N, 128), 93, np.uint8)
        y[::7] = 94
    elif kind == "sift":
        x, y = _sift128(m, rng), _sift128(N, rng)
    else:
        raise ValueError(kind)
    dups = []
    if kind == "dups":
        for j, k in enumerate(sorted({N - 1, N // 2, 0, 255, 256})):
            x[3 + 17 * j] = y[k]            # first slice
            x[70000 + j] = y[k]             # second slice
            x[m - 1 - j] = y[k]             # ragged tail
            dups.append(k)
    return x, y, dups


def _run(x, y, mode):
    """(idx, dist, (bounded, survivors, fallback pairs)) with the prune mode set for this call only."""
    import torch
    from spectavi_amd import device
    before = device.l1k2_get_prune()
    device.l1k2_set_prune(mode)
    try:
        xd, yd = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        idx, dist = device.l1k2(xd, yd)
        stats = device.l1k2_prune_stats()
        return idx.cpu().numpy().view(np.uint64), dist.cpu().numpy(), stats
    finally:
        device.l1k2_set_prune("auto" if before < 0 else before)


def check_case(kind, oracle_fn):
    """The body of the test, shared with the child process of the long-slice cases."""
    x, y, dups = _data(kind)
    oidx, odist = oracle_fn(x, y, nthreads=16)
    on_idx, on_dist, on_stats = _run(x, y, 1)
    again_idx, again_dist, _ = _run(x, y, 1)
    off_idx, off_dist, off_stats = _run(x, y, 0)
    assert np.array_equal(on_dist, odist) and np.array_equal(on_idx, oidx)
    assert np.array_equal(off_dist, odist) and np.array_equal(off_idx, oidx)
    # which pairs the shared thresholds skip depends on timing; the bytes that come out do not
    assert on_idx.tobytes() == again_idx.tobytes() and on_dist.tobytes() == again_dist.tobytes()
    # the forced path really ran the bound kernel, the other one did not
    assert on_stats[0] > 0 and on_stats[1] <= on_stats[0], on_stats
    assert off_stats == (0, 0, 0), off_stats
    if kind == "constant":   # nothing can be ruled out: the workgroups hand their slices to the exact kernel
        assert on_stats[2] > 0, on_stats
    for k in dups:
        assert np.array_equal(on_idx[k], expected_dup_rows(x, y, k).astype(np.uint64))
        assert np.array_equal(on_dist[k], [0, 0])
    return on_stats


@pytest.mark.parametrize("kind", ["uniform", "bits01", "bits0255", "constant", "dups", "sift", "short", "oneslice"])
def test_prune_on_and_off_match_the_oracle(oracle, kind):
    check_case(kind, oracle.nn_bruteforcel1k2)


@pytest.mark.parametrize("kind", ["constant", "sift", "uniform"])
def test_long_slices_in_a_child_process(kind):
    """With 8193 queries the plan cuts the database into slices of a few tiles.  SPECTAVI_L1K2_BLOCKS=64
    (read once per process, hence the child) makes them about a thousand tiles long, so that the
    hand-over to the exact kernel happens far from the end of a slice and thresholds travel through
    long slices."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("SPECTAVI_L1K2_")}
    env["SPECTAVI_L1K2_BLOCKS"] = "64"
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), kind]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0 and ("long slices ok: %s" % kind) in r.stdout, r.stdout


def test_setter_validates():
    from spectavi_amd import device
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    before = device.l1k2_get_prune()
    assert clib.spv_l1k2_set_prune(2) == SPV_ERR_INVALID
    for bad in (7, "on", [1], None, 1.0):
        with pytest.raises(ValueError):
            device.l1k2_set_prune(bad)
    device.l1k2_set_prune(0)
    assert device.l1k2_get_prune() == 0
    device.l1k2_set_prune("auto" if before < 0 else before)
    assert device.l1k2_get_prune() == before


if __name__ == "__main__":
    from oracle import oracle as _oracle
    from spectavi_amd import device as _device
    _plan = _device.l1k2_plan(M, N, 128)
    assert _plan["slice_rows"] >= 32 * 500, _plan
    check_case(sys.argv[1], _oracle.nn_bruteforcel1k2)
    print("long slices ok: %s" % sys.argv[1])
