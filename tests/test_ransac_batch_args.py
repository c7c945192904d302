"""The many-sets RANSAC and the batch gather without a GPU: what spv_ransac_fit_batch / _device reject (with no
device touched and no output written), the same through the Python layers, collections in which no set runs, and
the work items of a round (spv_ransac_fit_batch_plan): never across two sets, every (row, candidate) once, a
set's candidates cut over several items when the round has few row blocks."""
import ctypes as ct

import numpy as np
import pytest

SPV_OK, SPV_ERR_INVALID = 0, 1
SENTINEL = 77


def _outputs(npairs, total):
    return dict(success=np.full(npairs, SENTINEL, np.int32), essential=np.full((npairs, 9), 7.5),
                camera=np.full((npairs, 12), 7.5), inlier_percent=np.full(npairs, 7.5),
                inlier_idx=np.full(max(total, 1), SENTINEL, np.int32), n_inliers=np.full(npairs, SENTINEL, np.int32),
                best_try=np.full(npairs, SENTINEL, np.int32), best_root=np.full(npairs, SENTINEL, np.int32),
                tries_run=np.full(npairs, SENTINEL, np.int32))


def _untouched(out):
    return all(np.all(v == (SENTINEL if v.dtype == np.int32 else 7.5)) for v in out.values())


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _call(entry, x0, x1, off, npairs, tries, samples, seeds, out, drop=()):
    """entry 'host' or 'device' (the latter with host arrays standing in for device memory: every call here must
    return before it looks at them)."""
    from spectavi_amd._lib import clib
    o = {k: (None if k in drop else v) for k, v in out.items()}
    args = [_ptr(x0) if 'x0' not in drop else None, _ptr(x1) if 'x1' not in drop else None,
            _ptr(off) if 'pair_off' not in drop else None, npairs, 0.5, 1e-3, tries, 1, 3e-2, _ptr(samples), _ptr(seeds),
            _ptr(o['success']), _ptr(o['essential']), _ptr(o['camera']), _ptr(o['inlier_percent']), _ptr(o['inlier_idx']),
            _ptr(o['n_inliers']), _ptr(o['best_try']), _ptr(o['best_root']), _ptr(o['tries_run'])]
    if entry == 'host':
        return clib.spv_ransac_fit_batch(*args)
    return clib.spv_ransac_fit_batch_device(*args, None, None)


def _two_sets():
    rng = np.random.default_rng(1)
    x0, x1 = rng.standard_normal((32, 3)), rng.standard_normal((32, 3))
    off = np.array([0, 12, 32], np.int64)
    samples = np.tile(np.arange(1, 8, dtype=np.int32), (2, 5, 1))  # rows 1..7: inside both sets
    return x0, x1, off, samples


@pytest.mark.parametrize("entry", ["host", "device"])
def test_rejected_arguments_touch_nothing(entry):
    from spectavi_amd._lib import clib
    x0, x1, off, samples = _two_sets()
    seeds = np.array([3, 4], np.uint64)

    def rejected(**kw):
        out = _outputs(2, 32)
        a = dict(x0=x0, x1=x1, off=off, npairs=2, tries=5, samples=samples, seeds=None, out=out)
        a.update(kw)
        st = _call(entry, **a)
        assert st == SPV_ERR_INVALID and clib.spv_last_status() == SPV_ERR_INVALID, kw
        assert _untouched(out), kw

    for name in ('x0', 'x1', 'pair_off', 'success', 'essential', 'camera', 'inlier_percent', 'inlier_idx', 'n_inliers'):
        rejected(drop=(name,))
    rejected(samples=None, seeds=None)  # neither samples nor seeds
    rejected(npairs=-1)
    for bad in ([1, 12, 32], [0, 13, 12], [0, 12, 2 ** 31]):  # not from 0, decreasing, 2^31 rows
        rejected(off=np.array(bad, np.int64))
    rejected(tries=-1, samples=None, seeds=seeds)
    rejected(tries=700000001, samples=None, seeds=seeds)
    for p, v in ((0, 12), (1, 20), (0, -1)):  # row 12 of 12, row 20 of 20, a negative row
        s = samples.copy()
        s[p, 4, 6] = v
        rejected(samples=s)
    s = samples.copy()
    s[0, 0, 0] = 13  # a row of the NEXT set is still outside this one
    rejected(samples=s)


def test_python_layers_raise_value_error_before_a_device():
    import torch
    from spectavi_amd import device as spv
    from spectavi_amd import mvg
    x0, x1, off, samples = _two_sets()
    t0, t1 = torch.from_numpy(x0), torch.from_numpy(x1)  # host tensors: a call that got past its checks would TypeError
    bad = samples.copy()
    bad[0, 0, 0] = 12
    for kw in (dict(pair_off=[1, 12, 32], samples=samples), dict(pair_off=[0, 13, 12], samples=samples),
               dict(pair_off=[0, 12, 31], samples=samples), dict(pair_off=off, samples=bad),
               dict(pair_off=off, samples=samples[:1]), dict(pair_off=off, samples=samples[:, :, :6]),
               dict(pair_off=off, maximum_tries=-1), dict(pair_off=off, maximum_tries=700000001),
               dict(pair_off=off, seeds=[1, 2, 3])):
        with pytest.raises(ValueError):
            spv.ransac_fit_batch(t0, t1, **kw)
    with pytest.raises(ValueError):
        spv.ransac_fit_batch(t0, t1[:31], off, samples=samples)
    sets0, sets1 = [x0[:12], x0[12:]], [x1[:12], x1[12:]]
    for kw in (dict(samples=[bad[0], bad[1]]), dict(samples=[samples[0]]), dict(samples=[samples[0], samples[1][:4]]),
               dict(maximum_tries=-1), dict(maximum_tries=700000001), dict(seeds=[1])):
        with pytest.raises(ValueError):
            mvg.ransac_fit_batch(sets0, sets1, **kw)
    with pytest.raises(ValueError):
        mvg.ransac_fit_batch(sets0, sets1[:1])
    with pytest.raises(TypeError):
        mvg.ransac_fit_batch(sets0, [x1[:12], x1[12:31]])
    # the batch gather: the checks of l1k2_batch on seg_off and pairs
    geom = torch.zeros((32, 4), dtype=torch.float32)
    matches, count = torch.zeros((8, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    for seg, prs in (([1, 12, 32], [[0, 1]]), ([0, 13, 12], [[0, 1]]), ([0, 12, 31], [[0, 1]]), ([0, 12, 32], [[0, 2]]),
                     ([0, 12, 32], [[-1, 0]]), ([0, 12, 32], [0, 1])):
        with pytest.raises(ValueError):
            spv.match_coordinates_batch(geom, seg, prs, matches, count)
    with pytest.raises(ValueError):
        spv.match_coordinates_batch(geom[:, :3], [0, 12, 32], [[0, 1]], matches, count)


def test_gather_batch_rejects_at_the_c_entry():
    from spectavi_amd._lib import clib
    fake = np.zeros(64, np.int64)  # stands in for device memory: the call returns before it looks at it

    def st(seg, prs, npairs=None, cap=4):
        seg, prs = np.array(seg, np.int64), np.array(prs, np.int32).reshape(-1, 2)
        return clib.spv_gather_match_coords_batch_device(fake.ctypes.data, seg.ctypes.data, len(seg) - 1, prs.ctypes.data,
                                                         len(prs) if npairs is None else npairs, fake.ctypes.data,
                                                         fake.ctypes.data, cap, fake.ctypes.data, fake.ctypes.data,
                                                         fake.ctypes.data, None)
    assert st([1, 5], [[0, 0]]) == SPV_ERR_INVALID
    assert st([0, 5, 4], [[0, 1]]) == SPV_ERR_INVALID
    assert st([0, 5, 2 ** 31], [[0, 1]]) == SPV_ERR_INVALID
    assert st([0, 5, 9], [[0, 2]]) == SPV_ERR_INVALID
    assert st([0, 5, 9], [[-1, 1]]) == SPV_ERR_INVALID
    assert st([0, 5, 9], [[0, 1]], npairs=-1) == SPV_ERR_INVALID
    assert st([0, 5, 9], [[0, 1]], cap=-1) == SPV_ERR_INVALID
    assert not fake.any()


def test_collections_in_which_no_set_runs_need_no_device():
    from spectavi_amd import mvg
    rng = np.random.default_rng(2)
    sizes = [0, 9, 3, 0, 1]
    x0 = rng.standard_normal((sum(sizes), 3))
    x1 = rng.standard_normal((sum(sizes), 3))
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    samples = np.full((5, 4, 7), 1000, np.int32)  # not read: no set is large enough to own a subset
    for entry in ('host', 'device'):
        out = _outputs(5, 13)
        assert _call(entry, x0, x1, off, 5, 4, samples, None, out) == SPV_OK
        assert np.all(out['success'] == 0) and np.all(out['n_inliers'] == 0) and np.all(out['inlier_percent'] == 0.0)
        assert np.all(out['best_try'] == -1) and np.all(out['best_root'] == -1) and np.all(out['tries_run'] == 0)
        assert np.all(out['essential'] == 7.5) and np.all(out['camera'] == 7.5) and np.all(out['inlier_idx'] == SENTINEL)
        # optional outputs may be NULL; no sets at all; sets that would run, with no tries
        assert _call(entry, x0, x1, off, 5, 4, samples, None, _outputs(5, 13), drop=('best_try', 'best_root', 'tries_run')) == SPV_OK
        assert _call(entry, None, None, np.zeros(1, np.int64), 0, 4, None, None, _outputs(0, 0)) == SPV_OK
    out = _outputs(2, 32)
    x0, x1, off2, _ = _two_sets()
    assert _call('host', x0, x1, off2, 2, 0, None, None, out) == SPV_OK  # maximum_tries = 0
    assert np.all(out['success'] == 0) and np.all(out['best_try'] == -1) and np.all(out['tries_run'] == 0)
    sets0 = [x0[:9], x0[:0], x0[9:12]]
    rows = mvg.ransac_fit_batch(sets0, [x1[:9], x1[:0], x1[9:12]], seeds=[1, 2, 3])
    assert len(rows) == 3
    for r in rows:
        assert r == dict(r, success=False, essential=None, camera=None, inlier_percent=0.0, best_try=-1, best_root=-1,
                         tries_run=0) and len(r['inlier_idx']) == 0
    assert mvg.ransac_fit_batch([], []) == []


def _check_items(off, tries, cus):
    from spectavi_amd import device as spv
    plan, items = spv.ransac_fit_batch_plan(off, tries, cus, want_items=True)
    assert len(items) == plan['items']
    off = np.asarray(off)
    seen = {}
    for s, row0, rows, c0, nc in items:
        assert 1 <= rows <= 256 and nc >= 1
        assert off[s] <= row0 and row0 + rows <= off[s + 1]  # never across two sets
        seen.setdefault(s, []).append((row0, rows, c0, nc))
    for s, its in seen.items():
        npt = off[s + 1] - off[s]
        assert npt >= 10
        cands = sorted({(c0, nc) for _, _, c0, nc in its})
        blocks = sorted({(r0, r) for r0, r, _, _ in its})
        # a grid: every row block meets every candidate range once, and both tile their extent
        assert len(its) == len(cands) * len(blocks) == len(set(its))
        assert blocks[0][0] == off[s] and all(a[0] + a[1] == b[0] for a, b in zip(blocks, blocks[1:]))
        assert blocks[-1][0] + blocks[-1][1] == off[s + 1] and len(blocks) == -(-npt // 256)
        assert all(a[0] + a[1] == b[0] for a, b in zip(cands, cands[1:]))
        assert (cands[-1][0] + cands[-1][1] - cands[0][0]) % 3 == 0
    total_c = sorted((min(c0 for _, _, c0, _ in its), max(c0 + nc for _, _, c0, nc in its)) for its in seen.values())
    assert total_c[0][0] == 0 and all(a[1] == b[0] for a, b in zip(total_c, total_c[1:]))  # the sets' candidates tile the round's
    assert total_c[-1][1] == 3 * plan['tries'] and len(seen) == plan['sets']
    return plan, items


def test_plan_cuts_candidates_when_row_blocks_are_few():
    # 64 sets of 500 rows: 128 row blocks for 256 compute units -- each set's 768 first-round candidates are cut
    off = np.arange(65, dtype=np.int64) * 500
    plan, items = _check_items(off, 500, 256)
    assert plan['sets'] == 64 and plan['row_blocks'] == 128 and plan['tries'] == 64 * 256
    assert plan['items'] >= 4 * 256 and len({tuple(i[3:]) for i in items if i[0] == 5}) == 8
    # many row blocks: one item per row block
    plan, _ = _check_items(np.arange(9, dtype=np.int64) * 50000, 500, 256)
    assert plan['items'] == plan['row_blocks'] == 8 * 196
    # small sets are skipped by the plan as by the call; sizes at the row-block edge
    plan, _ = _check_items(np.cumsum([0, 0, 9, 10, 255, 256, 257, 2500]), 60, 256)
    assert plan['sets'] == 5 and plan['row_blocks'] == 1 + 1 + 1 + 2 + 10 and plan['tries'] == 5 * 60
    # a round is bounded: 300 sets of 256 tries each do not fit one round
    plan, _ = _check_items(np.arange(301, dtype=np.int64) * 100, 1000, 64)
    assert plan['tries'] == 32768 and plan['sets'] == 128
