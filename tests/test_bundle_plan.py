"""spv_bundle_adjust_plan without a GPU: the two forms around the lane/wave boundary, the longest track, and the chunks
of the view-major order on hand-made collections."""
import ctypes as ct

import numpy as np
import pytest


def plan_of(lengths, **kw):
    from spectavi_amd import device
    return device.bundle_adjust_plan(np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64), **kw)


def boundary():
    n = 1
    while plan_of([n + 1])["wave_tracks"] == 0:
        n += 1
    return n


def test_forms_and_longest():
    L = boundary()
    assert L >= 2
    lengths = [L - 1, L, L + 1, 2, 0, 1, 3, 300, 70, 64, 65]
    p = plan_of(lengths)
    wave = sum(1 for n in lengths if n > L)
    assert (p["lane_tracks"], p["wave_tracks"], p["longest"], p["chunks"]) == (len(lengths) - wave, wave, 300, 0)
    assert p["chunk"] >= 64 and p["chunk"] % 64 == 0
    assert plan_of([]) == dict(lane_tracks=0, wave_tracks=0, chunk=p["chunk"], chunks=0, longest=0)
    assert plan_of([L + 1] * 300)["lane_tracks"] == 0
    for bad in ([], [1, 2], [0, 3, 2], [0, 2 ** 31]):
        from spectavi_amd import device
        with pytest.raises(ValueError):
            device.bundle_adjust_plan(bad)


def collection(per_track_sets, rows):
    """Tracks given as lists of sets; member k of a track in set s names row (k-th use of s) % rows[s]."""
    used = [0] * len(rows)
    mem = []
    for sets in per_track_sets:
        for s in sets:
            mem.append((s, used[s] % max(rows[s], 1)))
            used[s] += 1
    return (np.array(mem, np.int32).reshape(-1, 2), np.concatenate([[0], np.cumsum(rows)]).astype(np.int64),
            [len(s) for s in per_track_sets])


def test_chunks_count_the_free_sets_lists():
    C = plan_of([2])["chunk"]
    # set 0 sees everything, set 1 exactly C tracks, set 2 C + 1, set 3 2 C + 1, set 4 one track alone with itself
    tracks = [[0] + [s for s, n in ((1, C), (2, C + 1), (3, 2 * C + 1)) if t < n] for t in range(2 * C + 1)]
    mem, seg, lengths = collection(tracks + [[4]], [2 * C + 1, C, C + 1, 2 * C + 1, 1])
    assert plan_of(lengths, members=mem, seg_off=seg)["chunks"] == 3 + 1 + 2 + 3        # set 4's track has one member
    assert plan_of(lengths, members=mem, seg_off=seg, mode=[2, 1, 1, 1, 1])["chunks"] == 1 + 2 + 3
    assert plan_of(lengths, members=mem, seg_off=seg, mode=[1, 2, 2, 1, 0])["chunks"] == 3 + 3
    # a set without a camera: its members are not usable and its list is not cut
    p = plan_of(lengths, members=mem, seg_off=seg, mode=[1, 0, 1, 1, 1])
    assert p["chunks"] == 3 + 2 + 3
    p = plan_of(lengths, members=mem, seg_off=seg, mode=[1, 0, 0, 0, 1])
    assert p["chunks"] == 0
    # garbage members count for nothing
    bad = mem.copy()
    bad[bad[:, 0] == 3] = (2 ** 31 - 1, -2 ** 31)
    assert plan_of(lengths, members=bad, seg_off=seg)["chunks"] == 2 + 1 + 2   # set 0 keeps the C + 1 tracks of two
    bad = mem.copy()
    bad[bad[:, 0] == 3, 1] = 2 * C + 1          # one past the set's last row
    assert plan_of(lengths, members=bad, seg_off=seg)["chunks"] == 2 + 1 + 2
    # two members of one set in one track are both counted
    mem2, seg2, len2 = collection([[0, 0]] * C + [[0, 0, 0]], [5])
    assert plan_of(len2, members=mem2, seg_off=seg2)["chunks"] == 3


def test_plan_entry_rejects():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    out = (ct.c_longlong * 5)(*[-7] * 5)
    ok = np.array([0, 2, 5], np.int64)
    mem, seg = np.zeros((5, 2), np.int32), np.array([0, 3], np.int64)

    def call(off, nt, members, sg, nseg, o):
        return clib.spv_bundle_adjust_plan(None if off is None else off.ctypes.data, nt, None if members is None else members.ctypes.data,
                                           None if sg is None else sg.ctypes.data, nseg, None, o)
    for args in ((None, 2, None, None, 0, out), (ok, -1, None, None, 0, out), (ok, 2, None, None, 0, None),
                 (np.array([1, 2, 5], np.int64), 2, None, None, 0, out), (np.array([0, 5, 2], np.int64), 2, None, None, 0, out),
                 (ok, 2, mem, None, 1, out), (ok, 2, mem, np.array([1, 3], np.int64), 1, out), (ok, 2, mem, seg, -1, out)):
        assert call(*args) == SPV_ERR_INVALID
        assert list(out) == [-7] * 5
    assert call(ok, 2, None, None, 0, out) == 0 and list(out)[:2] == [2, 0] and list(out)[3:] == [0, 3]
    assert call(ok, 2, mem, seg, 1, out) == 0 and list(out)[3] == 1
    from spectavi_amd import device
    for over in (dict(members=np.zeros((4, 2), np.int32), seg_off=[0, 3]), dict(members=mem, seg_off=[1, 3]),
                 dict(members=mem, seg_off=[0, 3], mode=[1, 1])):
        with pytest.raises(ValueError):
            device.bundle_adjust_plan(ok, **over)
