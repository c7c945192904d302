"""CPU-only: the argument rules of tracks_batch.  Every refusal is a ValueError from the Python wrappers before any
device is touched, and SPV_ERR_INVALID with a message from the C entries, which launch nothing; the workspace size
is 256-byte rounded and never decreases in either argument."""
import numpy as np
import pytest

SEG = [0, 3, 3, 10]
PAIRS = [[2, 0], [1, 0]]

# (what, seg_off, pairs, capacity, min_len)
REFUSALS = [
    ("seg_off does not start at 0", [1, 3, 10], PAIRS, 4, 2),
    ("seg_off decreases", [0, 5, 4, 10], PAIRS, 4, 2),
    ("2^31 rows", [0, 3, 2 ** 31], [[0, 1]], 4, 2),
    ("a pair names a set that is not there", SEG, [[3, 0]], 4, 2),
    ("a pair names a negative set", SEG, [[0, -1]], 4, 2),
    ("2^31 out rows", [0, 2 ** 30], [[0, 0], [0, 0]], 4, 2),
    ("negative capacity", SEG, PAIRS, -1, 2),
    ("min_len 1", SEG, PAIRS, 4, 1),
    ("min_len 0", SEG, PAIRS, 4, 0),
]


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_wrapper_refuses(case):
    import torch
    from spectavi_amd import device
    _, seg, pairs, cap, min_len = case
    with pytest.raises(ValueError):
        device._tracks_batch_args(seg, pairs, cap, min_len)
    if cap >= 0:   # (a tensor cannot have a negative capacity); CPU tensors: the rules come before the device
        with pytest.raises(ValueError):
            device.tracks_batch(seg, pairs, torch.zeros((cap, 2), dtype=torch.int32), torch.zeros(1, dtype=torch.int32),
                                min_len=min_len)


def test_wrapper_accepts_the_legal_edge_forms():
    from spectavi_amd import device
    seg, prs = device._tracks_batch_args(SEG, PAIRS + [[2, 2], [2, 0]], 0, 2)     # self and duplicate pairs, no capacity
    assert seg.dtype == np.int64 and prs.dtype == np.int32 and prs.shape == (4, 2)
    seg, prs = device._tracks_batch_args([0], [], 5, 7)                            # no set, no pair
    assert seg.tolist() == [0] and prs.shape == (0, 2)


def test_host_wrapper_refuses():
    from spectavi_amd import feature
    one = [np.zeros((0, 2), np.int32)]
    for sizes, pairs, matches, kw in (
            ([3, -1], [[1, 0]], one, {}),
            ([3, 4], [[2, 0]], one, {}),
            ([3, 4], [[1, 0]], one, {"min_len": 1}),
            ([3, 4], [[1, 0]], one + one, {}),
            ([3, 4], [[1, 0]], one, {"masks": [np.ones(3, np.uint8)]}),
            ([2 ** 30, 2 ** 30], [[1, 0]], one, {}),
            ([2 ** 30], [[0, 0], [0, 0]], one + one, {})):
        with pytest.raises(ValueError):
            feature.match_tracks_batch(sizes, pairs, matches, **kw)


@pytest.mark.parametrize("case", REFUSALS, ids=[c[0] for c in REFUSALS])
def test_c_entries_refuse(case):
    """Fake device pointers: a call that gets as far as a launch would fault, SPV_ERR_INVALID comes before."""
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    _, seg, pairs, cap, min_len = case
    seg = np.asarray(seg, np.int64)
    prs = np.asarray(pairs, np.int32).reshape(-1, 2)
    fake = np.zeros(64, np.int64)
    p = fake.ctypes.data
    st = clib.spv_tracks_batch_device(seg.ctypes.data, len(seg) - 1, prs.ctypes.data, len(prs), p, p, cap, None, min_len, 0,
                                      p, p, p, p, p, p, p, 1 << 40, None)
    assert st == SPV_ERR_INVALID and clib.spv_last_error()
    out = np.full(64, 7, np.int64)
    o = out.ctypes.data
    st = clib.spv_tracks_batch(seg.ctypes.data, len(seg) - 1, prs.ctypes.data, len(prs), p, cap, None, min_len, 0, o, o, o, o,
                               o, o)
    assert st == SPV_ERR_INVALID and clib.spv_last_error() and (out == 7).all()


def test_c_entries_refuse_counts_and_pointers():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    seg, prs = np.asarray(SEG, np.int64), np.asarray(PAIRS, np.int32)
    fake = np.zeros(64, np.int64)
    p = fake.ctypes.data

    def call(seg_p=seg.ctypes.data, nseg=3, prs_p=prs.ctypes.data, npairs=2, label=p, counts=p, ws=p, ws_bytes=1 << 40):
        return clib.spv_tracks_batch_device(seg_p, nseg, prs_p, npairs, p, p, 4, None, 2, 0, label, p, p, p, p, counts, ws,
                                            ws_bytes, None)
    for kw in (dict(nseg=-1), dict(npairs=-1), dict(seg_p=None), dict(prs_p=None), dict(label=None), dict(counts=None),
               dict(ws=None), dict(ws_bytes=256), dict(ws=p + 4)):
        assert call(**kw) == SPV_ERR_INVALID and clib.spv_last_error(), kw


def test_workspace_bytes():
    from spectavi_amd._lib import clib
    values = [0, 1, 255, 256, 257, 100000]
    size = {(n, c): clib.spv_tracks_batch_workspace_bytes(n, c) for n in values for c in values}
    assert all(b > 0 and b % 256 == 0 for b in size.values())
    for a, b in zip(values[:-1], values[1:]):
        for other in values:
            assert size[(a, other)] <= size[(b, other)] and size[(other, a)] <= size[(other, b)]
    assert size[(100000, 0)] >= 100000 * 21          # parent sizes, two key buffers, the digit counts
    assert clib.spv_tracks_batch_workspace_bytes(-1, 0) == 0 and clib.spv_tracks_batch_workspace_bytes(0, -1) == 0
    assert clib.spv_tracks_batch_workspace_bytes(2 ** 31, 0) == 0
