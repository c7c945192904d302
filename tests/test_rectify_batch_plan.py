"""Host only: the offsets and work items of rectify_batch (spv_rectify_batch_plan) against the shapes of the numpy
statement of the contract (tests/rectify_oracle.py), and the argument checks that run before any device is touched.
No GPU involved."""
import ctypes as ct

import numpy as np
import pytest

from tests import rectify_oracle as ro

# (wid, hgt) of six images of three sizes; pairs with a shared image (0), a repeat ((0, 1) twice) and a self pair
SIZES = [(50, 40), (50, 40), (131, 77), (131, 77), (7, 33), (50, 40)]
PAIRS = [(0, 1), (2, 3), (0, 5), (0, 1), (4, 4), (3, 2), (5, 1)]
USE = [1, 1, 0, 1, 1, 1, 1]
ITEM_ROWS = 8


def frames(nchan, sf, pairs=PAIRS, sizes=SIZES):
    return [ro.shape(sizes[a][0], sizes[a][1], nchan, sf)[:2] for a, _ in pairs]


def check_items(items, pairs, use, box):
    """Every window row of both images of every used pair exactly once, pair by pair; no item straddles pairs."""
    assert items.dtype == np.int32 and items.shape[1] == 4
    seen = {}
    order = []
    for p, img, row0, rows in items.tolist():
        assert 0 <= p < len(pairs) and img in (0, 1) and 1 <= rows <= ITEM_ROWS
        assert use[p] and box[p][3] > box[p][2], "an item of a pair that owns no sample"
        assert box[p][0] <= row0 and row0 + rows <= box[p][1], "an item leaves its pair's window"
        for r in range(row0, row0 + rows):
            assert (p, img, r) not in seen, "a window row is covered twice"
            seen[(p, img, r)] = True
        if not order or order[-1] != p:
            order.append(p)
    want = {(p, img, r) for p in range(len(pairs)) if use[p] and box[p][3] > box[p][2]
            for img in (0, 1) for r in range(box[p][0], box[p][1])}
    assert set(seen) == want
    assert order == sorted(set(order)), "the items of a pair are not contiguous"


@pytest.mark.parametrize("nchan,sf", [(1, 1.2), (3, 1.2), (1, 0.5), (2, 2.2)])
def test_whole_frames_match_the_oracle_shapes(nchan, sf):
    from spectavi_amd import device
    fr = frames(nchan, sf)
    plan, items = device.rectify_batch_plan(SIZES, PAIRS, nchan, sf, use=USE, want_items=True)
    sizes = [r * c if u else 0 for (r, c), u in zip(fr, USE)]
    assert plan["pairs"] == sum(USE) and plan["samples"] == sum(sizes) and plan["items"] == len(items)
    assert plan["out_off"].dtype == np.int64
    assert plan["out_off"].tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    box = [(0, r, 0, c) for r, c in fr]
    check_items(items, PAIRS, USE, box)
    assert len(items) == sum(2 * -(-r // ITEM_ROWS) for (r, c), u in zip(fr, USE) if u)
    # use = None takes every pair
    plan_all = device.rectify_batch_plan(SIZES, PAIRS, nchan, sf)
    assert plan_all["pairs"] == len(PAIRS) and plan_all["samples"] == sum(r * c for r, c in fr)


def test_caller_boxes():
    from spectavi_amd import device
    fr = frames(1, 1.2)
    box = [(3, 30, 5, 41), (0, fr[1][0], 0, fr[1][1]), (1, 2, 3, 4), (17, 18, 0, fr[3][1]), (4, 4, 0, 3),
           (9, 20, 6, 6), (fr[6][0] - 1, fr[6][0], fr[6][1] - 1, fr[6][1])]
    plan, items = device.rectify_batch_plan(SIZES, PAIRS, 1, 1.2, use=USE, box=box, want_items=True)
    sizes = [(b[1] - b[0]) * (b[3] - b[2]) if u else 0 for b, u in zip(box, USE)]
    assert plan["out_off"].tolist() == np.concatenate([[0], np.cumsum(sizes)]).tolist()
    assert plan["samples"] == sum(sizes) and plan["pairs"] == sum(USE)
    check_items(items, PAIRS, USE, box)
    assert not (items[:, 0] == 4).any() and not (items[:, 0] == 5).any()  # a window without a sample owns no item
    assert items[items[:, 0] == 3].tolist() == [[3, 0, 17, 1], [3, 1, 17, 1]]  # the single-row window
    # the box of a pair that is not used is not read
    box[2] = (-7, 10 ** 6, 5, 1)
    again = device.rectify_batch_plan(SIZES, PAIRS, 1, 1.2, use=USE, box=box)
    assert again["out_off"].tolist() == plan["out_off"].tolist()


def test_empty_collections_are_valid():
    from spectavi_amd import device
    for sizes, pairs, use in (([], [], None), (SIZES, [], None), (SIZES, PAIRS, [0] * len(PAIRS))):
        plan, items = device.rectify_batch_plan(sizes, pairs, use=use, want_items=True)
        assert (plan["pairs"], plan["items"], plan["samples"]) == (0, 0, 0) and len(items) == 0
        assert plan["out_off"].tolist() == [0] * (len(pairs) + 1)


def test_short_items_buffer_receives_the_first_items():
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    _, items = device.rectify_batch_plan(SIZES, PAIRS, use=USE, want_items=True)
    sizes, pairs, use = (np.array(a, np.int32) for a in (SIZES, PAIRS, USE))
    out = (ct.c_longlong * 3)()
    off = np.zeros(len(PAIRS) + 1, np.int64)
    few = np.full((3, 4), -5, np.int32)
    assert clib.spv_rectify_batch_plan(sizes.ctypes.data, len(SIZES), 1, 1.2, pairs.ctypes.data, len(PAIRS),
                                       use.ctypes.data, None, out, off.ctypes.data, few.ctypes.data, 2) == 0
    assert np.array_equal(few[:2], items[:2]) and few[2].tolist() == [-5] * 4 and out[1] == len(items)


def test_plan_rejects_bad_arguments_and_leaves_outputs_untouched():
    from spectavi_amd._lib import clib, SPV_ERR_INVALID
    fr = frames(1, 1.2)
    good_box = [(0, r, 0, c) for r, c in fr]

    def call(sizes=SIZES, nimg=None, nchan=1, sf=1.2, pairs=PAIRS, npairs=None, use=USE, box=None, out=True,
             off=True, items_cap=4, null_sizes=False, null_pairs=False):
        s = np.array(sizes, np.int32).reshape(-1, 2)
        p = np.array(pairs, np.int32).reshape(-1, 2)
        u = None if use is None else np.array(use, np.int32)
        b = None if box is None else np.array(box, np.int32)
        o = (ct.c_longlong * 3)(-7, -7, -7)
        oo = np.full(len(p) + 1, -7, np.int64)
        it = np.full((4, 4), -7, np.int32)
        st = clib.spv_rectify_batch_plan(None if null_sizes else s.ctypes.data, len(s) if nimg is None else nimg, nchan, sf,
                                         None if null_pairs else p.ctypes.data, len(p) if npairs is None else npairs,
                                         None if u is None else u.ctypes.data, None if b is None else b.ctypes.data,
                                         o if out else None, oo.ctypes.data if off else None, it.ctypes.data, items_cap)
        return st, list(o), oo, it

    st, o, oo, it = call()
    assert st == 0 and o[0] == sum(USE) and (oo >= 0).all() and (it[:, 0] == 0).all()

    def with_box(p, b):
        bx = list(good_box)
        bx[p] = b
        return bx
    bad = {
        "sf = 0": dict(sf=0.), "sf = nan": dict(sf=float("nan")), "sf = inf": dict(sf=float("inf")),
        "nchan = 0": dict(nchan=0),
        "wid = 0": dict(sizes=[(0, 40)] + SIZES[1:]), "hgt < 0": dict(sizes=SIZES[:4] + [(7, -1)] + SIZES[5:]),
        "rnx = 0": dict(sizes=SIZES[:4] + [(1, 33)] + SIZES[5:], sf=0.5),
        "hgt * wid >= 2^31": dict(sizes=SIZES[:4] + [(65536, 32768)] + SIZES[5:]),
        "image number = nimg": dict(pairs=PAIRS[:3] + [(0, 6)] + PAIRS[4:]),
        "image number < 0": dict(pairs=PAIRS[:3] + [(-1, 1)] + PAIRS[4:]),
        "bad image number in a pair that is not used": dict(pairs=PAIRS[:2] + [(0, 9)] + PAIRS[3:]),
        "unequal sizes": dict(pairs=PAIRS[:3] + [(0, 2)] + PAIRS[4:]),
        "unequal sizes, same pixel count": dict(sizes=[(50, 40), (40, 50)], pairs=[(0, 1)], use=None),
        "row_hi beyond the frame": dict(box=with_box(0, (0, fr[0][0] + 1, 0, fr[0][1]))),
        "col_hi beyond the frame": dict(box=with_box(1, (0, fr[1][0], 0, fr[1][1] + 1))),
        "row_lo < 0": dict(box=with_box(0, (-1, 5, 0, 5))), "col_lo < 0": dict(box=with_box(0, (0, 5, -1, 5))),
        "row_lo > row_hi": dict(box=with_box(3, (6, 5, 0, 5))), "col_lo > col_hi": dict(box=with_box(3, (0, 5, 6, 5))),
        "nimg < 0": dict(nimg=-1), "npairs < 0": dict(npairs=-1), "items_cap < 0": dict(items_cap=-1),
        "null sizes": dict(null_sizes=True), "null pairs": dict(null_pairs=True),
        "null out": dict(out=False), "null out_off": dict(off=False),
    }
    for name, kw in bad.items():
        st, o, oo, it = call(**kw)
        assert st == SPV_ERR_INVALID, name
        assert o == [-7] * 3 and (oo == -7).all() and (it == -7).all(), name + ": outputs touched"
        assert clib.spv_last_error(), name


def test_front_ends_check_their_counts():
    from spectavi_amd import device, mvg
    with pytest.raises(ValueError):
        device.rectify_batch_plan(SIZES, PAIRS, use=[1, 0])
    with pytest.raises(ValueError):
        device.rectify_batch_plan(SIZES, PAIRS, box=[(0, 1, 0, 1)])
    with pytest.raises(ValueError):
        mvg.image_pair_rectification_batch([np.zeros((4, 5))] * 2, [(0, 1)], [None, None])
    with pytest.raises(TypeError):
        mvg.image_pair_rectification_batch([np.zeros((4, 5)), np.zeros((5, 4))], [(0, 1)], [np.zeros((3, 4))])
    with pytest.raises(TypeError):
        mvg.image_pair_rectification_batch([np.zeros((4, 5))] * 2, [(0, 1)], [np.zeros((3, 3))])
    # a collection without a used pair touches no device: it runs without one
    assert mvg.image_pair_rectification_batch([np.zeros((4, 5))] * 2, [(0, 1), (1, 0)], [None, None]) == [None, None]
    assert mvg.image_pair_rectification_batch([], [], []) == []
