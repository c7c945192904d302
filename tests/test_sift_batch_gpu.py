"""sift_batch on the GPU: many images in one chain of launches.

The yardstick is spv_sift_device run on each image alone (device.sift), itself pinned to vlfeat's table by
tests/test_sift_gpu.py: for every image the batch's rows and count are the same bits, whatever else the batch holds,
wherever the image stands and however the call is cut into groups.  The largest image is 233 x 310."""
import numpy as np
import pytest

from tests import sift_cases as sc
from tests.sift_cases import assert_tables_match

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def _ragged():
    """Octave counts 1, 2, 3 and 5 side by side, images that sit out from octave -1 on, block and wave seams."""
    ims = [("min-side-15x21", sc.smooth_random(201, 15, 21)), ("min-side-16x21", sc.smooth_random(202, 16, 21)),
           ("min-side-45x32", sc.smooth_random(203, 45, 32)), ("min-side-45x33", sc.smooth_random(204, 45, 33)),
           ("seam-40x64", sc.smooth_random(205, 40, 64)), ("seam-40x257", sc.smooth_random(206, 40, 257)),
           ("no-interior-1x40", sc.smooth_random(207, 1, 40)),
           ("constant-20x20", np.full((20, 20), 42, np.float32)),
           ("seam-127x129", sc.smooth_random(208, 127, 129)), ("no-interior-2x3", sc.smooth_random(209, 2, 3)),
           ("blobs", sc.blobs()), ("checkerboard", sc.checkerboard()), ("sur_ogre", sc.sur_ogre()[0])]
    return [n for n, _ in ims], [np.ascontiguousarray(im, np.float32) for _, im in ims]


@pytest.fixture(scope="module")
def dev():
    from spectavi_amd import device
    return device


def _single(dev, im):
    import torch
    return dev.sift(torch.from_numpy(im).cuda()).cpu().numpy()


@pytest.fixture(scope="module")
def ragged(dev):
    """(names, images, the single-image tables): computed once, never changed."""
    names, ims = _ragged()
    want = [_single(dev, im) for im in ims]
    for t in want:
        t.setflags(write=False)
    by_name = dict(zip(names, want))
    assert len(by_name["constant-20x20"]) == len(by_name["no-interior-1x40"]) == len(by_name["no-interior-2x3"]) == 0
    assert sum(len(t) > 0 for t in want) == len(want) - 3
    from tests import sift_oracle as so
    assert {1, 2, 3, 5} <= {so.noctaves(im.shape[1], im.shape[0]) for im in ims}
    return names, ims, want


def _sizes(ims):
    return np.array([(im.shape[1], im.shape[0]) for im in ims], np.int32).reshape(-1, 2)


def _run(dev, ims, caps, ws_bytes=None):
    """One spv_sift_batch_device call into a table pre-filled with the sentinel: (table, counts, cap_off)."""
    import torch
    flat = torch.from_numpy(np.concatenate([im.reshape(-1) for im in ims]) if ims else np.zeros(0, np.float32)).cuda()
    cap_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    table = torch.full((int(cap_off[-1]), 132), SENTINEL, dtype=torch.float32, device="cuda")
    counts = torch.full((len(ims),), -1, dtype=torch.int32, device="cuda")
    ws = None if ws_bytes is None else torch.empty(int(ws_bytes), dtype=torch.uint8, device="cuda")
    dev.sift_batch_into(flat, _sizes(ims), table, cap_off, counts, ws)
    return table.cpu().numpy(), counts.cpu().numpy(), cap_off


def _assert_regions(table, counts, cap_off, want, names, what):
    """Every region holds its image's rows, bit for bit, and the sentinel behind them."""
    assert counts.tolist() == [len(t) for t in want], what
    for i, t in enumerate(want):
        region = table[cap_off[i]:cap_off[i + 1]]
        n = min(len(t), len(region))
        assert_tables_match(region[:n], t[:n], "%s: %s" % (what, names[i]), ulp=0)
        assert (region[n:] == SENTINEL).all(), "%s: %s: rows behind the result were touched" % (what, names[i])


def _caps(want, slack=3):
    return [len(t) + slack for t in want]


def test_ragged_batch_matches_every_image_alone(dev, ragged):
    names, ims, want = ragged
    table, counts, cap_off = _run(dev, ims, _caps(want))
    _assert_regions(table, counts, cap_off, want, names, "ragged")


def test_order_does_not_move_results(dev, ragged):
    names, ims, want = ragged
    table, counts, cap_off = _run(dev, ims[::-1], _caps(want[::-1]))
    _assert_regions(table, counts, cap_off, want[::-1], names[::-1], "reversed")


def test_neighbours_do_not_move_results(dev, ragged):
    names, ims, want = ragged
    castle = sc.castle("01")
    ogre, ogre_want = ims[names.index("sur_ogre")], want[names.index("sur_ogre")]
    castle_want = _single(dev, castle)
    trio, trio_want = [castle, ogre, castle], [castle_want, ogre_want, castle_want]
    table, counts, cap_off = _run(dev, trio, _caps(trio_want))
    _assert_regions(table, counts, cap_off, trio_want, ["castle-01", "sur_ogre", "castle-01"], "between castles")


def test_identical_images_give_identical_regions_and_vlfeats_table(dev, ragged):
    names, ims, want = ragged
    ogre, golden = sc.sur_ogre()
    table, counts, cap_off = _run(dev, [ogre] * 8, [len(golden)] * 8)
    assert counts.tolist() == [1168] * 8
    first = table[:1168]
    assert_tables_match(first, want[names.index("sur_ogre")], "sur_ogre x 8 against the image alone", ulp=0)
    for i in range(1, 8):
        assert table[cap_off[i]:cap_off[i + 1]].tobytes() == first.tobytes(), i
    # vlfeat's recorded table, at the bar tests/test_sift_gpu.py holds the single-image path to
    print("frame ulp distance to vlfeat's table: max %d" % sc.ulp_diff(first[:, :4], golden[:, :4]).max())
    assert np.allclose(first[:, :4], golden[:, :4])
    assert np.array_equal(first[:, 4:], golden[:, 4:])


def test_groups_do_not_move_results(dev, ragged):
    names, ims, want = ragged
    # sur_ogre needs more than all the others together: in the middle, the least workspace cuts before and behind it
    order = list(range(len(ims) - 1))
    order.insert(6, len(ims) - 1)
    names, ims, want = [names[i] for i in order], [ims[i] for i in order], [want[i] for i in order]
    plan = dev.sift_batch_plan(_sizes(ims))
    lo, hi = plan["min_workspace_bytes"], plan["workspace_bytes"]
    assert dev.sift_batch_plan(_sizes(ims), lo)["groups"] > 2
    # the smallest workspace that gives exactly two groups (the group count never grows with the workspace)
    a, b = lo, hi
    while a < b:
        mid = (a + b) // 2
        if dev.sift_batch_plan(_sizes(ims), mid)["groups"] <= 2:
            b = mid
        else:
            a = mid + 1
    assert dev.sift_batch_plan(_sizes(ims), a)["groups"] == 2
    for ws_bytes, what in ((lo, "many groups"), (a, "two groups"), (hi, "one group")):
        table, counts, cap_off = _run(dev, ims, _caps(want), ws_bytes)
        _assert_regions(table, counts, cap_off, want, names, what)


def test_capacity_and_overflow(dev, ragged):
    names, ims, want = ragged
    caps = _caps(want)
    zero, short = names.index("blobs"), names.index("seam-127x129")
    assert len(want[zero]) > 0 and len(want[short]) > 10
    caps[zero] = 0
    caps[short] = len(want[short]) - 10
    table, counts, cap_off = _run(dev, ims, caps)
    # the true counts, the rows that fit, the sentinel behind them; every other image complete
    _assert_regions(table, counts, cap_off, want, names, "short regions")
    assert counts[zero] == len(want[zero]) > caps[zero] and counts[short] == len(want[short]) > caps[short]


def test_empty_and_single(dev, ragged):
    import torch
    from spectavi_amd._lib import clib
    names, ims, want = ragged
    cap0 = np.zeros(1, np.int64)
    table = torch.full((4, 132), SENTINEL, dtype=torch.float32, device="cuda")
    counts = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    assert clib.spv_sift_batch_device(None, None, 0, ws.data_ptr(), 256, table.data_ptr(), cap0.ctypes.data,
                                      counts.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (table.cpu().numpy() == SENTINEL).all() and (counts.cpu().numpy() == -1).all()
    i = names.index("seam-40x257")
    table, counts, cap_off = _run(dev, [ims[i]], _caps([want[i]]))
    _assert_regions(table, counts, cap_off, [want[i]], [names[i]], "one image")


def test_pack(dev, ragged):
    import torch
    from spectavi_amd._lib import clib
    names, ims, want = ragged
    caps = _caps(want, slack=5)
    table, counts, cap_off = _run(dev, ims, caps)
    seg_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    d_table = torch.from_numpy(table).cuda()
    packed, geom, desc = dev.sift_batch_pack(d_table, cap_off, seg_off, want_packed=True, want_split=True)
    for i, t in enumerate(want):
        got = packed[seg_off[i]:seg_off[i + 1]].cpu().numpy()
        assert got.tobytes() == table[cap_off[i]:cap_off[i] + len(t)].tobytes() == t.tobytes(), names[i]
    assert [int(seg_off[i + 1] - seg_off[i]) for i in range(len(want)) if len(want[i]) == 0] == [0, 0, 0]
    g, d = dev.split_sift_table(packed)
    assert torch.equal(geom, g) and torch.equal(desc, d)
    # the split alone gives the same
    g2, d2 = dev.sift_batch_pack(d_table, cap_off, seg_off, want_packed=False, want_split=True)
    assert torch.equal(g2, g) and torch.equal(d2, d)
    # a segment longer than its capacity: SPV_ERR_INVALID, outputs untouched
    bad = seg_off.copy()
    k = names.index("blobs")
    bad[k + 1:] += caps[k] + 1 - (seg_off[k + 1] - seg_off[k])
    out = torch.full((int(bad[-1]), 132), SENTINEL, dtype=torch.float32, device="cuda")
    geo = torch.full((int(bad[-1]), 4), SENTINEL, dtype=torch.float32, device="cuda")
    des = torch.full((int(bad[-1]), 128), 77, dtype=torch.uint8, device="cuda")
    assert clib.spv_sift_batch_pack_device(d_table.data_ptr(), cap_off.ctypes.data, bad.ctypes.data, len(ims),
                                           out.data_ptr(), geo.data_ptr(), des.data_ptr(), None) == 1
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (geo == SENTINEL).all() and (des == 77).all()


def test_front_ends(dev, ragged):
    import torch
    from spectavi_amd._lib import SPV_ERR_OVERFLOW, SPV_OK, clib
    names, ims, want = ragged
    tensors = [torch.from_numpy(im).cuda() for im in ims]
    total = np.concatenate(want)
    seg = np.concatenate([[0], np.cumsum([len(t) for t in want])]).astype(np.int64)
    # a deliberately short capacity: the short images run again with exact capacities, the same bits
    table, seg_off = dev.sift_batch(tensors, capacity=8)
    assert seg_off.dtype == np.int64 and np.array_equal(seg_off, seg)
    assert table.cpu().numpy().tobytes() == total.tobytes()
    # the default capacity, and a capped workspace
    table, seg_off = dev.sift_batch(tensors)
    assert np.array_equal(seg_off, seg) and table.cpu().numpy().tobytes() == total.tobytes()
    lo = dev.sift_batch_plan(_sizes(ims))["min_workspace_bytes"]
    geom, desc, seg_off = dev.sift_batch(tensors, capacity=8, max_workspace_bytes=lo, want_split=True)
    g, d = dev.split_sift_table(torch.from_numpy(total).cuda())
    assert np.array_equal(seg_off, seg) and torch.equal(geom, g) and torch.equal(desc, d)
    # the host-pointer form
    flat = np.concatenate([im.reshape(-1) for im in ims])
    sizes = _sizes(ims)
    for slack, status in ((0, SPV_OK), (-10, SPV_ERR_OVERFLOW)):
        caps = [len(t) for t in want]
        k = names.index("checkerboard")
        caps[k] += slack
        cap_off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
        out = np.full((int(cap_off[-1]), 132), SENTINEL, np.float32)
        counts = np.full(len(ims), -1, np.int32)
        assert clib.spv_sift_tables(flat.ctypes.data, sizes.ctypes.data, len(ims), out.ctypes.data, cap_off.ctypes.data,
                                    counts.ctypes.data) == status
        _assert_regions(out, counts, cap_off, want, names, "spv_sift_tables, slack %d" % slack)


def test_hand_over_to_l1k2_batch(dev):
    """Shape and hand-over only: what sift_batch(want_split=True) returns is what l1k2_batch takes."""
    import torch
    tex = sc.smooth_random(310, 120, 160)
    crops = [torch.from_numpy(np.ascontiguousarray(tex[:96, :128])).cuda(),
             torch.from_numpy(np.ascontiguousarray(tex[10:106, 20:148])).cuda()]
    geom, desc, seg_off = dev.sift_batch(crops, want_split=True)
    assert geom.shape == (seg_off[-1], 4) and desc.shape == (seg_off[-1], 128) and (np.diff(seg_off) > 0).all()
    idx, dist, out_off = dev.l1k2_batch(desc, seg_off, [(0, 1), (1, 0)])
    for p, (q, db) in enumerate([(0, 1), (1, 0)]):
        t_q, t_db = desc[seg_off[q]:seg_off[q + 1]], desc[seg_off[db]:seg_off[db + 1]]
        i1, d1 = dev.l1k2(t_db.contiguous(), t_q.contiguous())
        assert torch.equal(idx[out_off[p]:out_off[p + 1]], i1) and torch.equal(dist[out_off[p]:out_off[p + 1]], d1)
