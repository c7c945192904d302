"""GPU: every device entry point that takes a workspace stays inside the size its query reports.

Each call runs three times: with a roomy workspace, with exactly the reported size, and with one byte less.  The
buffers are filled with 0xA5 and carry 4096 bytes beyond what is passed as ws_bytes.  With the reported size the
outputs equal the roomy run's bit for bit and the 4096 bytes stay untouched.  With one byte less the call returns
SPV_ERR_INVALID and has launched nothing (the whole buffer is untouched) -- or, for normalize and the hypothesis
scorer, whose workspace only buys a faster form, gives the same outputs again.  The shapes are the smallest at
which every piece of a layout is non-empty."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TAIL = 4096
FILL = 0xA5


class FixedWs:
    """Stands in for device.Workspace: always the first `nbytes` bytes of one buffer of nbytes + TAIL."""

    def __init__(self, nbytes):
        import torch
        self.nbytes = int(nbytes)
        self.buf = torch.full((self.nbytes + TAIL,), FILL, dtype=torch.uint8, device="cuda")

    def get(self, nbytes, device):
        return self.buf[:self.nbytes]

    def untouched(self, start):
        return bool((self.buf[start:] == FILL).all())


def check_bounds(reported, call, short_is_error=True):
    """call(workspace) -> the output tensors, every element of which the call writes."""
    import torch
    from spectavi_amd._lib import SPV_ERR_INVALID, SpectaviError

    def run(ws):
        outs = call(ws)
        torch.cuda.synchronize()
        return [t.cpu().numpy().tobytes() for t in outs]

    reported = int(reported)
    assert reported > 0
    want = run(FixedWs(reported + (1 << 20)))
    exact = FixedWs(reported)
    assert run(exact) == want, "outputs differ between a roomy workspace and one of the reported size"
    assert exact.untouched(reported), "the run wrote past the size its query reports"
    assert not exact.untouched(0), "the run never wrote to its workspace: this case checks nothing"
    short = FixedWs(reported - 1)
    if short_is_error:
        with pytest.raises(SpectaviError) as e:
            call(short)
        torch.cuda.synchronize()
        assert e.value.status == SPV_ERR_INVALID
        assert short.untouched(0), "a refused call has launched something"
    else:
        assert run(short) == want, "outputs differ in the form that needs no workspace"
        assert short.untouched(reported - 1)


def u8(seed, rows, dim):
    import torch
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (rows, dim), dtype=np.uint8)).cuda()


def f32(seed, rows, dim):
    import torch
    rng = np.random.default_rng(seed)
    return torch.from_numpy((rng.integers(0, 256, (rows, dim)) - 128).astype(np.float32)).cuda()


# 48: a tile width of its own; 176: padded copies of both sides (to 192); 128 with >= 32 database rows: the bound
# path's scratch is part of the layout, unused here
@pytest.mark.parametrize("xrows,yrows,dim", [(100, 70, 48), (100, 70, 176), (96, 300, 128)])
def test_l1k2(xrows, yrows, dim):
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    x, y = u8(1, xrows, dim), u8(2, yrows, dim)
    check_bounds(clib.spv_l1k2_workspace_bytes(xrows, yrows, dim), lambda ws: device.l1k2(x, y, workspace=ws))


def test_l1k2_bound_path():
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    x, y = u8(3, 96, 128), u8(4, 300, 128)
    before = device.l1k2_get_prune()
    device.l1k2_set_prune(1)

    def call(ws):
        out = device.l1k2(x, y, workspace=ws)
        assert device.l1k2_prune_stats()[0] > 0   # the bound path ran
        return out

    try:
        check_bounds(clib.spv_l1k2_workspace_bytes(96, 300, 128), call)
    finally:
        device.l1k2_set_prune(before)


def test_bruteforce():
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    x, y = f32(5, 300, 17), f32(6, 70, 17)
    check_bounds(clib.spv_bruteforce_workspace_bytes(300, 70, 17, 5),
                 lambda ws: device.bruteforce(x, y, k=5, p=2.0, workspace=ws))


def test_ann_l2():
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    x, y = f32(7, 700, 40), f32(8, 70, 40)
    check_bounds(clib.spv_ann_l2_workspace_bytes(700, 70, 40, 4, 0), lambda ws: device.ann_l2(x, y, k=4, workspace=ws))


@pytest.mark.parametrize("m,n,g", [(8, 2, 2), (24, 1, 2)])   # the group probe with its carried keys; the wave probe
def test_cascade(m, n, g):
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    x, y = f32(9, 2000, 128), f32(10, 700, 128)
    d = torch.from_numpy(np.random.default_rng(11).standard_normal((n, 128, m)).astype(np.float32)).cuda()
    check_bounds(clib.spv_cascade_workspace_bytes(2000, 700, 128, m, n, g),
                 lambda ws: device.cascade(x, y, d, g=g, workspace=ws, want_ncand=True))


@pytest.mark.parametrize("m,n,g", [(8, 2, 2), (24, 1, 2)])   # bucket bits = m: buckets copied; below m: filtered
def test_cascade_batch(m, n, g):
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    from tests import cascade_batch_cases as cb
    rows = [0, 70, 300, 33]   # the first set empty; more than one work item; less than one
    x, seg, d = cb.collection(rows, 128, m, n, g)
    prs = np.array(cb.BOOK, np.int32)
    dx, dd = torch.from_numpy(x).cuda(), torch.from_numpy(d).cuda()
    assert device.cascade_batch_plan(seg, cb.BOOK, 128, m, n, g)["hb"] == min(m, 12)

    def call(ws):
        idx, dist, _, ncand = device.cascade_batch(dx, seg, cb.BOOK, dd, g=g, workspace=ws, want_ncand=True)
        return [idx, dist, ncand]

    need = clib.spv_cascade_batch_workspace_bytes(seg.ctypes.data, len(rows), 128, m, n, g, prs.ctypes.data, len(prs))
    check_bounds(need, call)
    # order, ranks and the segment sums are not zeroed by the call: on a workspace of 0xA5 bytes it still is the oracle
    from tests.test_cascade_batch_gpu import assert_pairs_equal, oracle_pairs
    idx, dist, ncand = (t.cpu().numpy() for t in call(FixedWs(need)))
    out_off = np.concatenate([[0], np.cumsum([rows[a] for a, _ in cb.BOOK])])
    assert_pairs_equal((idx.view(np.uint64), dist, ncand, out_off), oracle_pairs(x, seg, d, cb.BOOK, g), seg, cb.BOOK, "0xA5")


def test_sift():
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    wid, hgt = 96, 64
    im = torch.from_numpy(np.random.default_rng(12).random((hgt, wid), dtype=np.float32)).cuda()

    def call(ws):
        table = torch.zeros((4096, 132), dtype=torch.float32, device="cuda")
        count = torch.zeros(1, dtype=torch.int32, device="cuda")
        device.sift_into(im, table, count, workspace=ws)
        return [count, table]

    assert 0 < int(call(None)[0].item()) <= 4096   # some keypoints, and all of them in the table
    check_bounds(clib.spv_sift_workspace_bytes(wid, hgt), call)


def test_ratio_test():
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    rng = np.random.default_rng(13)
    idx = torch.from_numpy(rng.integers(0, 100000, (5000, 2), dtype=np.int64)).cuda()
    dist = torch.from_numpy(np.sort(rng.integers(1, 1000, (5000, 2)).astype(np.int32), axis=1)).cuda()

    def call(ws):
        matches, count = device.ratio_test(idx, dist, 1.5, workspace=ws)
        n = int(count.item())
        assert 0 < n < 5000
        return [count, matches[:n].contiguous()]

    check_bounds(clib.spv_ratio_test_workspace_bytes(5000), call)


def ransac_inputs():
    import torch
    from tests.test_ransac_gpu import _candidates, _scene
    rng = np.random.default_rng(14)
    x0, x1, E_true, P1 = _scene(rng, npt=200)
    Fs = _candidates(rng, E_true, 30)
    return torch.from_numpy(Fs).cuda(), torch.from_numpy(x0).cuda(), torch.from_numpy(x1).cuda(), P1


@pytest.mark.parametrize("want_mask", [False, True])
def test_ransac_process_candidates(want_mask):
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    Fs, x0, x1, _ = ransac_inputs()

    def call(ws):
        out = device.ransac_process_candidates(Fs, x0, x1, required_percent_inliers=.5, reprojection_error_allowed=1e-2,
                                               want_mask=want_mask, workspace=ws)
        return [out[k] for k in sorted(out)]

    check_bounds(clib.spv_ransac_workspace_bytes(30, 200, int(want_mask)), call)


def test_normalize():
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    rows, dim = 65536, 20   # the fewest rows whose column sums are folded
    x = torch.from_numpy(np.random.default_rng(15).random((rows, dim), dtype=np.float32) * 255).cuda()
    full, walking = clib.spv_normalize_workspace_bytes_rows(rows, dim), clib.spv_normalize_workspace_bytes(dim)
    assert full > walking

    def call(ws):
        return device.normalize(x, want_float=True, want_ubyte=True, workspace=ws)

    check_bounds(full, call, short_is_error=False)   # one byte less: the walking form
    check_bounds(walking, call)


def test_dlt_score_hypotheses():
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib
    _, x0, x1, P1 = ransac_inputs()
    rng = np.random.default_rng(16)
    P1s = torch.from_numpy(P1[None] + 10.0 ** rng.uniform(-6, -1, (120, 1, 1)) * rng.standard_normal((120, 3, 4))).cuda()
    P0 = np.hstack([np.eye(3), np.zeros((3, 1))])
    check_bounds(clib.spv_dlt_score_workspace_bytes(120, 200),
                 lambda ws: device.dlt_score_hypotheses(P0, P1s, x0, x1, 1e-2, want_mask=True, workspace=ws),
                 short_is_error=False)   # one byte less: a shorter work list, down to the one-pass form
