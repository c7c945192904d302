"""tracks_batch on the GPU against tests/tracks_model.py: every output of every case must equal the model's exactly.

Internal lengths of the implementation (spectavi_amd/csrc/tracks_batch.hip).  The ordering phase has ONE path for
every track length, a stable radix sort of (track, row) by track number, so there is no short-track / long-track
threshold; what it does have are block sizes, and the number of its passes depends on the track count:
    64      keys the scatter of a pass takes in one step (one wave)
    256     lanes of the element-wise kernels
    1024    keys per workgroup of a pass; rows per workgroup of the three row scans
    256, 65536   track counts from which a second and a third 8-bit pass run
`test_length_thresholds` puts tracks of T - 1, T and T + 1 members for T = 64, 256 and 1024 in one call, their rows
interleaved; `test_pass_counts` runs 1, 2 and 3 passes."""
import ctypes as ct
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import tracks_cases as tc
from tests import tracks_model as tm

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("label", "track", "track_off", "members", "flags")
INSTANTIATED = {
    "tracks_init_kernel", "tracks_hook_kernel", "tracks_flatten_kernel", "tracks_sizes_kernel",
    "tracks_block_sums_kernel", "tracks_scan_kernel", "tracks_number_kernel", "tracks_place_kernel",
    "tracks_order_count_kernel", "tracks_order_scan_kernel", "tracks_order_scatter_kernel", "tracks_finish_kernel",
}
PROFILE_NAMES = ("tracks_init", "tracks_hook", "tracks_flatten", "tracks_sizes", "tracks_scan", "tracks_place",
                 "tracks_order", "tracks_flags")


def run(seg, pairs, matches, count=None, mask=None, min_len=2, label=None, capacity=None):
    """device.tracks_batch on host arrays -> the five outputs as numpy arrays, in the model's order."""
    import torch
    from spectavi_amd import device
    m = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
    if capacity is not None:
        m = np.concatenate([m, np.full((max(0, capacity - len(m)), 2), 123456789, np.int32)])[:capacity]
    cnt = len(matches) if count is None else count
    tm_ = torch.from_numpy(m.copy()).cuda()
    tk = None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda()
    tl = None if label is None else torch.from_numpy(np.ascontiguousarray(label, np.int32)).cuda()
    track_off, members, flags, lab, track = device.tracks_batch(seg, pairs, tm_, torch.tensor([cnt], dtype=torch.int32).cuda(),
                                                                mask=tk, min_len=min_len, label=tl)
    if tl is not None:
        assert lab.data_ptr() == tl.data_ptr(), "a label passed in is updated in place"
    return lab.cpu().numpy(), track.cpu().numpy(), track_off, members.cpu().numpy(), flags.cpu().numpy()


def assert_same(got, want, what, names=NAMES):
    assert len(got) == len(want) == len(names)
    for name, g, w in zip(names, got, want):
        assert g.dtype == w.dtype, (what, name, g.dtype, w.dtype)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        assert np.array_equal(g, w), (what, name, np.flatnonzero((g != w).reshape(len(g), -1).any(1))[:8])


@pytest.fixture(scope="module")
def ragged():
    """The ragged collection, its model results for min_len 2 and 3, and a random mask with its results."""
    seg, pairs, m = tc.ragged()
    mask = (np.random.default_rng(3).random(len(m)) < 0.6).astype(np.uint8)
    want = {ml: tm.tracks(seg, tm.edges_of(seg, pairs, m), ml) for ml in (2, 3)}
    want["mask"] = tm.tracks(seg, tm.edges_of(seg, pairs, m, mask=mask), 2)
    return seg, pairs, m, mask, want


def test_ragged_collection(ragged):
    seg, pairs, m, mask, want = ragged
    label, track, track_off, members, flags = want[2]
    length = np.diff(track_off)
    assert 0 < flags.sum() < len(flags), "consistent and inconsistent tracks"
    assert (length == 2).any() and (length == 3).any() and (length >= 5).any() and length.max() > 256
    assert len(want[3][4]) < len(flags) and 0 < len(want["mask"][4]) and not np.array_equal(want["mask"][0], label)
    assert_same(run(seg, pairs, m), want[2], "min_len 2")
    assert_same(run(seg, pairs, m, min_len=3), want[3], "min_len 3")
    assert_same(run(seg, pairs, m, mask=mask), want["mask"], "masked")


def test_edge_order_and_repetition(ragged):
    seg, pairs, m, _, want = ragged
    rng = np.random.default_rng(0)
    assert_same(run(seg, pairs, m[::-1]), want[2], "reversed")
    assert_same(run(seg, pairs, m[rng.permutation(len(m))]), want[2], "shuffled")
    assert_same(run(seg, pairs, np.concatenate([m, m[::2], m])), want[2], "edges repeated")
    for rep in range(5):
        assert_same(run(seg, pairs, m), want[2], "run %d" % rep)


def test_depth():
    seg, pairs, m = tc.depth()
    want = tm.tracks(seg, tm.edges_of(seg, pairs, m))
    assert np.diff(want[2]).tolist() == [20000] and want[4].tolist() == [1] and not want[0].any()
    assert np.array_equal(want[3], np.stack([np.repeat(np.arange(40), 500), np.tile(np.arange(500), 40)], 1))
    for what, order in (("ascending", np.argsort(m[:, 0], kind="stable")), ("descending", np.argsort(-m[:, 0], kind="stable")),
                        ("shuffled", np.random.default_rng(1).permutation(len(m)))):
        assert_same(run(seg, pairs, m[order]), want, what)


@pytest.mark.parametrize("centre_last", [False, True])
def test_contention(centre_last):
    seg, pairs, m = tc.star(centre_last)
    want = tm.tracks(seg, tm.edges_of(seg, pairs, m))
    assert np.diff(want[2]).tolist() == [4097] and not want[0].any()
    assert_same(run(seg, pairs, m), want, "star")


def test_length_thresholds():
    lengths = [63, 64, 65, 255, 256, 257, 1023, 1024, 1025]
    seg, pairs, m = tc.chains(lengths)
    want = tm.tracks(seg, tm.edges_of(seg, pairs, m))
    assert np.diff(want[2]).tolist() == lengths
    assert_same(run(seg, pairs, m), want, "one set")
    # the same rows cut into sets at block edges and off them: consistent and inconsistent tracks of every length
    total = sum(lengths)
    seg, pairs, m = tc.chains(lengths, [5, 1019, 1, 1024, total - 2049])
    want = tm.tracks(seg, tm.edges_of(seg, pairs, m))
    assert np.diff(want[2]).tolist() == lengths
    assert_same(run(seg, pairs, m), want, "five sets")
    assert_same(run(seg, pairs, m, min_len=256), tm.tracks(seg, tm.edges_of(seg, pairs, m), 256), "min_len 256")


@pytest.mark.parametrize("ntracks", [255, 256, 257, 65535, 65537])
def test_pass_counts(ntracks):
    """Track counts either side of where the ordering takes another 8-bit pass; tracks of 2 and 3 members whose rows
    interleave, in two sets."""
    lengths = [2 + (j % 7 == 0) for j in range(ntracks)]
    total = sum(lengths)
    seg, pairs, m = tc.chains(lengths, [ntracks + 1, total - ntracks - 1])
    want = tm.tracks(seg, tm.edges_of(seg, pairs, m))
    assert len(want[4]) == ntracks
    assert_same(run(seg, pairs, m), want, ntracks)


def test_continuing(ragged):
    seg, pairs, m, _, want = ragged
    h = len(m) // 2
    first = run(seg, pairs, m[:h])
    assert_same(first, tm.tracks(seg, tm.edges_of(seg, pairs, m[:h])), "first half")
    assert_same(run(seg, pairs, m[h:], label=first[0]), want[2], "second half on the first half's label")
    assert_same(run(seg, pairs, m[:0], label=want[2][0], capacity=0), want[2], "no new edge: the label alone")
    # a second pass with another pairs list: the same edges as rows of the reversed list, and new ones
    rev = pairs[::-1].copy()
    e = tm.edges_of(seg, pairs, m)
    off = tm.out_offsets(seg, rev)
    m2 = np.array([[off[p], 0] for p in range(len(rev)) if seg[rev[p, 0] + 1] > seg[rev[p, 0]] and seg[rev[p, 1] + 1] > seg[rev[p, 1]]],
                  np.int32)
    e2 = tm.edges_of(seg, rev, m2)
    assert len(e2) > 20
    assert_same(run(seg, rev, m2, label=first[0]), tm.tracks(seg, np.concatenate([e[:h], e2])), "other pairs")


def test_garbage_label(ragged):
    """-5, 2^31 - 1 and row + 1 in the incoming label stand for the row itself: the call returns, and every output
    index lies inside its array."""
    seg, pairs, m, _, want = ragged
    n = int(seg[-1])
    lab = np.arange(n, dtype=np.int64)
    rng = np.random.default_rng(4)
    lab[rng.choice(n, 300, replace=False)] = -5
    lab[rng.choice(n, 300, replace=False)] = 2 ** 31 - 1
    up = rng.choice(n - 1, 300, replace=False)
    lab[up] = up + 1
    got = run(seg, pairs, m, label=lab.astype(np.int32))
    assert_same(got, want[2], "entries out of range are the row itself")
    # a label that is in range but no earlier result: nothing to compare, but everything must stay in bounds
    junk = (rng.random(n) * (np.arange(n) + 1)).astype(np.int32)
    label, track, track_off, members, flags = run(seg, pairs, m, label=junk)
    nt = len(track_off) - 1
    assert label.min() >= 0 and np.all(label <= np.arange(n)) and track.min() >= -1 and track.max() == nt - 1
    assert track_off[0] == 0 and np.all(np.diff(track_off) >= 2) and track_off[-1] == len(members) <= n
    assert members[:, 0].min() >= 0 and members[:, 0].max() < len(seg) - 1 and members[:, 1].min() >= 0
    assert np.all(members[:, 1] < np.diff(seg)[members[:, 0]]) and flags.max() <= 1
    assert_same((label, track, track_off, members, flags), tm.tracks(seg, tm.edges_of(seg, pairs, m), label=junk), "junk")


def test_malformed_and_empty(ragged):
    seg, pairs, m, _, want = ragged
    out_rows = int(tm.out_offsets(seg, pairs)[-1])
    p = len(pairs) - 1                                            # (5, 3): out rows end at out_rows, database set of 255
    bad = np.array([[-1, 0], [out_rows, 0], [out_rows - 1, -1], [out_rows - 1, 255], [-2 ** 31, 5], [2 ** 31 - 1, 5],
                    [0, 2 ** 31 - 1], [0, 1]], np.int32)         # out row 0 is pair (1, 0): its database set is empty
    mixed = np.concatenate([bad, m[:100], bad, m[100:], bad])
    assert len(tm.edges_of(seg, pairs, mixed)) == len(m) and pairs[p].tolist() == [5, 3]
    assert_same(run(seg, pairs, mixed), want[2], "rows out of range are skipped")
    h = 300
    assert_same(run(seg, pairs, m[:h], count=len(m) + 7), tm.tracks(seg, tm.edges_of(seg, pairs, m[:h])), "count > capacity")
    assert_same(run(seg, pairs, m, count=h), tm.tracks(seg, tm.edges_of(seg, pairs, m, count=h)), "count < capacity")
    n = int(seg[-1])
    empty = (np.arange(n, dtype=np.int32), np.full(n, -1, np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32),
             np.zeros(0, np.uint8))
    assert_same(run(seg, pairs, m, count=0), empty, "count 0")
    assert_same(run(seg, pairs, m, count=-3), empty, "negative count")
    assert_same(run(seg, pairs, m[:0]), empty, "capacity 0")
    assert_same(run(seg, np.zeros((0, 2), np.int32), m), empty, "no pairs")
    assert_same(run(seg, pairs, m, mask=np.zeros(len(m), np.uint8)), empty, "all-zero mask")
    none = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64), np.zeros((0, 2), np.int32), np.zeros(0, np.uint8))
    assert_same(run([0, 0, 0], [[1, 0]], m[:5]), none, "no rows")
    assert_same(run([0], np.zeros((0, 2), np.int32), m[:5]), none, "no sets")


def test_guards(ragged):
    """64 sentinel elements either side of every output and of the workspace stay untouched, through the raw call;
    the outputs are the capacities of the header, B = min(total_rows, 2 capacity)."""
    import torch
    from spectavi_amd._lib import clib, check
    seg, pairs, m, _, want = ragged
    n, cap = int(seg[-1]), len(m)
    B = min(n, 2 * cap)
    assert B == 2 * cap < n
    G = 64

    def guarded(count, dtype, fill):
        t = torch.full((count + 2 * G,) , fill, dtype=dtype, device="cuda")
        return t, t[G:G + count]
    ws_bytes = clib.spv_tracks_batch_workspace_bytes(n, cap)
    bufs = {"label": guarded(n, torch.int32, -77), "track": guarded(n, torch.int32, -77),
            "track_off": guarded(B // 2 + 1, torch.int64, -77), "members": guarded(2 * B, torch.int32, -77),
            "flags": guarded(B // 2, torch.uint8, 0xEE), "counts": guarded(2, torch.int32, -77),
            "ws": guarded(ws_bytes // 4, torch.int32, -77)}
    tmat = torch.from_numpy(m).cuda()
    cnt = torch.tensor([cap], dtype=torch.int32).cuda()
    segc, prs = np.ascontiguousarray(seg, np.int64), np.ascontiguousarray(pairs, np.int32)
    check(clib.spv_tracks_batch_device(segc.ctypes.data, len(segc) - 1, prs.ctypes.data, len(prs), tmat.data_ptr(), cnt.data_ptr(),
                                       cap, None, 2, 0, *[bufs[k][1].data_ptr() for k in ("label", "track", "track_off", "members",
                                                                                          "flags", "counts", "ws")],
                                       ws_bytes, ct.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    for name, (whole, inner) in bufs.items():
        fill = 0xEE if name == "flags" else -77
        assert bool((whole[:G] == fill).all()) and bool((whole[G + inner.numel():] == fill).all()), name
    nt, nm = bufs["counts"][1].tolist()
    got = (bufs["label"][1].cpu().numpy(), bufs["track"][1].cpu().numpy(), bufs["track_off"][1][:nt + 1].cpu().numpy(),
           bufs["members"][1][:2 * nm].cpu().numpy().reshape(-1, 2), bufs["flags"][1][:nt].cpu().numpy())
    assert_same(got, want[2], "raw call")
    # beyond the counts the track arrays keep what they held
    assert bool((bufs["track_off"][1][nt + 1:] == -77).all()) and bool((bufs["members"][1][2 * nm:] == -77).all())
    assert bool((bufs["flags"][1][nt:] == 0xEE).all())


def test_host_form(ragged):
    from spectavi_amd import feature
    seg, pairs, m, mask, want = ragged
    off = tm.out_offsets(seg, pairs)
    per, per_mask = [], []
    for p in range(len(pairs)):
        sel = (m[:, 0] >= off[p]) & (m[:, 0] < off[p + 1])
        per.append(m[sel] - np.array([off[p], 0], np.int32))
        per_mask.append(mask[sel])
    for kw, key in (({}, 2), ({"min_len": 3}, 3), ({"masks": per_mask}, "mask")):
        track_off, members, flags = feature.match_tracks_batch(np.diff(seg), pairs, per, **kw)
        assert_same((track_off, members, flags), want[key][2:], "host form %s" % key, NAMES[2:])
    assert_same(feature.match_tracks_batch(np.diff(seg), pairs, per), run(seg, pairs, m)[2:], "host and device form", NAMES[2:])
    # rows outside their tables are skipped (the pair is (5, 3): 257 query rows, 255 database rows); no matches at
    # all give no track
    per[-1] = np.concatenate([per[-1], [[-1, 0], [257, 0], [0, 255], [0, -1]]])
    assert_same(feature.match_tracks_batch(np.diff(seg), pairs, per), want[2][2:], "host form, rows out of range", NAMES[2:])
    got = feature.match_tracks_batch(np.diff(seg), pairs, [np.zeros((0, 2), np.int64)] * len(pairs))
    assert got[0].tolist() == [0] and got[1].shape == (0, 2) and got[2].shape == (0,)
    got = feature.match_tracks_batch([], [], [])
    assert got[0].tolist() == [0] and got[1].shape == (0, 2) and got[2].shape == (0,)


@pytest.mark.parametrize("guided", [None, 4.0])
def test_pipeline(guided):
    from examples.multiview_from_sift_tables import multiview_pipeline, synthetic_sift_views
    tables, K = synthetic_sift_views(seed=3, n_views=4, n_points=300)
    out = multiview_pipeline(tables, K, guided=guided, tracks=True)
    inp = out["track_inputs"]
    seg, pairs = inp["seg_off"], out["pairs"]
    edges = tm.edges_of(seg, pairs, inp["matches"].cpu().numpy(), int(inp["count"]), inp["mask"].cpu().numpy())
    assert len(edges) > 300
    if guided is not None:
        more = tm.edges_of(seg, pairs, inp["guided_matches"].cpu().numpy(), int(inp["guided_count"]))
        assert len(more) > 300
        edges = np.concatenate([edges, more])
    track_off, members, flags, label, track = out["tracks"]
    got = (label.cpu().numpy(), track.cpu().numpy(), track_off, members.cpu().numpy(), flags.cpu().numpy())
    assert_same(got, tm.tracks(seg, edges), "pipeline")
    assert np.diff(track_off).max() >= 4, "tracks through all four views"


def test_profile_names():
    """A call with edges and more than 256 possible tracks ticks every phase once; one without a possible edge has no
    hooking launch; one whose capacity allows a single track has no ordering launch."""
    import torch
    from spectavi_amd import device
    seg, pairs, m = tc.ragged()
    counts = {}
    device.profile_enable(True)
    try:
        for what, mm in (("edges", m), ("one edge", m[:1]), ("capacity 0", m[:0])):
            t = torch.from_numpy(mm.copy()).cuda()
            device.profile_reset()
            device.tracks_batch(seg, pairs, t, torch.tensor([len(mm)], dtype=torch.int32).cuda())
            torch.cuda.synchronize()
            counts[what] = [device.profile_read(k)[0] for k in PROFILE_NAMES]
    finally:
        device.profile_enable(False)
        device.profile_reset()
    assert counts["edges"] == [1, 1, 1, 1, 1, 1, 1, 1]
    assert counts["one edge"] == [1, 1, 1, 1, 1, 1, 0, 1]
    assert counts["capacity 0"] == [1, 0, 1, 1, 1, 1, 0, 0]


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "tracks_batch.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out
