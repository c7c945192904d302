"""CPU-only: one table of calls through the public many-sets wrappers of spectavi_amd.device, .feature and .mvg, with
the class of every refusal and what the legal edge forms return.  The wrappers' own *_plan / *_args tests pin their
ops one by one; this table holds the cases they leave out, so that the argument rules can move between modules
without a caller noticing: the host matchers' pair and width rules, the camera and mask rules of the mvg batch
forms, every device rule alone (whichever rule a wrapper happens to look at first), and the 2^31 / 2^20 edges.

Device wrappers get CPU or meta tensors: their rules come before any device is touched, and a call that passes
them all ends in the TypeError of the "must be on the GPU" check -- which is how an accepted form shows here.  Meta
tensors have a shape and no storage, so a table of 2^31 rows costs nothing."""
import numpy as np
import pytest

import torch

from spectavi_amd import device, feature, mvg
from spectavi_amd._lib import SpectaviError

ACCEPTED = TypeError            # of a device wrapper handed tensors that are not on a GPU
B31 = 2 ** 31
CAP = 2 ** 20                   # sets per call of ransac_fit_batch and dlt_triangulate_batch


def meta(rows, cols, dtype=torch.float64):
    return torch.empty((rows, cols), dtype=dtype, device="meta")


def cpu(rows, cols, dtype=torch.float64):
    return torch.zeros((rows, cols), dtype=dtype)


U8 = np.zeros((0, 16), np.uint8)            # an empty descriptor table: nothing to run, so no device
U8_128 = np.zeros((0, 128), np.uint8)
F32 = np.zeros((0, 16), np.float32)
GEOM0 = np.zeros((0, 4), np.float32)
LINES0 = np.zeros((0, 3))
HD = np.zeros((2, 16, 6), np.float32)       # hash_dict [n, dim, m]
P = np.hstack([np.eye(3), np.ones((3, 1))])
X0 = np.zeros((0, 3))
X4 = np.zeros((4, 3))
SEG = [0, 3, 3, 10]                         # an empty set in the middle
COUNT = torch.zeros(1, dtype=torch.int32)


def views(got, dtypes, npairs, width=2):
    """A host matcher's list over empty tables: one tuple of empty arrays of the stated dtypes per pair."""
    assert isinstance(got, list) and len(got) == npairs
    for row in got:
        assert len(row) == len(dtypes)
        for a, dt in zip(row, dtypes):
            assert a.dtype == dt and len(a) == 0 and a.shape[1:] in ((width,), ())
    return True


def is_plan(got, **want):
    plan = got[0] if isinstance(got, tuple) else got
    for k, v in want.items():
        assert np.array_equal(plan[k], v), (k, plan[k], v)
        if isinstance(v, np.ndarray):
            assert plan[k].dtype == v.dtype
    return True


def off64(*v):
    return np.array(v, np.int64)


def tracks_args(got, seg, prs):
    s, p = got
    assert s.dtype == np.int64 and s.tolist() == seg and s.flags.c_contiguous
    assert p.dtype == np.int32 and p.shape == (len(prs), 2) and p.tolist() == prs and p.flags.c_contiguous
    return True


def dlt_args(got, off, use, p1_zero_rows):
    o, P1s, P0s, u = got
    assert o.dtype == np.int64 and o.tolist() == off
    assert P1s.dtype == np.float64 and P1s.shape == (len(off) - 1, 12) and P1s.flags.c_contiguous
    assert [bool((row == 0).all()) for row in P1s] == p1_zero_rows
    assert P0s is None
    assert (u is None and use is None) or (u.dtype == np.int32 and u.tolist() == use and u.flags.c_contiguous)
    return True


def tri_args(got, use):
    seg, cams, u, off, max_error = got
    assert seg.dtype == off.dtype == np.int64 and cams.dtype == np.float64 and cams.shape == (len(seg) - 1, 12)
    assert (u is None and use is None) or (u.dtype == np.int32 and u.tolist() == use)
    assert isinstance(max_error, float)
    return True


def rect_args(got, use, npairs):
    sizes, pairs, P1s, P0s, u, box = got
    assert sizes.dtype == pairs.dtype == np.int32 and pairs.shape == (npairs, 2)
    assert P1s.dtype == np.float64 and P1s.shape == (npairs, 12) and P0s is None and box is None
    assert (u is None and use is None) or (u.dtype == np.int32 and u.tolist() == use)
    return True


def fits_without_a_model(got, n):
    assert len(got) == n
    for r in got:
        assert r["success"] is False and r["essential"] is None and r["camera"] is None and r["tries_run"] == 0
        assert r["inlier_idx"].dtype == np.int32 and len(r["inlier_idx"]) == 0 and r["best_try"] == -1
    return True


def shapes(got, *want):
    assert [tuple(a.shape) for a in got] == list(want), [a.shape for a in got]
    return True


def l1(tables, pairs=None):
    return feature.nn_bruteforcel1k2_batch(tables, pairs)


def gd(tables, geoms, lines, pairs=None):
    return feature.nn_bruteforcel1k2_guided_batch(tables, geoms, lines, 1.0, pairs)


def ch(tables, hd=HD, pairs=None, g=2, **kw):
    return feature.nn_cascading_hash_batch(tables, hd, pairs, g=g, **kw)


def dfit(x0, x1, off, **kw):
    return device.ransac_fit_batch(x0, x1, off, **kw)


def ddlt(x0, x1, off, P1s, **kw):
    return device.dlt_triangulate_batch(x0, x1, off, P1s, **kw)


def dgather(geom, seg, prs, matches=None):
    return device.match_coordinates_batch(geom, seg, prs, cpu(8, 2, torch.int32) if matches is None else matches, COUNT)


def dtracks(seg, prs, cap=4, **kw):
    return device.tracks_batch(seg, prs, cpu(cap, 2, torch.int32), COUNT, **kw)


def dtri(geom, seg, cams, off, members, **kw):
    return device.triangulate_tracks(geom, seg, cams, off, members, **kw)


def rect(ims, pairs, P1s, P0s=None, **kw):
    return mvg.image_pair_rectification_batch(ims, pairs, P1s, P0s, **kw)


def hdlt(P1s, x0s, x1s=None, **kw):
    return mvg.dlt_triangulate_batch(P1s, x0s, x0s if x1s is None else x1s, **kw)


IM = np.zeros((4, 5))
SAMPLES = np.tile(np.arange(7, dtype=np.int32), (2, 3, 1))
TWO_CAMS = np.zeros((2, 3, 4))
GEOM6, MEM5 = cpu(6, 4, torch.float32), cpu(5, 2, torch.int32)

# (what, call, the class raised -- or a function of what comes back that asserts and returns True)
CASES = [
    # ---- feature.nn_bruteforcel1k2_batch: tables, width and pair rules on the host
    ("l1k2 host: no tables", lambda: l1([]), ValueError),
    ("l1k2 host: a 1-D table", lambda: l1([np.zeros(16, np.uint8)]), ValueError),
    ("l1k2 host: a float table", lambda: l1([F32, F32]), ValueError),
    ("l1k2 host: two widths", lambda: l1([U8, U8_128]), ValueError),
    ("l1k2 host: width 8", lambda: l1([np.zeros((0, 8), np.uint8)] * 2), ValueError),
    ("l1k2 host: width 0", lambda: l1([np.zeros((0, 0), np.uint8)] * 2), ValueError),
    ("l1k2 host: width 272", lambda: l1([np.zeros((0, 272), np.uint8)] * 2), ValueError),
    ("l1k2 host: width 256 is taken", lambda: l1([np.zeros((0, 256), np.uint8)] * 2), lambda r: views(r, ("uint64", "int32"), 1)),
    ("l1k2 host: a pair past the tables", lambda: l1([U8, U8], [(0, 2)]), ValueError),
    ("l1k2 host: a negative pair", lambda: l1([U8, U8], [(-1, 0)]), ValueError),
    ("l1k2 host: pairs 1-D", lambda: l1([U8, U8], [0, 1]), ValueError),
    ("l1k2 host: pairs [n, 3]", lambda: l1([U8, U8], [(0, 1, 0)]), ValueError),
    ("l1k2 host: float pairs", lambda: l1([U8, U8], [(0.0, 1.0)]), ValueError),
    ("l1k2 host: pairs=None of 3 tables", lambda: l1([U8] * 3), lambda r: views(r, ("uint64", "int32"), 3)),
    ("l1k2 host: pairs=None of 1 table", lambda: l1([U8]), lambda r: r == []),
    ("l1k2 host: no pairs", lambda: l1([U8, U8], []), lambda r: r == []),
    ("l1k2 host: self and duplicate pairs", lambda: l1([U8, U8], [(0, 0), (1, 0), (1, 0)]),
     lambda r: views(r, ("uint64", "int32"), 3)),
    ("l1k2 host: unsigned pairs", lambda: l1([U8, U8], np.array([(1, 0)], np.uint8)), lambda r: views(r, ("uint64", "int32"), 1)),
    # ---- feature.nn_bruteforcel1k2_guided_batch
    ("guided host: no tables", lambda: gd([], [], LINES0), ValueError),
    ("guided host: width 16", lambda: gd([U8, U8], [GEOM0, GEOM0], LINES0), ValueError),
    ("guided host: two widths", lambda: gd([U8_128, U8], [GEOM0, GEOM0], LINES0), ValueError),
    ("guided host: a float table", lambda: gd([np.zeros((0, 128), np.float32)] * 2, [GEOM0, GEOM0], LINES0), ValueError),
    ("guided host: one geom short", lambda: gd([U8_128, U8_128], [GEOM0], LINES0), ValueError),
    ("guided host: float64 geom", lambda: gd([U8_128, U8_128], [GEOM0, GEOM0.astype(np.float64)], LINES0), ValueError),
    ("guided host: geom rows", lambda: gd([U8_128, U8_128], [GEOM0, np.zeros((1, 4), np.float32)], LINES0), ValueError),
    ("guided host: a pair past the tables", lambda: gd([U8_128, U8_128], [GEOM0, GEOM0], LINES0, [(2, 0)]), ValueError),
    ("guided host: a negative pair", lambda: gd([U8_128, U8_128], [GEOM0, GEOM0], LINES0, [(0, -1)]), ValueError),
    ("guided host: float pairs", lambda: gd([U8_128, U8_128], [GEOM0, GEOM0], LINES0, [(0.5, 1)]), ValueError),
    ("guided host: lines rows", lambda: gd([U8_128, U8_128], [GEOM0, GEOM0], np.zeros((1, 3))), ValueError),
    ("guided host: float32 lines", lambda: gd([U8_128, U8_128], [GEOM0, GEOM0], LINES0.astype(np.float32)), ValueError),
    ("guided host: pairs=None of 3 tables", lambda: gd([U8_128] * 3, [GEOM0] * 3, LINES0),
     lambda r: views(r, ("uint64", "int32", "int32"), 3)),
    ("guided host: lines as a list per pair", lambda: gd([U8_128] * 2, [GEOM0] * 2, [LINES0, LINES0], [(0, 1), (0, 1)]),
     lambda r: views(r, ("uint64", "int32", "int32"), 2)),
    ("guided host: no pairs", lambda: gd([U8_128] * 2, [GEOM0] * 2, [], []), lambda r: r == []),
    # ---- feature.nn_cascading_hash_batch
    ("cascade host: no tables", lambda: ch([]), ValueError),
    ("cascade host: a 1-D table", lambda: ch([np.zeros(16, np.float32)]), ValueError),
    ("cascade host: two widths", lambda: ch([F32, np.zeros((0, 32), np.float32)]), ValueError),
    ("cascade host: hash_dict 2-D", lambda: ch([F32, F32], HD[0]), ValueError),
    ("cascade host: hash_dict of another width", lambda: ch([F32, F32], np.zeros((2, 32, 6), np.float32)), ValueError),
    ("cascade host: width 8", lambda: ch([np.zeros((0, 8), np.float32)] * 2, np.zeros((2, 8, 6), np.float32)), ValueError),
    ("cascade host: width 272", lambda: ch([np.zeros((0, 272), np.float32)] * 2, np.zeros((2, 272, 6), np.float32)), ValueError),
    ("cascade host: m 32", lambda: ch([F32, F32], np.zeros((2, 16, 32), np.float32)), ValueError),
    ("cascade host: m 0", lambda: ch([F32, F32], np.zeros((2, 16, 0), np.float32)), ValueError),
    ("cascade host: no hash table", lambda: ch([F32, F32], np.zeros((0, 16, 6), np.float32)), ValueError),
    ("cascade host: g above m", lambda: ch([F32, F32], g=7), ValueError),
    ("cascade host: g negative", lambda: ch([F32, F32], g=-1), ValueError),
    ("cascade host: a pair past the tables", lambda: ch([F32, F32], pairs=[(0, 2)]), ValueError),
    ("cascade host: a negative pair", lambda: ch([F32, F32], pairs=[(-1, 0)]), ValueError),
    ("cascade host: pairs 1-D", lambda: ch([F32, F32], pairs=[0, 1]), ValueError),
    ("cascade host: float pairs", lambda: ch([F32, F32], pairs=[(0.0, 1.0)]), ValueError),
    ("cascade host: pairs=None of 3 tables", lambda: ch([F32] * 3), lambda r: views(r, ("uint64", "float32"), 3)),
    ("cascade host: with ncand", lambda: ch([F32] * 2, return_ncand=True), lambda r: views(r, ("uint64", "float32", "int32"), 1)),
    ("cascade host: no pairs", lambda: ch([F32, F32], pairs=[]), lambda r: r == []),
    ("cascade host: self and duplicate pairs", lambda: ch([F32, F32], pairs=[(1, 1), (0, 1), (0, 1)]),
     lambda r: views(r, ("uint64", "float32"), 3)),
    # ---- feature.normalize_to_ubyte_and_multiple_16_dim_batch (its own dim range)
    ("normalize host: dim 2049", lambda: feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros((0, 2049), np.float32)]),
     ValueError),
    ("normalize host: a 1-D table", lambda: feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros(4, np.float32)]),
     ValueError),
    ("normalize host: empty tables", lambda: feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros((0, 20),
     np.uint8)] * 2),
     lambda r: len(r) == 2 and all(a.shape == (0, 32) and a.dtype == np.float32 for a in r)),
    ("normalize host: empty tables, both images",
     lambda: feature.normalize_to_ubyte_and_multiple_16_dim_batch([np.zeros((0, 20), np.float32)] * 2, want_ubyte=True),
     lambda r: len(r) == 2 and all(a.dtype == np.float32 and b.dtype == np.uint8 and b.shape == (0, 32) for a, b in r)),
    # ---- feature.match_tracks_batch: legal edges (its refusals are in test_tracks_batch_args.py)
    ("tracks host: no table, no pair", lambda: feature.match_tracks_batch([], [], []), lambda r: shapes(r, (1,), (0, 2), (0,))),
    ("tracks host: pairs 1-D", lambda: feature.match_tracks_batch([3, 4], [1, 0], [np.zeros((0, 2), np.int32)]), ValueError),
    ("tracks host: float sizes", lambda: feature.match_tracks_batch([3.0, 4.0], [[1, 0]], [np.zeros((0, 2), np.int32)]),
     ValueError),
    ("tracks host: sizes 2-D", lambda: feature.match_tracks_batch([[3, 4]], [[1, 0]], [np.zeros((0, 2), np.int32)]), ValueError),
    ("tracks host: min_len 2.5", lambda: feature.match_tracks_batch([3, 4], [[1, 0]], [np.zeros((0, 2), np.int32)], min_len=2.5),
     ValueError),
    # ---- mvg.ransac_fit_batch (lists of sets)
    ("fit host: a sample list short", lambda: mvg.ransac_fit_batch([X4, X4], [X4, X4], samples=[SAMPLES[0]]), ValueError),
    ("fit host: samples [ntries, 6]", lambda: mvg.ransac_fit_batch([X4], [X4], samples=[SAMPLES[0][:, :6]]), ValueError),
    ("fit host: seeds short", lambda: mvg.ransac_fit_batch([X4, X4], [X4, X4], seeds=[1]), ValueError),
    ("fit host: tries negative", lambda: mvg.ransac_fit_batch([X4], [X4], maximum_tries=-1), ValueError),
    ("fit host: tries above 7e8", lambda: mvg.ransac_fit_batch([X4], [X4], maximum_tries=700000001), ValueError),
    ("fit host: tries at 7e8, no set runs", lambda: mvg.ransac_fit_batch([X4, X0], [X4, X0], maximum_tries=700000000),
     lambda r: fits_without_a_model(r, 2)),
    ("fit host: coordinate shapes differ", lambda: mvg.ransac_fit_batch([X4], [X0]), TypeError),
    ("fit host: coordinates [n, 2]", lambda: mvg.ransac_fit_batch([X4[:, :2]], [X4[:, :2]]), TypeError),
    ("fit host: samples of short sets are not read", lambda: mvg.ransac_fit_batch([X4, X0], [X4, X0],
     samples=list(SAMPLES + 100)),
     lambda r: fits_without_a_model(r, 2)),
    # ---- mvg.dlt_triangulate_batch: cameras and masks
    ("dlt host: P1s short", lambda: hdlt([P], [X0, X0]), ValueError),
    ("dlt host: camera [4, 4]", lambda: hdlt([np.zeros((4, 4))], [X0]), TypeError),
    ("dlt host: camera [12]", lambda: hdlt([np.zeros(12)], [X0]), TypeError),
    ("dlt host: P0s short", lambda: hdlt([P, P], [X0, X0], P0s=[P]), ValueError),
    ("dlt host: P0s [3, 3]", lambda: hdlt([P], [X0], P0s=[np.zeros((3, 3))]), TypeError),
    ("dlt host: P0s None for a used set", lambda: hdlt([P, P], [X0, X0], P0s=[P, None]), TypeError),
    ("dlt host: P0s None for a skipped set", lambda: hdlt([P, None], [X0, X4], P0s=[P, None]),
     lambda r: shapes(r, (0, 4), (0, 4))),
    ("dlt host: masks short", lambda: hdlt([P, P], [X0, X0], masks=[None]), ValueError),
    ("dlt host: a mask of another length", lambda: hdlt([None], [X4], masks=[np.ones(3)]), ValueError),
    ("dlt host: a mask [n, 1] of the right size", lambda: hdlt([None], [X4], masks=[np.ones((4, 1))]),
     lambda r: shapes(r, (0, 4))),
    ("dlt host: masks with a None entry", lambda: hdlt([None, None], [X4, X4], masks=[None, np.zeros(4)]),
     lambda r: shapes(r, (0, 4), (0, 4))),
    ("dlt host: coordinate shapes differ", lambda: hdlt([P], [X4], [X0]), TypeError),
    ("dlt host: errors of skipped sets", lambda: hdlt([None, P], [X4, X0], ret_error=True),
     lambda r: shapes(r[0], (0, 4), (0, 4)) and shapes(r[1], (0, 1), (0, 1))),
    # ---- mvg.image_pair_rectification_batch: cameras
    ("rectify host: P1s short", lambda: rect([IM, IM], [(0, 1), (1, 0)], [None]), ValueError),
    ("rectify host: P0s short", lambda: rect([IM, IM], [(0, 1)], [None], [None, None]), ValueError),
    ("rectify host: camera [3, 3]", lambda: rect([IM, IM], [(0, 1)], [np.zeros((3, 3))]), TypeError),
    ("rectify host: camera [12]", lambda: rect([IM, IM], [(0, 1)], [np.zeros(12)]), TypeError),
    ("rectify host: P0s [4, 4]", lambda: rect([IM, IM], [(0, 1)], [P], [np.zeros((4, 4))]), TypeError),
    ("rectify host: P0s None for a used pair", lambda: rect([IM, IM], [(0, 1)], [P], [None]), TypeError),
    ("rectify host: P0s None for a skipped pair", lambda: rect([IM, IM], [(0, 1)], [None], [None]), lambda r: r == [None]),
    ("rectify host: a bad P0 of a skipped pair", lambda: rect([IM, IM], [(0, 1)], [None], [np.zeros((2, 2))]), TypeError),
    ("rectify host: channels differ", lambda: rect([IM, np.zeros((4, 5, 3))], [(0, 0)], [None]), TypeError),
    ("rectify host: sizes differ", lambda: rect([IM, IM.T], [(0, 1)], [None]), TypeError),
    ("rectify host: no pairs", lambda: rect([IM], [], []), lambda r: r == []),
    ("rectify host: self and duplicate pairs, none used", lambda: rect([IM, IM], [(0, 0), (1, 0), (1, 0)], [None] * 3),
     lambda r: r == [None] * 3),
    # ---- mvg.triangulate_tracks: a None camera with use, no tracks
    ("tracks triangulate host: None camera and use", lambda: mvg.triangulate_tracks(
        [np.zeros((2, 2)), np.zeros((0, 2)), np.zeros((4, 3))], None, [P, None, P], [0], np.zeros((0, 2), np.int32), use=[0, 1, 1]),
     lambda r: shapes(r, (0, 4), (0,), (0,), (0,))),
    ("tracks triangulate host: camera [4, 4]", lambda: mvg.triangulate_tracks(
        [np.zeros((2, 2))], None, [np.zeros((4, 4))], [0], np.zeros((0, 2), np.int32)), ValueError),
    ("tracks triangulate host: track_off decreases", lambda: mvg.triangulate_tracks(
        [np.zeros((2, 2))], None, [P], [0, 2, 1], np.zeros((1, 2), np.int32)), ValueError),
    ("tracks triangulate host: track_off empty", lambda: mvg.triangulate_tracks(
        [np.zeros((2, 2))], None, [P], [], np.zeros((0, 2), np.int32)), ValueError),
    # ---- device.ransac_fit_batch: every rule alone
    ("fit device: accepted", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 32]), ACCEPTED),
    ("fit device: x1 of another shape", lambda: dfit(cpu(32, 3), cpu(31, 3), [0, 12, 32]), ValueError),
    ("fit device: coordinates [n, 2]", lambda: dfit(cpu(32, 2), cpu(32, 2), [0, 12, 32]), ValueError),
    ("fit device: pair_off empty", lambda: dfit(cpu(0, 3), cpu(0, 3), []), ValueError),
    ("fit device: pair_off from 1", lambda: dfit(cpu(32, 3), cpu(32, 3), [1, 12, 32]), ValueError),
    ("fit device: pair_off decreases", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 33, 32]), ValueError),
    ("fit device: pair_off ends short", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 31]), ValueError),
    ("fit device: 2^31 - 1 rows", lambda: dfit(meta(B31 - 1, 3), meta(B31 - 1, 3), [0, B31 - 1]), ACCEPTED),
    ("fit device: 2^31 rows", lambda: dfit(meta(B31, 3), meta(B31, 3), [0, B31]), ValueError),
    ("fit device: 2^20 sets", lambda: dfit(meta(0, 3), meta(0, 3), np.zeros(CAP + 1, np.int64)), ACCEPTED),
    ("fit device: 2^20 + 1 sets", lambda: dfit(meta(0, 3), meta(0, 3), np.zeros(CAP + 2, np.int64)), ValueError),
    ("fit device: no sets", lambda: dfit(cpu(0, 3), cpu(0, 3), [0]), ACCEPTED),
    ("fit device: float samples", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 32], samples=SAMPLES.astype(np.float64)),
     ValueError),
    ("fit device: samples 2-D", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 32], samples=SAMPLES[0]), ValueError),
    ("fit device: a sample past its set", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 32], samples=SAMPLES + 6), ValueError),
    ("fit device: samples of a short set are not read", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 9, 32], samples=SAMPLES + 6),
     ACCEPTED),
    ("fit device: seeds 2-D of the right size", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 32], seeds=[[1], [2]]), ACCEPTED),
    ("fit device: tries at 7e8", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 32], maximum_tries=700000000), ACCEPTED),
    ("fit device: samples decide the tries", lambda: dfit(cpu(32, 3), cpu(32, 3), [0, 12, 32], samples=SAMPLES, maximum_tries=-1),
     ACCEPTED),
    # ---- device.ransac_fit_batch_plan / dlt_triangulate_batch_plan: only emptiness is theirs, the library has the rest
    ("fit plan: pair_off empty", lambda: device.ransac_fit_batch_plan([]), ValueError),
    ("fit plan: pair_off from 1", lambda: device.ransac_fit_batch_plan([1, 20]), SpectaviError),
    ("fit plan: pair_off decreases", lambda: device.ransac_fit_batch_plan([0, 20, 10]), SpectaviError),
    ("fit plan: 2^31 rows", lambda: device.ransac_fit_batch_plan([0, B31]), SpectaviError),
    ("fit plan: 2^31 - 1 rows", lambda: device.ransac_fit_batch_plan([0, B31 - 1]), lambda r: r["sets"] == 1),
    ("fit plan: no sets", lambda: device.ransac_fit_batch_plan([0]), lambda r: r == dict(sets=0, tries=0, items=0, row_blocks=0)),
    ("fit plan: 2^20 + 1 sets", lambda: device.ransac_fit_batch_plan(np.zeros(CAP + 2, np.int64)), SpectaviError),
    ("fit plan: 2^20 sets", lambda: device.ransac_fit_batch_plan(np.zeros(CAP + 1, np.int64)), lambda r: r["sets"] == 0),
    ("dlt plan: pair_off empty", lambda: device.dlt_triangulate_batch_plan([]), ValueError),
    ("dlt plan: pair_off decreases", lambda: device.dlt_triangulate_batch_plan([0, 3, 2]), SpectaviError),
    ("dlt plan: 2^31 rows", lambda: device.dlt_triangulate_batch_plan([0, B31]), SpectaviError),
    ("dlt plan: 2^31 - 1 rows", lambda: device.dlt_triangulate_batch_plan([0, B31 - 1]), lambda r: r["bound"] == B31 - 1),
    ("dlt plan: 2^20 + 1 sets", lambda: device.dlt_triangulate_batch_plan(np.zeros(CAP + 2, np.int64)), SpectaviError),
    ("dlt plan: 2^20 sets", lambda: device.dlt_triangulate_batch_plan(np.zeros(CAP + 1, np.int64)), lambda r: r["sets"] == CAP),
    ("dlt plan: use short", lambda: device.dlt_triangulate_batch_plan([0, 2, 4], use=[1]), ValueError),
    ("dlt plan: use of any non-zero value", lambda: device.dlt_triangulate_batch_plan([0, 2, 4, 9], use=[-3, 0.0, 0.5]),
     lambda r: r == dict(sets=2, items=2, bound=7)),
    # ---- device.dlt_triangulate_batch
    ("dlt device: accepted", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 5], TWO_CAMS), ACCEPTED),
    ("dlt device: x1 of another shape", lambda: ddlt(cpu(5, 3), cpu(4, 3), [0, 3, 5], TWO_CAMS), ValueError),
    ("dlt device: pair_off empty", lambda: ddlt(cpu(0, 3), cpu(0, 3), [], TWO_CAMS[:0]), ValueError),
    ("dlt device: pair_off from 1", lambda: ddlt(cpu(5, 3), cpu(5, 3), [1, 3, 5], TWO_CAMS), ValueError),
    ("dlt device: pair_off decreases", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 6, 5], TWO_CAMS), ValueError),
    ("dlt device: pair_off ends short", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 4], TWO_CAMS), ValueError),
    ("dlt device: 2^31 rows", lambda: ddlt(meta(B31, 3), meta(B31, 3), [0, B31], TWO_CAMS[:1]), ValueError),
    ("dlt device: 2^31 - 1 rows", lambda: ddlt(meta(B31 - 1, 3), meta(B31 - 1, 3), [0, B31 - 1], TWO_CAMS[:1]), ACCEPTED),
    ("dlt device: 2^20 + 1 sets", lambda: ddlt(meta(0, 3), meta(0, 3), np.zeros(CAP + 2, np.int64), TWO_CAMS), ValueError),
    ("dlt device: no sets", lambda: ddlt(cpu(0, 3), cpu(0, 3), [0], []), ACCEPTED),
    ("dlt device: use short", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 5], TWO_CAMS, use=[1]), ValueError),
    ("dlt device: a camera short", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 5], TWO_CAMS[:1]), ValueError),
    ("dlt device: a list with None short", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 5], [None]), ValueError),
    ("dlt device: P0s short", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 5], TWO_CAMS, P0s=TWO_CAMS[:1]), ValueError),
    ("dlt device: cameras [n, 12]", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 5], np.zeros((2, 12))), ACCEPTED),
    ("dlt device: a None camera with use", lambda: ddlt(cpu(5, 3), cpu(5, 3), [0, 3, 5], [None, P], use=[1, 1]), ACCEPTED),
    ("dlt args: a None camera with use", lambda: device._dlt_batch_args([0, 3, 5, 5], 5, [P, None, P], None, [0, 2, 1]),
     lambda r: dlt_args(r, [0, 3, 5, 5], [0, 0, 1], [False, True, False])),
    ("dlt args: a None camera without use", lambda: device._dlt_batch_args([0, 3, 5], None, [None, P], None, None),
     lambda r: dlt_args(r, [0, 3, 5], [0, 1], [True, False])),
    ("dlt args: no None, no use", lambda: device._dlt_batch_args([0, 3, 5], 5, [P, P], None, None),
     lambda r: dlt_args(r, [0, 3, 5], None, [False, False])),
    ("dlt args: no sets", lambda: device._dlt_batch_args([0], 0, [], None, []), lambda r: dlt_args(r, [0], [], [])),
    # ---- device.match_coordinates_batch (the pair rules without a width rule)
    ("gather: accepted", lambda: dgather(cpu(10, 4, torch.float32), SEG, [[2, 0], [1, 0], [2, 2], [2, 0]]), ACCEPTED),
    ("gather: no sets, no pairs", lambda: dgather(cpu(0, 4, torch.float32), [0], []), ACCEPTED),
    ("gather: seg_off empty", lambda: dgather(cpu(0, 4, torch.float32), [], []), ValueError),
    ("gather: seg_off ends short", lambda: dgather(cpu(10, 4, torch.float32), [0, 3, 9], [[0, 1]]), ValueError),
    ("gather: a pair past the sets", lambda: dgather(cpu(10, 4, torch.float32), SEG, [[3, 0]]), ValueError),
    ("gather: float pairs", lambda: dgather(cpu(10, 4, torch.float32), SEG, [[1.0, 0.0]]), ValueError),
    ("gather: pairs [n, 3]", lambda: dgather(cpu(10, 4, torch.float32), SEG, [[1, 0, 0]]), ValueError),
    ("gather: pairs None", lambda: dgather(cpu(10, 4, torch.float32), SEG, None), ValueError),
    ("gather: matches [n, 3]", lambda: dgather(cpu(10, 4, torch.float32), SEG, [[1, 0]], cpu(8, 3, torch.int32)), ValueError),
    ("gather: 2^31 - 1 rows", lambda: dgather(meta(B31 - 1, 4, torch.float32), [0, B31 - 1], [[0, 0]]), ACCEPTED),
    ("gather: 2^31 rows", lambda: dgather(meta(B31, 4, torch.float32), [0, B31], []), ValueError),
    ("gather: 2^31 out rows", lambda: dgather(meta(2 ** 30, 4, torch.float32), [0, 2 ** 30], [[0, 0], [0, 0]]), ValueError),
    # ---- device.tracks_batch / _tracks_batch_args
    ("tracks device: accepted", lambda: dtracks(SEG, [[2, 0], [1, 0]]), ACCEPTED),
    ("tracks device: seg_off empty", lambda: dtracks([], []), ValueError),
    ("tracks device: float pairs", lambda: dtracks(SEG, [[2.0, 0.0]]), ValueError),
    ("tracks device: pairs 1-D", lambda: dtracks(SEG, [2, 0]), ValueError),
    ("tracks device: matches [n, 3]", lambda: device.tracks_batch(SEG, [[2, 0]], cpu(4, 3, torch.int32), COUNT), ValueError),
    ("tracks device: min_len 2.5", lambda: dtracks(SEG, [[2, 0]], min_len=2.5), ValueError),
    ("tracks args: 2^31 - 1 rows", lambda: device._tracks_batch_args([0, B31 - 1], [[0, 0]], 0, 2),
     lambda r: tracks_args(r, [0, B31 - 1], [[0, 0]])),
    ("tracks args: 2^31 rows", lambda: device._tracks_batch_args([0, B31], [], 0, 2), ValueError),
    ("tracks args: 2^31 - 1 out rows", lambda: device._tracks_batch_args([0, 2 ** 30, B31 - 1], [[0, 0], [1, 1]], 0, 2),
     lambda r: tracks_args(r, [0, 2 ** 30, B31 - 1], [[0, 0], [1, 1]])),
    ("tracks args: empty set in the middle, unsigned pairs",
     lambda: device._tracks_batch_args(SEG, np.array([[1, 1], [2, 1]], np.uint16), 3,
     3),
     lambda r: tracks_args(r, SEG, [[1, 1], [2, 1]])),
    # ---- device.triangulate_tracks / its plan
    ("triangulate device: accepted with a None camera and use",
     lambda: dtri(GEOM6, [0, 2, 6], [None, P], [0, 2, 5], MEM5, use=[1, 0]), ACCEPTED),
    ("triangulate device: no sets, no tracks", lambda: dtri(cpu(0, 4, torch.float32), [0], [], [0], cpu(0, 2, torch.int32)),
     ACCEPTED),
    ("triangulate device: seg_off empty", lambda: dtri(GEOM6, [], TWO_CAMS, [0, 2, 5], MEM5), ValueError),
    ("triangulate device: 2^31 - 1 members", lambda: dtri(GEOM6, [0, 2, 6], TWO_CAMS, [0, B31 - 1], meta(B31 - 1, 2,
     torch.int32)),
     ACCEPTED),
    ("triangulate device: 2^31 members", lambda: dtri(GEOM6, [0, 2, 6], TWO_CAMS, [0, B31], meta(B31, 2, torch.int32)),
     ValueError),
    ("triangulate device: 2^31 - 1 rows", lambda: dtri(meta(B31 - 1, 4, torch.float32), [0, 2, B31 - 1], TWO_CAMS, [0, 2, 5],
     MEM5),
     ACCEPTED),
    ("triangulate device: 2^31 rows", lambda: dtri(meta(B31, 4, torch.float32), [0, 2, B31], TWO_CAMS, [0, 2, 5], MEM5),
     ValueError),
    ("triangulate device: a camera that is no number", lambda: dtri(GEOM6, [0, 2, 6], [P, "camera"], [0, 2, 5], MEM5),
     ValueError),
    ("triangulate device: a ragged camera list", lambda: dtri(GEOM6, [0, 2, 6], [P, P[:2]], [0, 2, 5], MEM5), ValueError),
    ("triangulate args: a None camera with use",
     lambda: device._tracks_triangulate_args((6, 4), [0, 2, 2, 6], [P, None, P], [0, 2, 5], (5, 2), 1, [5, 1, 0]),
     lambda r: tri_args(r, [1, 0, 0])),
    ("triangulate args: no None, no use",
     lambda: device._tracks_triangulate_args((6, 4), [0, 2, 6], TWO_CAMS, [0, 2, 5], (5, 2), 1, None), lambda r: tri_args(r, None)),
    ("triangulate plan: 2^31 - 1 members", lambda: device.triangulate_tracks_plan([0, 2, B31 - 1]),
     lambda r: r["longest"] == B31 - 3 and r["lane_tracks"] + r["wave_tracks"] == 2),
    ("triangulate plan: 2^31 members", lambda: device.triangulate_tracks_plan([0, B31]), ValueError),
    # ---- the matchers' plans: offsets, width and pair rules of the device side
    ("l1k2 plan: no sets, no pairs", lambda: device.l1k2_batch_plan([0], [], 16),
     lambda r: is_plan(r, items=0, out_rows=0, out_off=off64(0))),
    ("l1k2 plan: empty sets, self and duplicate pairs", lambda: device.l1k2_batch_plan(SEG, [[1, 0], [2, 2], [0, 2], [0, 2]],
     128),
     lambda r: is_plan(r, out_rows=13, out_off=off64(0, 0, 7, 10, 13))),
    ("l1k2 plan: seg_off empty", lambda: device.l1k2_batch_plan([], [], 16), ValueError),
    ("l1k2 plan: float pairs", lambda: device.l1k2_batch_plan(SEG, [[1.0, 0.0]], 16), ValueError),
    ("l1k2 plan: pairs None", lambda: device.l1k2_batch_plan(SEG, None, 16), ValueError),
    ("l1k2 plan: width 0", lambda: device.l1k2_batch_plan(SEG, [[1, 0]], 0), ValueError),
    ("l1k2 plan: width 272", lambda: device.l1k2_batch_plan(SEG, [[1, 0]], 272), ValueError),
    ("l1k2 plan: 2^31 - 1 rows", lambda: device.l1k2_batch_plan([0, B31 - 1], [], 16),
     lambda r: is_plan(r, out_rows=0, out_off=off64(0))),
    ("l1k2 plan: 2^31 rows", lambda: device.l1k2_batch_plan([0, B31], [], 16), ValueError),
    ("guided plan: no sets, no pairs", lambda: device.l1k2_guided_batch_plan([0], []),
     lambda r: is_plan(r, items=0, out_off=off64(0))),
    ("guided plan: width 144", lambda: device.l1k2_guided_batch_plan(SEG, [[1, 0]], 144), ValueError),
    ("guided plan: width 8", lambda: device.l1k2_guided_batch_plan(SEG, [[1, 0]], 8), ValueError),
    ("guided plan: 2^31 rows", lambda: device.l1k2_guided_batch_plan([0, B31], []), ValueError),
    ("cascade plan: no sets, no pairs", lambda: device.cascade_batch_plan([0], [], 16, 6, 2, 2),
     lambda r: is_plan(r, items=0, out_off=off64(0))),
    ("cascade plan: empty set in the middle", lambda: device.cascade_batch_plan(SEG, [[2, 1], [1, 2], [0, 0]], 16, 6, 2, 2),
     lambda r: is_plan(r, out_rows=10, out_off=off64(0, 7, 7, 10))),
    ("cascade plan: a pair past the sets", lambda: device.cascade_batch_plan(SEG, [[3, 0]], 16, 6, 2, 2), ValueError),
    ("cascade plan: width 24", lambda: device.cascade_batch_plan(SEG, [[1, 0]], 24, 6, 2, 2), ValueError),
    ("cascade plan: m 32", lambda: device.cascade_batch_plan(SEG, [[1, 0]], 16, 32, 2, 2), ValueError),
    ("cascade plan: g above m", lambda: device.cascade_batch_plan(SEG, [[1, 0]], 16, 6, 2, 7), ValueError),
    ("cascade plan: nseg * n above 65535", lambda: device.cascade_batch_plan(np.zeros(32769, np.int64), [], 16, 6, 2, 2),
     ValueError),
    ("cascade plan: 2^31 rows", lambda: device.cascade_batch_plan([0, B31], [], 16, 6, 2, 2), ValueError),
    ("normalize plan: 2^31 rows", lambda: device.normalize_batch_plan([0, B31], 128, "uint8"), ValueError),
    ("normalize plan: 2^31 - 1 rows", lambda: device.normalize_batch_plan([0, 0, B31 - 1], 128, np.float32),
     lambda r: r["sets"] == 1 and r["rows"] == B31 - 1),
    ("normalize plan: no sets", lambda: device.normalize_batch_plan([0], 128, torch.uint8),
     lambda r: r["sets"] == 0 and r["rows"] == 0),
    ("normalize plan: dim 24 (its own range)", lambda: device.normalize_batch_plan([0, 4], 24, "float32"),
     lambda r: r["sets"] == 1),
    # ---- device.epipolar_lines_batch: what comes before the device check
    ("lines: geom [n, 3]", lambda: device.epipolar_lines_batch(cpu(10, 3, torch.float32), SEG, [[1, 0]], np.zeros((1, 9))),
     ValueError),
    ("lines: float64 geom", lambda: device.epipolar_lines_batch(cpu(10, 4), SEG, [[1, 0]], np.zeros((1, 9))), ValueError),
    ("lines: accepted as far as the device",
     lambda: device.epipolar_lines_batch(cpu(10, 4, torch.float32), SEG, [[1, 0]], np.zeros((1,
     9))),
     ACCEPTED),
    # ---- the rectify batch: counts are the wrapper's, pairs and sizes the library's
    ("rectify plan: a pair past the images", lambda: device.rectify_batch_plan([(5, 4)], [(0, 1)]), SpectaviError),
    ("rectify plan: no pairs", lambda: device.rectify_batch_plan([(5, 4)], []),
     lambda r: is_plan(r, pairs=0, items=0, out_off=off64(0))),
    ("rectify plan: use of any non-zero value", lambda: device.rectify_batch_plan([(5, 4)], [(0, 0), (0, 0)], use=[0, -2]),
     lambda r: r["pairs"] == 1),
    ("rectify args: a None camera with use", lambda: device._rectify_batch_args([(5, 4)], [(0, 0)] * 3, [P, None, P], None, [0, 1,
     7]),
     lambda r: rect_args(r, [0, 0, 1], 3)),
    ("rectify args: a None camera without use", lambda: device._rectify_batch_args([(5, 4)], [(0, 0)] * 2, [None, P], None, None),
     lambda r: rect_args(r, [0, 1], 2)),
    ("rectify args: a list with None short", lambda: device._rectify_batch_args([(5, 4)], [(0, 0)] * 2, [None], None, None),
     ValueError),
    ("rectify args: cameras short", lambda: device._rectify_batch_args([(5, 4)], [(0, 0)] * 2, TWO_CAMS[:1], None, None),
     ValueError),
    ("rectify args: P0s short", lambda: device._rectify_batch_args([(5, 4)], [(0, 0)] * 2, TWO_CAMS, TWO_CAMS[:1], None),
     ValueError),
    ("rectify args: use short", lambda: device._rectify_batch_args([(5, 4)], [(0, 0)] * 2, TWO_CAMS, None, [1]), ValueError),
    # ---- the SIFT batch offsets (its sizes rule is its own)
    ("sift: cap_off short", lambda: device.sift_batch_into(cpu(1, 20, torch.float32), [(5, 4)], cpu(8, 132, torch.float32), [0],
     COUNT),
     ValueError),
    ("sift: cap_off from 1",
     lambda: device.sift_batch_into(cpu(1, 20, torch.float32), [(5, 4)], cpu(8, 132, torch.float32), [1, 8],
     COUNT),
     ValueError),
    ("sift: cap_off decreases", lambda: device.sift_batch_into(cpu(1, 40, torch.float32), [(5, 4)] * 2, cpu(8, 132,
     torch.float32),
                                                             [0, 9, 8], torch.zeros(2, dtype=torch.int32)), ValueError),
    ("sift: cap_off to 2^31",
     lambda: device.sift_batch_into(cpu(1, 20, torch.float32), [(5, 4)], cpu(8, 132, torch.float32), [0, B31],
     COUNT),
     ValueError),
    ("sift: cap_off to 2^31 - 1", lambda: device.sift_batch_into(cpu(1, 20, torch.float32), [(5, 4)], cpu(8, 132, torch.float32),
                                                               [0, B31 - 1], COUNT), ACCEPTED),
    ("sift: a side of 8193", lambda: device.sift_batch_plan([(8193, 4)]), ValueError),
]

assert len({c[0] for c in CASES}) == len(CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_wrapper(case):
    _, call, want = case
    if isinstance(want, type):
        with pytest.raises(want) as info:
            call()
        assert info.type is want, "the class itself, not a subclass of it"
    else:
        assert want(call()) is True
