"""normalize_batch on the GPU: every set of a collection bit for bit device.normalize of that set alone (whose numpy
identity tests/test_sift_adapter_gpu.py pins) and, where NaN does not make numpy's uint8 cast platform-defined,
numpy's own result -- the float table always, the uint8 table where the float table is finite.

Which case reaches which instantiation of normalize_batch.hip (INSTANTIATED):
  normalize_batch_stats_kernel<16>              uint8 ragged at dim 128; the 2^24 edge (dim 16)
  normalize_batch_stats_kernel<1>               uint8 ragged at dim 20 and 21; dim 1
  normalize_batch_finish_kernel<unsigned char>  every uint8 case: the integer shortcut in the ragged ones and the edge's
                                                65793-row set, the walk in the edge's 65800- and 140000-row sets
  normalize_batch_finish_kernel<float>          every float32 case
  normalize_batch_kernel<unsigned char, 4>      uint8 ragged at dim 128 and 20; the edge
  normalize_batch_kernel<float, 4>              float32 ragged at dim 128 and 20
  normalize_batch_kernel<unsigned char, 1>      uint8 ragged at dim 21; dim 1
  normalize_batch_kernel<float, 1>              float32 ragged at dim 21; dim 1
"""
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INSTANTIATED = {"normalize_batch_stats_kernel<16>", "normalize_batch_stats_kernel<1>",
                "normalize_batch_finish_kernel<unsigned char>", "normalize_batch_finish_kernel<float>",
                "normalize_batch_kernel<unsigned char, 4>", "normalize_batch_kernel<unsigned char, 1>",
                "normalize_batch_kernel<float, 4>", "normalize_batch_kernel<float, 1>"}

SIZES = [0, 1, 2, 255, 256, 257, 0, 1500, 3]
BIG = 7  # the 1500-row set: six work items
DIMS = [128, 20, 21]  # 16-byte loads; padded to 32, no 16-byte loads; no 4-wide loads either
EDGE = [65793, 65800, 140000]  # 255 * 65793 = 2^24 - 1


def _off(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def bits(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def numpy_tables(x):
    """(float table, uint8 table, where the uint8 table is numpy's to say) of one set, by the reference's function."""
    from spectavi_amd import feature
    with np.errstate(all="ignore"):
        f = feature.normalize_to_ubyte_and_multiple_16_dim(x.astype(np.float32))
        finite = np.isfinite(f)
        u = (np.where(finite, f, 0) + 128).astype(np.uint8)
    return f, u, finite


@functools.lru_cache(maxsize=None)
def ragged(kind, dim):
    """The sets of the ragged collection (read only): random bytes, for float32 plus a random fraction so that the
    column sums round; column 3 constant within the 1500-row set, column 5 constant across all sets; for float32 an
    inf in column 1 and a nan in column 2 of the 1500-row set."""
    rng = np.random.default_rng(1000 * dim + (kind == "float32"))
    sets = []
    for s, n in enumerate(SIZES):
        x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
        x[:, 5] = 77
        if s == BIG:
            x[:, 3] = 200
        if kind == "float32":
            x = x.astype(np.float32) + rng.random((n, dim), dtype=np.float32)
            x[:, 5] = 77.25
            if s == BIG:
                x[:, 3] = -3.5
                x[1000, 1] = np.inf
                x[700, 2] = np.nan
        x.setflags(write=False)
        sets.append(x)
    return tuple(sets)


@functools.lru_cache(maxsize=None)
def single_calls(kind, dim):
    """device.normalize of every set of ragged(kind, dim) alone: (float table, uint8 table) per set, on the host."""
    import torch
    from spectavi_amd import device
    out = []
    for x in ragged(kind, dim):
        if len(x) == 0:
            out.append((np.zeros((0, (dim + 15) // 16 * 16), np.float32), np.zeros((0, (dim + 15) // 16 * 16), np.uint8)))
            continue
        f, u = device.normalize(torch.from_numpy(x.astype(np.float32)).cuda(), want_float=True, want_ubyte=True)
        out.append((f.cpu().numpy(), u.cpu().numpy()))
    return out


def run_batch(sets, **kw):
    """device.normalize_batch of the sets in this order -> per-set (float table, uint8 table) on the host."""
    import torch
    from spectavi_amd import device
    off = _off([len(x) for x in sets])
    f, u = device.normalize_batch(torch.from_numpy(np.concatenate(sets)).cuda(), off, want_float=True, want_ubyte=True, **kw)
    f, u = f.cpu().numpy(), u.cpu().numpy()
    return [(f[a:b], u[a:b]) for a, b in zip(off[:-1], off[1:])]


def assert_same_bits(got, want, what):
    for s, ((gf, gu), (wf, wu)) in enumerate(zip(got, want)):
        assert gf.shape == wf.shape and gu.shape == wu.shape, (what, s)
        assert np.array_equal(bits(gf), bits(wf)), "%s: float table of set %d" % (what, s)
        assert np.array_equal(gu, wu), "%s: uint8 table of set %d" % (what, s)


def assert_numpys(got, sets, what):
    for s, ((gf, gu), x) in enumerate(zip(got, sets)):
        if len(x) == 0:
            continue
        f, u, finite = numpy_tables(x)
        assert np.array_equal(gf, f, equal_nan=True), "%s: float table of set %d against numpy" % (what, s)
        assert np.array_equal(gu[finite], u[finite]), "%s: uint8 table of set %d against numpy" % (what, s)


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "normalize_batch.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("kind", ["float32", "uint8"])
def test_ragged_collection(kind, dim):
    from spectavi_amd import device, feature
    sets = ragged(kind, dim)
    plan = device.normalize_batch_plan(_off(SIZES), dim, kind)
    assert plan["sets"] == 7 and plan["items"] == 1 + 1 + 1 + 1 + 2 + 6 + 1
    got = run_batch(sets)
    assert_same_bits(got, single_calls(kind, dim), "device form")
    assert_numpys(got, sets, "device form")
    # what the 1500-row set is there for: NaN columns (0 / 0), and for float32 the inf and nan columns
    f = got[BIG][0]
    assert np.isnan(f[:, 3]).all() and np.isnan(f[:, 5]).all() and np.isfinite(f[:, 0]).all()
    assert np.isnan(got[1][0][:, :dim]).all() and not got[1][0][:, dim:].any(), "a one-row set is 0 / 0, padded with zeros"
    if kind == "float32":
        assert np.isnan(f[:, 1]).all() and np.isnan(f[:, 2]).all()
    host = feature.normalize_to_ubyte_and_multiple_16_dim_batch(list(sets), want_ubyte=True)
    assert_same_bits(host, got, "host form")
    floats_only = feature.normalize_to_ubyte_and_multiple_16_dim_batch(list(sets))
    assert all(np.array_equal(bits(a), bits(b[0])) for a, b in zip(floats_only, got))


@pytest.mark.parametrize("kind", ["float32", "uint8"])
def test_position_independence(kind):
    """The same sets in another order, and one set as a collection of one: the same bits per set."""
    sets, want = ragged(kind, 128), single_calls(kind, 128)
    order = [7, 3, 0, 8, 5, 1, 6, 4, 2]
    got = run_batch([sets[s] for s in order])
    assert_same_bits(got, [want[s] for s in order], "permuted")
    for s in (BIG, 4, 1):
        assert_same_bits(run_batch([sets[s]]), [want[s]], "set %d alone" % s)


def test_only_its_rows_are_written():
    """Guard rows either side of both outputs keep their sentinel; with the float table alone nothing is allocated
    for the other one."""
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib, check
    sets = ragged("uint8", 20)
    off = _off(SIZES)
    total, guard = int(off[-1]), 64
    x = torch.from_numpy(np.concatenate(sets)).cuda()
    f = torch.full((total + 2 * guard, 32), 12345.0, dtype=torch.float32, device="cuda")
    u = torch.full((total + 2 * guard, 32), 199, dtype=torch.uint8, device="cuda")
    ws = torch.zeros(device.normalize_batch_plan(off, 20, "uint8")["workspace_bytes"], dtype=torch.uint8, device="cuda")
    stream = device._stream()
    for of, ou in ((f, u), (f, None), (None, u)):
        if of is not None:
            of.fill_(12345.0)
        if ou is not None:
            ou.fill_(199)
        check(clib.spv_normalize_batch_device(x.data_ptr(), 1, off.ctypes.data, len(SIZES), 20,
                                              of[guard:].data_ptr() if of is not None else None,
                                              ou[guard:].data_ptr() if ou is not None else None, ws.data_ptr(), ws.numel(), stream))
        torch.cuda.synchronize()
        want = single_calls("uint8", 20)
        if of is not None:
            h = of.cpu().numpy()
            assert np.all(h[:guard] == 12345.0) and np.all(h[guard + total:] == 12345.0), "the float guard rows"
            assert np.array_equal(bits(h[guard:guard + total]), bits(np.concatenate([w[0] for w in want])))
        if ou is not None:
            h = ou.cpu().numpy()
            assert np.all(h[:guard] == 199) and np.all(h[guard + total:] == 199), "the uint8 guard rows"
            assert np.array_equal(h[guard:guard + total], np.concatenate([w[1] for w in want]))
    # the wrapper: one table asked for, one table allocated (the workspace is there after the first call)
    wsp = device.Workspace()
    device.normalize_batch(x, off, workspace=wsp)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    out = device.normalize_batch(x, off, workspace=wsp)
    grown = torch.cuda.memory_allocated() - before
    assert isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.shape == (total, 32)
    assert out.numel() * 4 <= grown <= out.numel() * 4 + 512, grown
    only_u = device.normalize_batch(x, off, want_float=False, want_ubyte=True, workspace=wsp)
    assert only_u.dtype == torch.uint8 and only_u.shape == (total, 32)


@functools.lru_cache(maxsize=None)
def edge_sets():
    rng = np.random.default_rng(24)
    sets = []
    for n in EDGE:
        x = rng.integers(0, 256, (n, 16), dtype=np.uint8)
        x[:, 0], x[:, 1] = 255, 254
        x.setflags(write=False)
        sets.append(x)
    return tuple(sets)


def shortcut_table(x):
    """The float table with mean = float32(integer sum) / float32(rows): what the finish kernel's shortcut alone gives."""
    with np.errstate(all="ignore"):
        mean = x.sum(axis=0, dtype=np.int64).astype(np.float32) / np.float32(len(x))
        x0 = x.astype(np.float32) - mean
        norm = np.maximum(x0.max(axis=0), -x0.min(axis=0))
        return np.clip(np.round(x0 / norm * np.float32(128)), -128, 127)


def test_the_two_to_the_24_edge():
    """uint8 at dim 16, column 0 all 255 and column 1 all 254: 65793 rows sum to 2^24 - 1, where the integer sum is
    still numpy's chain; at 65800 and 140000 rows it is not, and the columns must be walked."""
    import torch
    from spectavi_amd import device
    sets = edge_sets()
    # on the CPU first: the shortcut alone cannot pass the last two sets, and is exact for the first
    for s, x in enumerate(sets):
        f, _, finite = numpy_tables(x)
        differs = bool(np.any((shortcut_table(x) != f)[finite]))
        assert differs == (s > 0), "set of %d rows" % len(x)
    got = run_batch(sets)
    assert_numpys(got, sets, "edge")
    single = []
    for x in sets:
        f, u = device.normalize(torch.from_numpy(x.astype(np.float32)).cuda(), want_float=True, want_ubyte=True)
        single.append((f.cpu().numpy(), u.cpu().numpy()))
    assert_same_bits(got, single, "edge")


@pytest.mark.parametrize("kind", ["float32", "uint8"])
def test_single_column(kind):
    """dim 1: one-row sets are accepted and match the single call (0 / 0); any longer set raises."""
    import torch
    from spectavi_amd import device
    x = np.arange(3, 8, dtype=kind).reshape(5, 1)
    sets = [x[0:1], x[1:1], x[1:2], x[2:3], x[3:4], x[4:5]]
    got = run_batch(sets)
    single = []
    for s in sets:
        if len(s) == 0:
            single.append((np.zeros((0, 16), np.float32), np.zeros((0, 16), np.uint8)))
            continue
        f, u = device.normalize(torch.from_numpy(s.astype(np.float32)).cuda(), want_float=True, want_ubyte=True)
        single.append((f.cpu().numpy(), u.cpu().numpy()))
    assert_same_bits(got, single, "dim 1")
    assert all(np.isnan(f[:, 0]).all() and not f[:, 1:].any() for f, _ in got)
    with pytest.raises(ValueError):
        device.normalize_batch(torch.from_numpy(x).cuda(), [0, 1, 3, 5])


def test_feeds_cascade_batch():
    """The uint8 split of three synthetic views through normalize_batch, then cascade_batch: the bits of cascade_batch
    on the torch.cat of per-view normalize calls."""
    import torch
    from spectavi_amd import device, feature
    spec = importlib.util.spec_from_file_location("multiview_from_sift_tables",
                                                  os.path.join(ROOT, "examples", "multiview_from_sift_tables.py"))
    mv = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mv)
    tables, _ = mv.synthetic_sift_views(seed=3, n_views=3, n_points=300)
    seg = _off([len(t) for t in tables])
    _, desc = device.split_sift_table(torch.from_numpy(np.concatenate(tables)).cuda())
    assert desc.dtype == torch.uint8
    rows = device.normalize_batch(desc, seg)
    loop = torch.cat([device.normalize(desc[a:b].to(torch.float32)) for a, b in zip(seg[:-1], seg[1:])])
    assert torch.equal(rows.view(torch.int32), loop.view(torch.int32))
    pairs = np.array([(1, 0), (2, 0), (2, 1)], np.int32)
    m = feature.auto_hash_bit_rate(*[max(len(t) for t in tables)] * 2)
    hd = torch.from_numpy(feature.generate_hash_dict(0x5eed, rows.shape[1], m, 2)).cuda()
    got = device.cascade_batch(rows, seg, pairs, hd, g=2)
    want = device.cascade_batch(loop, seg, pairs, hd, g=2)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    assert np.array_equal(got[2], want[2])


def test_profile_names():
    """One call ticks each of its launches once and never "normalize": three launches for uint8; a float32 table has
    no statistics launch, its minimum and maximum come from the walk."""
    import torch
    from spectavi_amd import device
    names = ("normalize_batch_stats", "normalize_batch_finish", "normalize_batch", "normalize")
    counts = {}
    device.profile_enable(True)
    try:
        for kind in ("uint8", "float32"):
            x = torch.from_numpy(np.concatenate(ragged(kind, 128))).cuda()
            device.profile_reset()
            device.normalize_batch(x, _off(SIZES))
            torch.cuda.synchronize()
            counts[kind] = [device.profile_read(k)[0] for k in names]
    finally:
        device.profile_enable(False)
        device.profile_reset()
    assert counts["uint8"] == [1, 1, 1, 0]
    assert counts["float32"] == [0, 1, 1, 0]
