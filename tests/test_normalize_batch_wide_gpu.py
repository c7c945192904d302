"""normalize_batch on the GPU where tests/test_normalize_batch_gpu.py does not go: tables wider than one pass of the
256-lane grid, more work items than the launch has workgroups, and bases off the alignment the wide loads need.
The reference is numpy (feature.normalize_to_ubyte_and_multiple_16_dim on the float32 conversion of a set: the float
table always, the uint8 table where the float table is finite); device.normalize of a set alone is the second check,
bit for bit, and is itself pinned to numpy here at the widths where the batch form leans on it.

LaneGrid lays w = min(groups, 256) column groups side by side and 256 / w row lanes over them; lanes from w * (256 / w)
on are idle.  Which dim reaches which loop (uint8 collections run the statistics kernel, float32 ones have none; the
apply kernel is the same for both, and the finish kernel walks column_stats_block for every float32 set):

  dim   dim16  statistics kernel (uint8)                        apply kernel
  272   272    stats<16>, w = 17, 15 row lanes, 1 lane idle     apply<T, 4>, w = 68, 3 row lanes, 52 lanes idle
  300   304    stats<1>, two passes, the last of 44 columns     apply<T, 4>, w = 76 (one group of padding), 28 lanes idle
  301   304    stats<1>, two passes, the last of 45 columns     apply<T, 1>, two passes (g += 256), the last of 48 columns
  1040  1040   stats<16>, w = 65, 3 row lanes, 61 lanes idle    apply<T, 4>, two passes, the last of 4 groups
  2047  2048   stats<1>, eight passes, the last of 255 columns  apply<T, 1>, eight passes
  2048  2048   stats<16>, w = 128, 2 row lanes: s_part is full  apply<T, 4>, two full passes
               to its last word

  more items than the grid   cap = 32 * compute units workgroups walk b, b + cap, ...: stats<16> (two barriers per
                             item, s_part reused), apply<unsigned char, 4> at dim 128; apply<float, 4> at dim 20
  misaligned bases           uint8 base at byte 1: stats<1> and apply<unsigned char, 1> at dim 128; at byte 4: stats<1>
                             and apply<unsigned char, 4>; float32 base one element on: apply<float, 1>
"""
import functools

import numpy as np
import pytest

from tests.test_normalize_batch_gpu import _off, assert_numpys, assert_same_bits, numpy_tables, ragged, run_batch

pytestmark = pytest.mark.gpu

WIDE_SIZES = [0, 1, 2, 255, 256, 257, 600, 3]
LONG = 6  # the 600-row set: three work items
WIDE_DIMS = [272, 300, 301, 1040, 2047, 2048]
GROUPS_PER_CU = 32  # kNormalizeBatchGroupsPerCu
WALK_ROWS = [1, 2, 3, 5, 64, 257, 0, 300]  # the eight tables of the walk; 257 and 300 rows are two items each


def table(rng, kind, n, dim):
    """ragged()'s generator: random bytes, for float32 plus a random fraction so that the column sums round."""
    x = rng.integers(0, 256, (n, dim), dtype=np.uint8)
    if kind == "float32":
        x = x.astype(np.float32) + rng.random((n, dim), dtype=np.float32)
    return x


@functools.lru_cache(maxsize=None)
def wide(kind, dim):
    """The sets of a wide collection (read only): column 5 constant across all sets, the last column constant within
    the 600-row set; for float32 an inf in column 1 and a nan in column dim - 2 of the 600-row set."""
    rng = np.random.default_rng(7000 * dim + (kind == "float32"))
    sets = []
    for s, n in enumerate(WIDE_SIZES):
        x = table(rng, kind, n, dim)
        x[:, 5] = 77 if kind == "uint8" else 77.25
        if s == LONG:
            x[:, dim - 1] = 200 if kind == "uint8" else -3.5
            if kind == "float32":
                x[400, 1] = np.inf
                x[599, dim - 2] = np.nan
        x.setflags(write=False)
        sets.append(x)
    return tuple(sets)


def single_call(x):
    """device.normalize of one non-empty set -> (float table, uint8 table) on the host."""
    import torch
    from spectavi_amd import device
    f, u = device.normalize(torch.from_numpy(x.astype(np.float32)).cuda(), want_float=True, want_ubyte=True)
    return f.cpu().numpy(), u.cpu().numpy()


@pytest.mark.parametrize("dim", WIDE_DIMS)
@pytest.mark.parametrize("kind", ["float32", "uint8"])
def test_wide_tables(kind, dim):
    from spectavi_amd import device
    sets = wide(kind, dim)
    dim16 = (dim + 15) // 16 * 16
    assert dim > 256 and dim <= 2048
    plan = device.normalize_batch_plan(_off(WIDE_SIZES), dim, kind)
    assert plan["sets"] == 7 and plan["items"] == 1 + 1 + 1 + 1 + 2 + 3 + 1
    got = run_batch(sets)
    assert all(f.shape == (len(x), dim16) and u.shape == (len(x), dim16) for (f, u), x in zip(got, sets))
    assert_numpys(got, sets, "wide, dim %d" % dim)
    single = [single_call(x) if len(x) else (np.zeros((0, dim16), np.float32), np.zeros((0, dim16), np.uint8)) for x in sets]
    assert_same_bits(got, single, "wide, dim %d" % dim)
    # what the planted columns are there for, at the far end of the last pass too
    f = got[LONG][0]
    assert np.isnan(f[:, 5]).all() and np.isnan(f[:, dim - 1]).all() and np.isfinite(f[:, 0]).all()
    assert np.isfinite(f[:, 257]).all() and not f[:, dim:].any()
    if kind == "float32":
        assert np.isnan(f[:, 1]).all() and np.isnan(f[:, dim - 2]).all()


@pytest.mark.parametrize("dim", [272, 301, 2048])
def test_the_single_call_at_the_same_widths(dim):
    """device.normalize on float32 [600, dim] against numpy: column_stats_block over 17, 19 and 128 column blocks (the
    last one of 13 columns at dim 301) and adapter.hip's apply kernel, which the batch form is compared with above."""
    x = wide("float32", dim)[LONG]
    assert x.shape == (600, dim) and x.dtype == np.float32
    assert_numpys([single_call(x)], [x], "single call, dim %d" % dim)


def _walk_collection(kind, dim, nsets):
    """nsets sets, set s a copy of table s % 8 -> (the eight tables, their numpy results, the sets back to back)."""
    rng = np.random.default_rng(900 + dim + (kind == "float32"))
    tables = [table(rng, kind, n, dim) for n in WALK_ROWS]
    period = np.concatenate(tables)
    whole, rest = divmod(nsets, 8)
    x = np.concatenate([np.tile(period, (whole, 1))] + tables[:rest])
    return tables, [numpy_tables(t) if len(t) else None for t in tables], x


@pytest.mark.parametrize("kind,dim", [("uint8", 128), ("float32", 20)])
def test_more_items_than_the_grid(kind, dim):
    """cap + 300 sets: every workgroup of the statistics (uint8) and apply kernels walks a second item, a good many a
    third.  Neighbouring items belong to tables of other sizes, so a word of s_part left from the item before, or an
    item taken at the wrong stride, gives another table's numbers."""
    import torch
    from spectavi_amd import device
    cap = GROUPS_PER_CU * torch.cuda.get_device_properties(0).multi_processor_count
    nsets = cap + 300
    sizes = [WALK_ROWS[s % 8] for s in range(nsets)]
    off = _off(sizes)
    plan = device.normalize_batch_plan(off, dim, kind)
    assert plan["items"] > cap and plan["items"] == sum(-(-n // 256) for n in sizes)
    assert int(off[-1]) <= 1100000
    tables, want, x = _walk_collection(kind, dim, nsets)
    assert len(x) == off[-1]
    f, u = device.normalize_batch(torch.from_numpy(x).cuda(), off, want_float=True, want_ubyte=True)
    f, u = f.cpu().numpy(), u.cpu().numpy()
    dim16 = (dim + 15) // 16 * 16
    assert f.shape == u.shape == (len(x), dim16)
    # all sets of one table at once: their rows, [copies, rows of the table, dim16]
    first = _off(WALK_ROWS)
    for k, n in enumerate(WALK_ROWS):
        if n == 0:
            continue
        starts = off[k:-1:8]
        rows = (starts[:, None] + np.arange(n)[None, :]).reshape(-1)
        assert len(starts) == len(range(k, nsets, 8)) and (np.diff(off)[k::8] == n).all() and first[k + 1] - first[k] == n
        wf, wu, finite = want[k]
        gf, gu = f[rows].reshape(len(starts), n, dim16), u[rows].reshape(len(starts), n, dim16)
        bad = ~((gf == wf[None]) | (np.isnan(gf) & np.isnan(wf[None]))).all(axis=(1, 2))
        assert not bad.any(), "float table of set %d (table %d, %d rows) against numpy" % (k + 8 * np.flatnonzero(bad)[0], k, n)
        bad = ~((gu == wu[None]) | ~finite[None]).all(axis=(1, 2))
        assert not bad.any(), "uint8 table of set %d (table %d, %d rows) against numpy" % (k + 8 * np.flatnonzero(bad)[0], k, n)
    # the single call on each table: the float bits, NaN payloads included, of the first and the last copy
    for k, n in enumerate(WALK_ROWS):
        if n == 0:
            continue
        sf, su = single_call(tables[k])
        for s in (k, k + 8 * ((nsets - 1 - k) // 8)):
            a, b = int(off[s]), int(off[s + 1])
            assert np.array_equal(f[a:b].view(np.int32), sf.view(np.int32)) and np.array_equal(u[a:b], su), "set %d" % s


def _at_offset(flat, elems, total, dim):
    """rows [total, dim] of the flat device buffer starting `elems` elements in."""
    return flat[elems:elems + total * dim].view(total, dim)


@pytest.mark.parametrize("kind,elems,base_mod_16", [("uint8", 1, 1), ("uint8", 4, 4), ("float32", 1, 4)])
def test_misaligned_bases(kind, elems, base_mod_16):
    """The ragged collection at dim 128 read from a base off 16 bytes: the statistics kernel falls back to single
    bytes, and where the base is off four elements too the apply kernel to single elements.  The outputs are the
    aligned call's bits, which tests/test_normalize_batch_gpu.py compares with numpy and the single call."""
    import torch
    from spectavi_amd import device
    sets = ragged(kind, 128)
    off = _off([len(x) for x in sets])
    total = int(off[-1])
    host = np.concatenate(sets)
    aligned = torch.from_numpy(host).cuda()
    flat = torch.zeros(total * 128 + 64, dtype=aligned.dtype, device="cuda")
    x = _at_offset(flat, elems, total, 128)
    x.copy_(aligned)
    assert aligned.data_ptr() % 16 == 0 and x.data_ptr() % 16 == base_mod_16 and x.is_contiguous()
    assert np.array_equal(x.cpu().numpy(), host, equal_nan=True)
    want = device.normalize_batch(aligned, off, want_float=True, want_ubyte=True)
    got = device.normalize_batch(x, off, want_float=True, want_ubyte=True)
    assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32)), "the float table"
    assert torch.equal(got[1], want[1]), "the uint8 table"
    f, u = got[0].cpu().numpy(), got[1].cpu().numpy()
    assert_numpys([(f[a:b], u[a:b]) for a, b in zip(off[:-1], off[1:])], sets, "base %d elements on" % elems)
    assert not flat[:elems].any() and not flat[elems + total * 128:].any(), "the input's neighbours are not written"
