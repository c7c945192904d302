"""Where l1k2_prune_wide_kernel makes a tile's thresholds and accumulators, in the gfx950 assembly the Makefile's flags
produce: at the end of the tile before, between the mid-tile barrier and the end-of-tile barrier, and no longer in the
tile's top, ahead of its MFMA run.  With the `asm` fixture of tests/test_l1k2_prune_isa.py and the loop and segment
parsing of tests/test_l1k2_prune_stagger_isa.py.  No GPU is needed: the file is only compiled.

What the compiler makes of the source, for the reader of a failure:
  * the read of the two k2s[] entries is one ds_read2_b32 of their high dwords, not a ds_read_b64 (the ds_read_b64 between
    the barriers are the drains' reads of a pair's second best); both forms are looked for in the top;
  * the 64 accumulator registers are set by 32 v_mov_b32, row half 0, and 16 v_mov_b64 that copy them to row half 1, so the
    moves are counted in registers written."""
import hashlib
import re

import pytest

from tests import test_l1k2_prune_isa as narrow
from tests import test_l1k2_prune_stagger_isa as stagger

KERNEL = stagger.KERNEL
MFMA = narrow.MFMA
# sha256 of "\n".join(narrow._register_blind(narrow._body(asm))) for l1k2_prune.hip of commit 340aded, the parent of the
# change that moved what the two kernels share into common functions, compiled with the Makefile's flags as the `asm`
# fixture does (git show 340aded:spectavi_amd/csrc/l1k2_prune.hip into a scratch copy of csrc, hipcc CXXFLAGS
# --cuda-device-only -S).  Register-blind: a change of the source that leaves the instruction stream alone may still
# let the allocator swap two register numbers.  The raw text at that commit hashed to a5d39ba7...b9b7d.
NARROW_BODY_SHA256 = "7afb1bd7784a4665677bbb9155e57bb52aa407da3ce5cdf9ccd318a5e247dd6b"

asm = narrow.asm     # the module-scoped fixture: one compilation of l1k2_prune.hip for this module
loop = stagger.loop  # the wide kernel's tile loop


def _moved_registers(lines):
    return sum(l.startswith("v_mov_b32") for l in lines) + 2 * sum(l.startswith("v_mov_b64") for l in lines)


@pytest.fixture(scope="module")
def parts(loop):
    """(the top: what stands ahead of the first MFMA in the loop's first segment; what stands between the two barriers)."""
    top, mid, _ = stagger._segments(loop)
    first = next(i for i, l in enumerate(top) if l.startswith(MFMA))
    return top[:first], mid


def test_the_top_neither_reads_k2s_nor_sets_the_accumulators(parts):
    top, _ = parts
    reads = [l for l in top if l.startswith(("ds_read_b64", "ds_read2_b32"))]
    assert not reads, reads
    moves = [l for l in top if l.startswith("v_mov_b32")]   # the ragged tile's five lane offsets, twice
    assert len(moves) < 16 and _moved_registers(top) < 16, moves


def test_the_first_a_read_waits_for_no_lds_round_trip(parts):
    """No s_waitcnt ahead of the first ds_read_b128 names lgkmcnt(0).  (The two waits that stand there are lgkmcnt(1), for
    the compiler's view of the loop's exit, which shares a block with the latch: on that path the two A reads are pending
    and their registers are written again here.  A trailing wave has one read in flight at that point, its flag, so the
    first passes at once and the second, behind the first A read, waits for the flag.)"""
    top, _ = parts
    first = next(i for i, l in enumerate(top) if l.startswith("ds_read_b128"))
    waits = [l for l in top[:first] if l.startswith("s_waitcnt") and "lgkmcnt(0)" in l]
    assert not waits, waits
    # the flag is looked at ahead of the MFMA run, under the counted waits
    assert any(l.startswith("v_readfirstlane_b32") for l in top[first:]), top[first:]


def test_the_arming_stands_between_the_two_barriers(parts):
    _, mid = parts
    assert _moved_registers(mid) >= 64, _moved_registers(mid)
    assert sum(l.startswith("v_mov_b32") for l in mid) >= 32
    assert any(l.startswith("ds_read_b64") for l in mid)
    assert any(l.startswith("ds_read2_b32") for l in mid), "the read of k2s[] is not between the barriers"
    # and the publication with it
    assert sum(l.startswith("global_atomic_umin") for l in mid) == 2, [l for l in mid if l.startswith("global_atomic")]


def test_registers(asm):
    md = narrow._metadata(asm, KERNEL)
    assert md["vgpr_count"] <= 256, md
    assert md["vgpr_spill_count"] == 0, md
    assert md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md


def test_the_narrow_kernel_is_the_parent_s(asm):
    body = narrow._body(asm)
    assert re.match(r"s_|v_", body[0]), body[0]
    blind = narrow._register_blind(body)
    assert not any(re.search(r"\b[vsa]\d", l) for l in blind), "a register operand was left in"
    assert hashlib.sha256("\n".join(blind).encode()).hexdigest() == NARROW_BODY_SHA256, len(body)
