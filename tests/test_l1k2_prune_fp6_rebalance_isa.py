"""Where l1k2_prune_wide6_kernel (the FP6 form of the wide bound kernel) makes a tile's thresholds and accumulators, in the
gfx950 assembly the Makefile's flags produce: in the tile's own top, behind its first A read and ahead of its first MFMA,
and no longer between the two barriers, at the end of the compare of the tile before, where the int8 form keeps them
(tests/test_l1k2_prune_arm_isa.py).  With the `asm` fixture of tests/test_l1k2_prune_isa.py, the loop of
tests/test_l1k2_prune_fp6_isa.py and the segments of tests/test_l1k2_prune_stagger_isa.py.  No GPU is needed: the file is
only compiled.  The budgets and the 40-MFMA run stay with tests/test_l1k2_prune_fp6_isa.py.

Of the levers the change was to try, this one shipped; the flag test behind the sign fold and the leading waves staging the
whole tile did not ("FP6: arming back in M"), and nothing is asserted of them.

What the compiler makes of the source, for the reader of a failure: the two k2s[] entries are read by one ds_read2_b32 of their
high dwords, and the 64 accumulator registers are set by v_mov_b32 and v_mov_b64, counted in registers written."""
import pytest

from tests import test_l1k2_prune_arm_isa as arm
from tests import test_l1k2_prune_fp6_isa as fp6
from tests import test_l1k2_prune_isa as narrow
from tests import test_l1k2_prune_stagger_isa as stagger

KERNEL = fp6.KERNEL
MFMA = fp6.MFMA

asm = narrow.asm   # the module-scoped fixture: one compilation of l1k2_prune.hip for this module


@pytest.fixture(scope="module")
def parts(asm):
    """(the top: what stands ahead of the first MFMA in the loop's first segment; what stands between the two barriers)."""
    top, mid, _ = stagger._segments(fp6._loop(asm))
    first = next(i for i, l in enumerate(top) if l.startswith(MFMA))
    return top[:first], mid


def _longest_move_run(lines):
    """Registers written by the longest run of consecutive moves."""
    best = cur = 0
    for l in lines:
        cur = cur + (1 if l.startswith("v_mov_b32") else 2) if l.startswith(("v_mov_b32", "v_mov_b64")) else 0
        best = max(best, cur)
    return best


def test_no_run_of_accumulator_moves_between_the_barriers(parts):
    _, mid = parts
    assert _longest_move_run(mid) < 8, _longest_move_run(mid)
    # nor the refresh: the read of k2s[] and the publication went with the moves
    assert not any(l.startswith("ds_read2_b32") for l in mid)
    assert not any(l.startswith("global_atomic_umin") for l in mid), [l for l in mid if l.startswith("global_atomic")]


def test_the_arming_stands_in_the_top_behind_the_first_a_read(parts):
    top, _ = parts
    first_read = next(i for i, l in enumerate(top) if l.startswith("ds_read_b128"))
    behind = top[first_read:]
    assert arm._moved_registers(behind) >= 64, arm._moved_registers(behind)
    assert _longest_move_run(behind) >= 32, _longest_move_run(behind)
    assert arm._moved_registers(top[:first_read]) < 16
    assert sum(l.startswith("ds_read2_b32") for l in behind) == 1, "the read of k2s[] is not in the top"
    assert sum(l.startswith("global_atomic_umin") for l in behind) == 2, [l for l in top if l.startswith("global_atomic")]
    # the trailing waves' look at the flag, and their way out, stand ahead of the arming
    flag = next(i for i, l in enumerate(behind) if l.startswith("v_readfirstlane_b32"))
    k2s = next(i for i, l in enumerate(behind) if l.startswith("ds_read2_b32"))
    assert flag < k2s and any(l.startswith("s_cbranch") for l in behind[flag:k2s]), behind[flag:k2s]
    # the threshold loads for the next tile write seen[] again: they stand behind the refresh that reads it
    loads = [i for i, l in enumerate(behind) if l.startswith("global_load_dword ")]
    assert len(loads) == 2 and min(loads) > k2s, loads


def test_registers(asm):
    md = narrow._metadata(asm, KERNEL)
    assert md["vgpr_count"] <= 256, md
    assert md["vgpr_spill_count"] == 0, md
    assert md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert not any("scratch_" in l for l in narrow._body(asm, KERNEL))
