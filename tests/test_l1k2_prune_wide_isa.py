"""The register, LDS and wait budget of l1k2_prune_wide_kernel (512 threads, one workgroup per CU, 64-row tiles),
read from the gfx950 assembly the Makefile's flags produce, with the parsing of tests/test_l1k2_prune_isa.py.
No GPU is needed: the file is only compiled."""
import pytest

from tests import test_l1k2_prune_isa as narrow

KERNEL = "l1k2_prune_wide_kernel"
MFMA = narrow.MFMA

asm = narrow.asm   # the module-scoped fixture: one compilation of l1k2_prune.hip for this module


@pytest.fixture(scope="module")
def wide(asm):
    """(metadata, body) of the wide kernel, through the narrow test's parsers."""
    return narrow._metadata(asm, KERNEL), narrow._body(asm, KERNEL)


def test_the_narrow_kernel_is_still_told_apart(asm):
    """One metadata entry each: neither name matches the other's entry."""
    assert KERNEL not in narrow.KERNEL and narrow.KERNEL not in KERNEL
    assert narrow._metadata(asm)["group_segment_fixed_size"] <= 81920


def test_register_and_lds_budget(wide):
    md, _ = wide
    assert md["vgpr_count"] <= 256, md
    assert md["vgpr_spill_count"] == 0, md
    assert md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert 81920 < md["group_segment_fixed_size"] <= 163840, md    # one workgroup per CU, and it fits
    assert md["max_flat_workgroup_size"] == 512, md


def test_no_vector_memory_wait_inside_a_tiles_mfmas(wide):
    """The longest run of MFMAs is the 64 of a tile, and no s_waitcnt between its first and its last names vmcnt."""
    _, body = wide
    first, last, count = narrow._longest_mfma_run(body)
    assert count == 64, "the tile's MFMA run has %d instructions, expected 64" % count
    waits = [l for l in body[first:last + 1] if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert not waits, "%d vmcnt waits inside the tile's MFMA run: %s" % (len(waits), waits)
    # the A operand is read ahead through counted waits: only the last pairs wait for everything
    lgkm = [l for l in body[first:last + 1] if l.startswith("s_waitcnt") and "lgkmcnt" in l]
    assert sum("lgkmcnt(0)" in l for l in lgkm) <= 2, lgkm
