"""What the direct-to-LDS staging of l1k2_prune_kernel must look like in the gfx950 assembly, beside the
budget of tests/test_l1k2_prune_isa.py.  No GPU is needed: the file is only compiled.

The loads are an asm statement because the compiler, once it knows of a load to LDS in flight, waits for
vmcnt(0) ahead of the tile's first A-operand read (right behind the loads of the next tile), and replaces the
counted lgkmcnt waits between the MFMA pairs by lgkmcnt(0).  Either would pass the budget test and cost
more than the staging saves; this file keeps them from coming back unnoticed."""
import re

from tests.test_l1k2_prune_isa import _body, _longest_mfma_run, asm  # noqa: F401  (asm is the module's fixture)

DMA = "global_load_lds_dwordx4"


def _tile_run(body):
    """(index of the first, index of the last) MFMA of the tile's run of 32."""
    first, last, count = _longest_mfma_run(body)
    assert count == 32, count
    return first, last


def test_tiles_are_loaded_straight_into_lds(asm):
    body = _body(asm)
    dma = [i for i, l in enumerate(body) if l.startswith(DMA)]
    # four wave-instructions of 1 KiB for the 16 KiB feature tile of a workgroup of four waves and one for the
    # 4 KiB of raw rows, before the loop and in it
    assert len(dma) == 10, len(dma)
    first, _ = _tile_run(body)
    in_loop = [i for i in dma if i < first][-5:]
    assert len(in_loop) == 5
    waits = [l for l in body[in_loop[-1]:first] if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert not waits, "the tile waits for the next tile's loads before its own MFMAs: %s" % waits


def test_a_operand_waits_stay_counted(asm):
    body = _body(asm)
    first, last = _tile_run(body)
    waits = [l for l in body[first:last + 1] if l.startswith("s_waitcnt")]
    counted = [l for l in waits if re.search(r"lgkmcnt\([1-9]", l)]
    assert len(counted) >= 12, waits
