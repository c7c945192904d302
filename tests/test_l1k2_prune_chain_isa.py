"""The top of a tile of l1k2_prune_kernel in the gfx950 assembly, beside tests/test_l1k2_prune_isa.py and
tests/test_l1k2_prune_staging_isa.py.  No GPU is needed: the file is only compiled.

What a wave does between the head of the tile loop and the first MFMA of the tile is a dependent chain that the
matrix pipe waits for.  The stage loads take their addresses from a scalar base (advanced once per tile by the
scalar unit) plus a tile-invariant lane offset, instead of five 64-bit per-lane addresses rebuilt every tile, and
that is held here: the scalar-base form of the five loads, and fewer vector instructions at the tile's top than
the kernel had before (counted with the same function on the assembly of that commit)."""
import re

from tests.test_l1k2_prune_isa import KERNEL, _longest_mfma_run, asm  # noqa: F401  (asm is the module's fixture)

DMA = "global_load_lds_dwordx4"
# vector instructions, MFMAs aside, between the loop head and the tile's first MFMA in the assembly of commit
# e3f58af (the Makefile's flags, ROCm 7.2), counted by tile_top() below
PARENT_TOP_VALU = 40


def kernel_lines(asm):
    """The kernel's lines with labels kept (as 'NAME:'), comments and directives dropped."""
    start = re.search(r"^_Z\w*%s\w*:" % KERNEL, asm, re.M)
    end = asm.index(".end_amdhsa_kernel", start.end())
    lines = [l.split(";")[0].strip() for l in asm[start.end():end].splitlines()]
    return [l for l in lines if l and (not l.startswith(".") or re.match(r"\.LBB\d+_\d+:", l))]


def tile_top(lines):
    """(index of the loop head's label, index of the first MFMA of the tile's run of 32).  The loop head is the
    first label between the barrier ahead of the loop and the loop's five stage loads that a branch behind the
    run jumps back to (a later one is where a block that was laid out behind the loop comes back in)."""
    first_mfma, last_mfma, count = _longest_mfma_run(lines)
    assert count == 32, count
    run = [first_mfma, last_mfma]
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    dma = [i for i, l in enumerate(lines) if l.startswith(DMA) and i < run[0]][-5:]
    back = [labels[m.group(1)] for l in lines[run[-1]:] for m in [re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)", l)]
            if m and labels[m.group(1)] < dma[0]]
    barrier = max(i for i, l in enumerate(lines[:dma[0]]) if l.startswith("s_barrier"))
    back = [i for i in back if i > barrier]
    assert back, "no branch behind the MFMA run jumps back ahead of the stage loads"
    return min(back), run[0]


def test_stage_loads_take_a_scalar_base(asm):
    lines = kernel_lines(asm)
    head, first = tile_top(lines)
    dma = [l for l in lines[head:first] if l.startswith(DMA)]
    assert len(dma) == 5, dma
    for l in dma:
        assert re.match(r"%s\s+v\d+,\s*s\[\d+:\d+\]" % DMA, l), l


def test_fewer_vector_instructions_at_the_tiles_top(asm):
    lines = kernel_lines(asm)
    head, first = tile_top(lines)
    valu = [l for l in lines[head:first] if l.startswith("v_") and not l.startswith("v_mfma")]
    print("vector instructions between the loop head and the first MFMA: %d (parent %d)" % (len(valu), PARENT_TOP_VALU))
    assert len(valu) < PARENT_TOP_VALU, (len(valu), valu)
