"""The register, LDS and wait budget of l1k2_prune_wide6_kernel (the FP6 form of the wide bound kernel) and its two
half-steps, read from the gfx950 assembly the Makefile's flags produce, with the `asm` fixture and the parsers of
tests/test_l1k2_prune_isa.py.  No GPU is needed: the file is only compiled."""
import re

import pytest

from tests import test_l1k2_prune_isa as narrow
from tests import test_l1k2_prune_stagger_isa as stagger

KERNEL = "l1k2_prune_wide6_kernel"
MFMA = "v_mfma_scale_f32_32x32x64_f8f6f4"

asm = narrow.asm   # the module-scoped fixture: one compilation of l1k2_prune.hip for this module


@pytest.fixture(scope="module")
def wide6(asm):
    """(metadata, body) of the FP6 kernel, through the narrow test's parsers."""
    return narrow._metadata(asm, KERNEL), narrow._body(asm, KERNEL)


def _longest_run(body):
    """narrow._longest_mfma_run for this kernel's MFMA: (first, last, count); a run ends at a branch or a barrier."""
    runs, cur = [], None
    for i, l in enumerate(body):
        if l.startswith(MFMA):
            cur = cur or [i, i, 0]
            cur[1] = i
            cur[2] += 1
        elif cur is not None and re.match(r"s_(c?branch|barrier|endpgm|setpc)", l):
            runs.append(cur)
            cur = None
    if cur is not None:
        runs.append(cur)
    assert runs, "no %s in the kernel" % MFMA
    return tuple(max(runs, key=lambda r: r[2]))


def _loop(asm):
    """The tile loop as tests/test_l1k2_prune_stagger_isa.py finds the int8 kernel's: everything that lies on a cycle through
    the first MFMA in the kernel's control flow graph, in the order of the text."""
    start = re.search(r"^_Z\w*%s\w*:" % KERNEL, asm, re.M)
    end = asm.index(".end_amdhsa_kernel", start.end())
    lines = [l.split(";")[0].strip() for l in asm[start.end():end].splitlines()]
    lines = [l for l in lines if l and (not l.startswith(".") or re.match(r"\.LBB\d+_\d+:$", l))]
    where = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    succ = []
    for i, l in enumerate(lines):
        m = re.match(r"s_c?branch\w*\s+(\.LBB\d+_\d+)$", l)
        nxt = [where[m.group(1)]] if m else []
        if not re.match(r"s_branch|s_endpgm|s_setpc", l) and i + 1 < len(lines):
            nxt.append(i + 1)
        succ.append(nxt)
    pred = [[] for _ in lines]
    for i, nxt in enumerate(succ):
        for j in nxt:
            pred[j].append(i)

    def reach(edges, root):
        seen, todo = set(), [root]
        while todo:
            for j in edges[todo.pop()]:
                if j not in seen:
                    seen.add(j)
                    todo.append(j)
        return seen
    first = next(i for i, l in enumerate(lines) if l.startswith(MFMA))
    body = sorted(reach(succ, first) & reach(pred, first))
    assert first in body, "the tile's MFMAs are in no loop"
    return [lines[i] for i in body]


def test_the_other_kernels_are_still_told_apart(asm):
    """One metadata entry each: no name matches another's entry, and the int8 kernels hold no FP6 MFMA."""
    assert narrow._metadata(asm)["group_segment_fixed_size"] <= 81920
    assert narrow._metadata(asm, stagger.KERNEL)["max_flat_workgroup_size"] == 512
    for other in (narrow.KERNEL, stagger.KERNEL):
        assert not any(l.startswith(MFMA) for l in narrow._body(asm, other)), other


def test_register_and_lds_budget(wide6):
    md, _ = wide6
    assert md["vgpr_count"] <= 256, md
    assert md["vgpr_spill_count"] == 0, md
    assert md["sgpr_spill_count"] == 0, md
    assert md["private_segment_fixed_size"] == 0, md
    assert 81920 < md["group_segment_fixed_size"] <= 163840, md    # one workgroup per CU, and it fits
    assert md["max_flat_workgroup_size"] == 512, md


def test_the_tile_is_forty_fp6_mfmas_with_no_memory_wait_among_them(wide6):
    _, body = wide6
    assert not any(l.startswith(narrow.MFMA) for l in body), "an int8 MFMA in the FP6 kernel"
    first, last, count = _longest_run(body)
    assert count == 40, "the tile's MFMA run has %d instructions, expected 40" % count
    assert sum(l.startswith(MFMA) for l in body) == 40
    run = body[first:last + 1]
    assert all("cbsz:2" in l and "blgp:2" in l for l in run if l.startswith(MFMA)), "an operand that is not FP6"
    waits = [l for l in run if l.startswith("s_waitcnt") and "vmcnt" in l]
    assert not waits, "%d vmcnt waits inside the tile's MFMA run: %s" % (len(waits), waits)
    # the A operand is read ahead through counted waits: only the last pairs wait for everything
    lgkm = [l for l in run if l.startswith("s_waitcnt") and "lgkmcnt" in l]
    assert sum("lgkmcnt(0)" in l for l in lgkm) <= 2, lgkm
    # one 16-byte and one 8-byte read per k-step; the reads of all but the first two or three of the 20 k-steps stand inside
    # the run (the compiler may put the third ahead of the first MFMA); nothing goes to scratch
    b128, b64 = (sum(l.startswith(op) for l in run) for op in ("ds_read_b128", "ds_read_b64"))
    assert b128 == b64 and b128 in (17, 18), run
    assert not any("scratch_" in l for l in body)


def test_two_barriers_per_tile_and_none_inside_the_run(asm):
    loop = _loop(asm)
    assert sum(l.startswith("s_barrier") for l in loop) == 2, [l for l in loop if l.startswith("s_barrier")]
    mf = [i for i, l in enumerate(loop) if l.startswith(MFMA)]
    assert len(mf) == 40
    inside = [l for l in loop[mf[0]:mf[-1] + 1] if re.match(r"s_barrier|s_c?branch", l)]
    assert not inside, inside
    # the run lies in the first half-step: both barriers follow it
    assert not any(l.startswith("s_barrier") for l in loop[:mf[-1]])
