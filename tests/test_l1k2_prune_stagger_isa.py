"""The half-steps of l1k2_prune_wide_kernel in the gfx950 assembly the Makefile's flags produce, with the parsers of
tests/test_l1k2_prune_isa.py: two barriers in the tile loop, the features and the raw rows of the next tile issued on
either side of the mid-tile barrier on the leading waves' path, and no barrier inside the tile's MFMA run.
No GPU is needed: the file is only compiled."""
import re

import pytest

from tests import test_l1k2_prune_isa as narrow

KERNEL = "l1k2_prune_wide_kernel"
MFMA = narrow.MFMA
LOAD = "global_load_lds_dwordx4"

asm = narrow.asm   # the module-scoped fixture: one compilation of l1k2_prune.hip for this module


@pytest.fixture(scope="module")
def loop(asm):
    """The instructions and labels of the tile loop in the order of the text: everything that lies on a cycle through
    the first MFMA in the kernel's control flow graph (reached from it and reaching it)."""
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


def _segments(loop):
    """The loop body cut at its barriers."""
    cuts = [i for i, l in enumerate(loop) if l.startswith("s_barrier")]
    return [loop[a:b] for a, b in zip([0] + cuts, cuts + [len(loop)])]


def test_two_barriers_per_tile(loop):
    assert sum(l.startswith("s_barrier") for l in loop) == 2, [l for l in loop if l.startswith("s_barrier")]


def test_the_mfma_run_has_no_barrier_inside(loop):
    mf = [i for i, l in enumerate(loop) if l.startswith(MFMA)]
    assert len(mf) == 64
    inside = [l for l in loop[mf[0]:mf[-1] + 1] if re.match(r"s_barrier|s_c?branch", l)]
    assert not inside, inside
    # and it lies in one half-step, the first: both barriers follow it
    assert all(l.startswith("s_barrier") is False for l in loop[:mf[-1]])


def test_features_and_raw_rows_are_issued_in_different_half_steps(loop):
    """Ahead of the mid-tile barrier the steady state has two ways to stage: all five loads in one run (the trailing
    waves) and a run of the four feature loads alone (the leading waves).  The leading waves' fifth, the raw rows, is
    the one load between the two barriers.  A load's base tells features (one base for four) from raw rows."""
    top, mid, _ = _segments(loop)
    mf = [i for i, l in enumerate(top) if l.startswith(MFMA)]
    ahead = top[:mf[0]]
    assert not any(l.startswith(LOAD) for l in top[mf[0]:]), "a load to LDS inside or behind the MFMA run"
    runs, cur = [], []
    for l in ahead:
        if l.startswith(LOAD):
            cur.append(l.split(",")[-1].strip())
        elif cur and re.match(r"s_c?branch|\.LBB", l):
            runs.append(cur)
            cur = []
    if cur:
        runs.append(cur)
    steady = [r for r in runs if len(r) in (4, 5)]
    shapes = sorted((len(r), len(set(r))) for r in steady)
    # the ragged tile's recomputed offsets may give each form a second copy
    assert {(4, 1), (5, 2)} == set(shapes), runs
    between = [l for l in mid if l.startswith(LOAD)]
    assert len(between) == 1, between
    lead_feat = [r for r in steady if len(r) == 4][0]
    trail = [r for r in steady if len(r) == 5][0]
    assert between[0].split(",")[-1].strip() == trail[4] != lead_feat[0] == trail[0]
