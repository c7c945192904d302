"""ann_l2 on the kernels and buffer sizes that tests/test_ann_gpu.py never launches.  Every expected value
comes from tests/bruteforce_oracle.py, from the float64 model of tests/ann_coarse_model.py with its derived
bound, or from the library's plan (only to say which kernel runs); none from the kernel's own output.

  1. a case table that reaches every ann_coarse_kernel<SHAPE, KG> and both ann_rerank_kernel<PER>: the
     Mfma<32> half here, the Mfma<16> half in a child process (tests/knob_child.py, "ann_mfma16");
  2. ncand and k up to their limits on the exact domain: every survivor buffer length, wave_select<6>,
     ann_rerank_kernel<4>, a large keep;
  3. the coarse stage off the exact domain against the float64 model;
  4. the corner of the exact domain: sums of products just under 2^24;
  5. the re-rank's scalar loop for rows that are not 16-byte aligned.

The two table tests need no GPU; the others are marked gpu one by one."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ann_cases as ac

gpu = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# what ann_run can launch for the coarse stage and the re-rank (spectavi_amd/csrc/ann.hip)
COARSE_INSTANTIATED = {"ann_coarse_kernel<%d, %d>" % (shape, kg) for shape in (16, 32) for kg in range(5)}
RERANK_INSTANTIATED = {"ann_rerank_kernel<1>", "ann_rerank_kernel<4>"}


def plan(xrows, yrows, dim, k, ncand=0, slices=0):
    from spectavi_amd import device
    return device.ann_l2_plan(xrows, yrows, dim, k, ncand, slices)


# ---- 1. the case table ------------------------------------------------------------------------------
def test_case_table_reaches_every_instantiation():
    coarse = {"ann_coarse_kernel<%d, %d>" % (shape, ac.coarse_kg(plan(1000, 150, dim, ac.EDGE_K, ac.EDGE_K)["kpad"]))
              for shape in ac.COARSE_SHAPES for dim in ac.COARSE_CASES}
    assert coarse == COARSE_INSTANTIATED
    assert [ac.coarse_kg(plan(1000, 150, dim, ac.EDGE_K, ac.EDGE_K)["kpad"]) for dim in ac.COARSE_CASES] == [1, 2, 3, 3, 4, 0]
    rerank = {"ann_rerank_kernel<%d>" % ac.rerank_per(plan(1500, 150, 33, 8, ncand)["ncand"]) for ncand in ac.RERANK_CASES}
    assert rerank == RERANK_INSTANTIATED
    # the large pairs sit on both sides of every buffer step and of the re-rank's
    assert sorted({plan(1500, 150, 33, k, n)["buflen"] for k, n in ac.LARGE_PAIRS}) == [128, 192, 256, 320, 384]
    assert {ac.rerank_per(n) for _, n in ac.LARGE_PAIRS} == {1, 4}
    from tests.knob_child import SETTINGS
    assert SETTINGS["ann_mfma16"][0] == {"SPECTAVI_ANN_MFMA": "16"} and 16 in ac.COARSE_SHAPES


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "ann.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert {k for k in listed if k.startswith("ann_coarse_kernel")} == COARSE_INSTANTIATED, out
    assert {k for k in listed if k.startswith("ann_rerank_kernel")} == RERANK_INSTANTIATED, out


@gpu
@pytest.mark.parametrize("slices", ac.COARSE_SLICES)
@pytest.mark.parametrize("dim", ac.COARSE_CASES)
def test_coarse_widths(dim, slices):
    """1000 x 150 at ncand = k = 8 under the default shape, bit-equal to the oracle."""
    ac.check_coarse_case(dim, slices, 32)


# ---- 2. large ncand and k on the exact domain ----------------------------------------------------------
@gpu
@pytest.mark.parametrize("k,ncand", ac.LARGE_PAIRS)
@pytest.mark.parametrize("dim", ac.LARGE_DIMS)
def test_large_ncand_and_k(dim, k, ncand):
    """1500 x 150, values in [0, 15], bit-equal to the oracle with the plan's slices and with 7 forced
    ones.  At k = ncand the result is the whole candidate set, so every compaction decision shows.  For
    ncand > 64 only the best 64 of the candidates show (k <= 64), so a key lost beyond them passes here;
    test_coarse_model (k = ncand up to 64) and test_coarse_widths carry the rest."""
    ac.check_large_case(dim, k, ncand, 32)


# ---- 3. off the exact domain: the float64 model ------------------------------------------------------------
@gpu
@pytest.mark.parametrize("ncand", ac.MODEL_NCAND)
@pytest.mark.parametrize("name", ac.MODEL_SETS)
def test_coarse_model(name, ncand):
    """The candidate set at k = ncand holds every row the model says it must and none it must not, for
    every query, with the plan's slices and with 3 forced ones."""
    print(ac.check_model_case(name, ncand, 32))


# ---- 4. the window corner of the exact domain ----------------------------------------------------------------
@gpu
@pytest.mark.parametrize("a", ac.WINDOW_BASES)
@pytest.mark.parametrize("dim", ac.WINDOW_DIMS)
def test_window_corner(dim, a):
    x, y, (oi, od) = ac.window_case(dim, a)
    for k in ac.WINDOW_K:
        ac.assert_bits(ac.device_run(x, y, k, k), (oi[:, :k], od[:, :k]), "window dim=%d a=%d k=%d" % (dim, a, k))


# ---- 5. rows that are not 16-byte aligned ------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("xrows,ncand", [(40, 64), (1000, 8)])
def test_unaligned_rows(xrows, ncand):
    """x and y as contiguous views one element into their allocations: 4-byte but not 16-byte aligned, so
    the re-rank takes its scalar loop although dim % 4 == 0.  40 rows at ncand = 64: every row is a
    candidate and no coarse stage runs; 1000 rows: the whole chain."""
    import torch
    from spectavi_amd import device
    dim, k = 64, 8
    x, y = ac.edge_rows(xrows, 70, dim)
    assert (xrows <= plan(xrows, 70, dim, k, ncand)["ncand"]) == (xrows == 40)
    want = ac.bo.nn_bruteforce(x, y, 2.0, k)
    views = []
    for a in (x, y):
        flat = torch.zeros(a.size + 8, dtype=torch.float32, device="cuda")
        v = flat[1:1 + a.size].view(a.shape)
        v.copy_(torch.from_numpy(a))
        assert v.is_contiguous() and v.data_ptr() % 16 == 4
        views.append(v)
    i, d = device.ann_l2(views[0], views[1], k=k, ncand=ncand)
    torch.cuda.synchronize()
    got = i.cpu().numpy().view(np.uint64), d.cpu().numpy()
    ac.assert_bits(got, ac.device_run(x, y, k, ncand), "unaligned against aligned, xrows=%d" % xrows)
    ac.assert_bits(got, want, "unaligned against the oracle, xrows=%d" % xrows)
