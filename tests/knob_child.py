"""Child process of tests/test_knobs_gpu.py: runs a short fixed case list against the oracle under
one of the library's A/B knobs (SPECTAVI_* variables; SPECTAVI_L1K2_Q and SPECTAVI_ANN_MFMA are read once
per process, so they cannot be switched inside the pytest process).  The parent puts the knob in this process's
environment; argv[1] names the setting.  Before each case the child asks the library's plan
whether the knob took effect.  Exits 1 on the first mismatch, printing the case.

    python tests/knob_child.py <setting>"""
import ctypes as ct
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

# setting -> (the environment the parent sets, kind, cases).  Cascade cases are (dim, m, n, g); the comment
# names what the knob makes the library launch, PLAN_WANTS what the child asserts of device.cascade_plan.
SETTINGS = {
    # VALU projection for n*m <= 64: project_kernel<MC, 2, ..>, at n = 1 too (one odd pass)
    "mfma0": ({"SPECTAVI_CASCADE_MFMA": "0"}, "cascade",
              [(128, 2, 1, 1), (128, 8, 1, 2), (64, 12, 1, 5), (144, 16, 1, 3), (128, 20, 1, 6),
               (96, 24, 1, 4), (128, 17, 2, 2), (32, 6, 2, 2)]),
    # left-over columns on the 16-column MFMA tiles instead of 4x4x1: project_mfma_kernel
    "mfma4_0": ({"SPECTAVI_CASCADE_MFMA4": "0"}, "cascade",
                [(128, 9, 2, 2), (64, 6, 1, 3), (256, 11, 2, 4), (128, 17, 2, 2), (512, 13, 3, 2)]),
    # wave-per-query probe_refine_kernel<1, 4> / <2, 4> where the group kernel would run
    "group0": ({"SPECTAVI_CASCADE_GROUP": "0"}, "cascade",
               [(16, 4, 2, 2), (48, 9, 2, 3), (128, 8, 2, 2), (144, 8, 4, 3), (256, 10, 2, 4), (128, 17, 2, 2)]),
    # sorted probe with the query histogram in a kernel of its own (query_rank_kernel)
    "qhist0": ({"SPECTAVI_CASCADE_QHIST": "0", "SPECTAVI_CASCADE_SORT": "1"}, "cascade",
               [(128, 10, 2, 2), (128, 17, 2, 2), (64, 6, 1, 3), (144, 8, 4, 3), (32, 16, 2, 1)]),
    # two rows per round of the wave-per-query refine (m > bucket bits, rows <= 128 bytes): probe_refine_kernel<1, 2>
    "ru2": ({"SPECTAVI_CASCADE_RU": "2"}, "cascade", [(128, 25, 2, 3), (64, 23, 2, 2), (32, 30, 2, 5), (96, 24, 1, 4)]),
    # queries per lane forced (clamped to what the width allows), small ragged shapes
    "l1k2_q1": ({"SPECTAVI_L1K2_Q": "1"}, "l1k2", 1),
    "l1k2_q2": ({"SPECTAVI_L1K2_Q": "2"}, "l1k2", 2),
    "l1k2_q4": ({"SPECTAVI_L1K2_Q": "4"}, "l1k2", 4),
    # the 16x16x32 bf16 MFMA in the coarse stage of ann_l2: ann_coarse_kernel<16, KG>, every KG
    "ann_mfma16": ({"SPECTAVI_ANN_MFMA": "16"}, "ann", 16),
}

PLAN_WANTS = {"mfma0": {"family": 0}, "mfma4_0": {"family": 1}, "group0": {"probe_kind": 0},
              "qhist0": {"sorted": True, "qhist_fused": False}, "ru2": {"probe_kind": 0, "cpl": 1, "ru": 2}}

L1K2_DIMS = (16, 48, 64, 128, 144, 256, 400)
L1K2_YROWS = (1, 257, 1025)
ANN_SLICES = (0, 3)
ANN_LARGE_PAIRS = ((64, 64), (8, 161), (64, 256))
ANN_MODEL_NCAND = (4, 64)


def _fail(what):
    print("MISMATCH: %s" % (what,), flush=True)
    sys.exit(1)


def run_cascade(cases, wants, oracle):
    from spectavi_amd import device, feature
    from tests.cascade_variant_cases import cascade_data
    for dim, m, n, g in cases:
        x, y, d = cascade_data(dim, m, n, g, xrows=2000, yrows=700)
        plan = device.cascade_plan(len(x), len(y), dim, m, n, g)
        if any(plan[k] != v for k, v in wants.items()):
            _fail("cascade plan dim=%d m=%d n=%d g=%d: %r, the knob wants %r" % (dim, m, n, g, plan, wants))
        idx, dist, ncand = feature.nn_cascading_hash_with_dict(x, y, d, g=g, return_ncand=True)
        oidx, odist, oncand, _ = oracle.nn_cascading_hash(x, y, m, n, g, d)
        for name, a, b in (("ncand", ncand, oncand), ("dist", dist, odist), ("idx", idx, oidx)):
            if not np.array_equal(a, b):
                _fail("cascade dim=%d m=%d n=%d g=%d: %s differs" % (dim, m, n, g, name))
        print("ok cascade dim=%d m=%d n=%d g=%d" % (dim, m, n, g), flush=True)


def run_l1k2(q, oracle):
    from spectavi_amd._lib import clib, check
    for dim in L1K2_DIMS:
        for yrows in L1K2_YROWS:
            xrows = 700 + yrows % 7
            plan = (ct.c_int * 5)()
            check(clib.spv_l1k2_plan(xrows, yrows, dim, plan))
            want = min(q, 4 if plan[0] <= 64 else 2)
            if plan[1] != want:
                _fail("l1k2 plan %dx%dx%d: q=%d, SPECTAVI_L1K2_Q=%d wants %d" % (xrows, yrows, dim, plan[1], q, want))
            rng = np.random.default_rng([xrows, yrows, dim])
            hi = 3 if yrows == 257 else 256
            x = rng.integers(0, hi, (xrows, dim), dtype=np.uint8)
            y = rng.integers(0, hi, (yrows, dim), dtype=np.uint8)
            x[5] = x[xrows - 1] = y[yrows - 1]   # an exact copy in the first and the last slice
            idx = np.empty((yrows, 2), np.uint64)
            dist = np.empty((yrows, 2), np.int32)
            check(clib.spv_nn_bruteforcel1k2(x.ctypes.data, y.ctypes.data, xrows, yrows, dim,
                                             idx.ctypes.data, dist.ctypes.data))
            oidx, odist = oracle.nn_bruteforcel1k2(x, y, nthreads=oracle.max_threads())
            if not (np.array_equal(idx, oidx) and np.array_equal(dist, odist)):
                _fail("l1k2 %dx%dx%d hi=%d q=%d" % (xrows, yrows, dim, hi, plan[1]))
            print("ok l1k2 %dx%dx%d q=%d" % (xrows, yrows, dim, plan[1]), flush=True)


def run_ann(mfma):
    """The variant cases of tests/ann_cases.py on the other MFMA shape; every check asserts first that the
    plan names that shape."""
    from tests import ann_cases as ac
    try:
        for dim in ac.COARSE_CASES:
            for slices in ANN_SLICES:
                ac.check_coarse_case(dim, slices, mfma)
                print("ok ann coarse dim=%d slices=%d" % (dim, slices), flush=True)
        for dim in ac.LARGE_DIMS:
            for k, ncand in ANN_LARGE_PAIRS:
                ac.check_large_case(dim, k, ncand, mfma)
                print("ok ann large dim=%d k=%d ncand=%d" % (dim, k, ncand), flush=True)
        for ncand in ANN_MODEL_NCAND:
            print("ok " + ac.check_model_case("randn", ncand, mfma), flush=True)
    except AssertionError as e:
        _fail("ann mfma=%d: %s" % (mfma, e))


def main(setting):
    env, kind, cases = SETTINGS[setting]
    for k, v in env.items():
        if os.environ.get(k) != v:
            _fail("the parent must set %s=%s for setting %s" % (k, v, setting))
    if kind == "ann":
        run_ann(cases)
        print("all ok: %s" % setting, flush=True)
        return
    from oracle import oracle
    oracle.lib()
    if kind == "cascade":
        run_cascade(cases, PLAN_WANTS[setting], oracle)
    else:
        run_l1k2(cases, oracle)
    print("all ok: %s" % setting, flush=True)


if __name__ == "__main__":
    main(sys.argv[1])
