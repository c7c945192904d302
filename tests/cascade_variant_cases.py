"""The cascade projection case table: one (dim, m, n, g) per query-side projection kernel
instantiation the default selection of spectavi_amd/csrc/cascade.hip can pick, and the data recipe.
Used by tests/test_cascade_variants_gpu.py (against the oracle), tests/knob_child.py and the
CPU-only table check in tests/test_abi.py."""
import numpy as np


def projection_kernels(dim, m, n, g):
    """The (database, query) projection instantiations the default selection launches for this
    case: a restatement of cascade_run -> launch_project_mfma / launch_project, used for the test ids
    and to check that the table below reaches each of them (tools/kernel_coverage.py checks the same
    against a kernel trace)."""
    nm = n * m
    if nm <= 64:
        full = dim % 32 == 0
        ctm, left = nm // 16, nm % 16
        if full and dim <= 512 and 1 <= left <= 8:
            ng = (left + 3) // 4
            gq = 2 if g <= 2 else 16
            return ("project_mfma4_kernel<%d, %d, false, 1>" % (ctm, ng),
                    "project_mfma4_kernel<%d, %d, true, %d>" % (ctm, ng, gq))
        ct = min((nm + 15) // 16, 4)
        gq = 2 if g <= 2 else 4 if g <= 4 else 16
        f = "true" if full else "false"
        return ("project_mfma_kernel<%d, false, 1, %s>" % (ct, f), "project_mfma_kernel<%d, true, %d, %s>" % (ct, gq, f))
    mc = min((m + 3) // 4 * 4, 32)
    nt = 2 if n >= 2 and mc <= 24 else 1
    gq = 4 if g <= 4 else 16
    return ("project_kernel<%d, %d, false, 1>" % (mc, nt), "project_kernel<%d, %d, true, %d>" % (mc, nt, gq))


# (dim, m, n, g); the comment names the query-side instantiation the case targets
CASES = [
    # project_kernel<MC, NT, true, G> (VALU projection, n*m > 64): two tables per pass up to MC 24
    (128, 4, 17, 3),     # <4, 2, true, 4>
    (128, 5, 13, 4),     # <8, 2, true, 4>
    (144, 8, 9, 6),      # <8, 2, true, 16>
    (128, 9, 8, 2),      # <12, 2, true, 4>
    (64, 12, 6, 7),      # <12, 2, true, 16>
    (128, 13, 5, 4),     # <16, 2, true, 4>
    (96, 16, 5, 9),      # <16, 2, true, 16>
    (128, 17, 4, 1),     # <20, 2, true, 4>
    (48, 20, 4, 12),     # <20, 2, true, 16>
    (128, 21, 4, 4),     # <24, 2, true, 4>
    (256, 24, 3, 6),     # <24, 2, true, 16>  (m > bucket bits: probe_refine_kernel<2, 4>)
    (128, 25, 3, 2),     # <28, 1, true, 4>
    (80, 28, 3, 5),      # <28, 1, true, 16>
    (128, 29, 3, 4),     # <32, 1, true, 4>
    (32, 31, 3, 16),     # <32, 1, true, 16>
    # project_mfma_kernel<CT, true, G, FULL> (n*m <= 64 without 1..8 left-over columns, or dim % 32 != 0)
    (128, 16, 1, 2),     # <1, true, 2, true>
    (64, 12, 1, 4),      # <1, true, 4, true>
    (256, 10, 1, 7),     # <1, true, 16, true>
    (144, 8, 1, 1),      # <1, true, 2, false>
    (48, 4, 2, 3),       # <1, true, 4, false>
    (80, 6, 2, 6),       # <1, true, 16, false>
    (128, 16, 2, 2),     # <2, true, 2, true>
    (32, 13, 2, 3),      # <2, true, 4, true>
    (128, 14, 2, 8),     # <2, true, 16, true>
    (112, 9, 2, 1),      # <2, true, 2, false>
    (176, 10, 3, 4),     # <2, true, 4, false>
    (144, 11, 2, 11),    # <2, true, 16, false>
    (128, 16, 3, 1),     # <3, true, 2, true>
    (96, 21, 2, 4),      # <3, true, 4, true>
    (256, 23, 2, 9),     # <3, true, 16, true>
    (208, 12, 3, 2),     # <3, true, 2, false>
    (48, 20, 2, 3),      # <3, true, 4, false>
    (240, 15, 3, 6),     # <3, true, 16, false>
    (128, 16, 4, 2),     # <4, true, 2, true>
    (160, 15, 4, 4),     # <4, true, 4, true>
    (64, 31, 2, 5),      # <4, true, 16, true>
    (80, 25, 2, 0),      # <4, true, 2, false>
    (144, 13, 4, 3),     # <4, true, 4, false>
    (16, 29, 2, 16),     # <4, true, 16, false>
    # project_mfma4_kernel<CT, NG, true, G> (1..8 left-over columns on 4x4x1 MFMAs, dim % 32 == 0, dim <= 512)
    (128, 2, 1, 1),      # <0, 1, true, 2>
    (64, 4, 1, 3),       # <0, 1, true, 16>
    (64, 6, 1, 2),       # <0, 2, true, 2>
    (256, 8, 1, 5),      # <0, 2, true, 16>
    (128, 9, 2, 2),      # <1, 1, true, 2>
    (32, 19, 1, 7),      # <1, 1, true, 16>
    (128, 11, 2, 2),     # <1, 2, true, 2>
    (512, 12, 2, 4),     # <1, 2, true, 16>
    (128, 17, 2, 2),     # <2, 1, true, 2>
    (96, 12, 3, 3),      # <2, 1, true, 16>
    (192, 13, 3, 1),     # <2, 2, true, 2>
    (128, 20, 2, 9),     # <2, 2, true, 16>
    (64, 25, 2, 2),      # <3, 1, true, 2>
    (128, 17, 3, 3),     # <3, 1, true, 16>
    (256, 14, 4, 0),     # <3, 2, true, 2>
    (32, 27, 2, 11),     # <3, 2, true, 16>
]

# every query-side form launch_project / launch_project_mfma can pick by default (m <= 31, g <= m,
# g <= 16: a G = 16 form needs m >= 5, so project_kernel<4, 2, true, 16> cannot be selected)
_MC_NT = [(mc, 2) for mc in (4, 8, 12, 16, 20, 24)] + [(28, 1), (32, 1)]
REACHABLE_QUERY_FORMS = (
    {"project_kernel<%d, %d, true, %d>" % (mc, nt, G) for mc, nt in _MC_NT for G in (4, 16) if (mc, G) != (4, 16)}
    | {"project_mfma_kernel<%d, true, %d, %s>" % (ct, G, f) for ct in (1, 2, 3, 4) for G in (2, 4, 16)
       for f in ("true", "false")}
    | {"project_mfma4_kernel<%d, %d, true, %d>" % (ct, ng, G) for ct in range(4) for ng in (1, 2) for G in (2, 16)})


def cascade_data(dim, m, n, g, xrows=3000, yrows=1100):
    """test_left_over_hyperplane_columns' recipe -- planted near-copies, non-integer rows on both
    sides -- plus every third hyperplane column rounded to integers and some all-zero rows, so that
    projections tie in magnitude or are exactly zero."""
    rng = np.random.default_rng([dim, m, n, g, 7])
    x = rng.integers(-128, 128, (xrows, dim)).astype(np.float32)
    y = rng.integers(-128, 128, (yrows, dim)).astype(np.float32)
    y[:500] = np.clip(x[rng.integers(0, xrows, 500)] + rng.integers(-2, 3, (500, dim)), -128, 127)
    x[100:200] += rng.uniform(-0.49, 0.49, (100, dim)).astype(np.float32)
    y[600:700] += rng.uniform(-0.49, 0.49, (100, dim)).astype(np.float32)
    x[::97] = 0.0
    y[3::89] = 0.0
    d = rng.standard_normal((n, dim, m)).astype(np.float32)
    d[:, :, ::3] = np.round(d[:, :, ::3])
    return x, y, d
