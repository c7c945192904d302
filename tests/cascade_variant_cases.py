"""The cascade projection case table: one (dim, m, n, g) per query-side projection kernel
instantiation the default selection of spectavi_amd/csrc/cascade.hip (cascade_plan) can pick, with
that instantiation; the static sets of the forms the plan may name; and the data recipe.
Used by tests/test_cascade_variants_gpu.py (against the oracle), tests/knob_child.py and the
CPU-only checks of the library's own plan (device.cascade_plan) in tests/test_abi.py."""
import numpy as np


# (dim, m, n, g, the query-side instantiation the case targets -- project_query of device.cascade_plan)
CASES = [
    # project_kernel<MC, NT, true, G> (VALU projection, n*m > 64): two tables per pass up to MC 24
    (128, 4, 17, 3, "project_kernel<4, 2, true, 4>"),
    (128, 5, 13, 4, "project_kernel<8, 2, true, 4>"),
    (144, 8, 9, 6, "project_kernel<8, 2, true, 16>"),
    (128, 9, 8, 2, "project_kernel<12, 2, true, 4>"),
    (64, 12, 6, 7, "project_kernel<12, 2, true, 16>"),
    (128, 13, 5, 4, "project_kernel<16, 2, true, 4>"),
    (96, 16, 5, 9, "project_kernel<16, 2, true, 16>"),
    (128, 17, 4, 1, "project_kernel<20, 2, true, 4>"),
    (48, 20, 4, 12, "project_kernel<20, 2, true, 16>"),
    (128, 21, 4, 4, "project_kernel<24, 2, true, 4>"),
    (256, 24, 3, 6, "project_kernel<24, 2, true, 16>"),  # m > bucket bits: probe_refine_kernel<2, 4>
    (128, 25, 3, 2, "project_kernel<28, 1, true, 4>"),
    (80, 28, 3, 5, "project_kernel<28, 1, true, 16>"),
    (128, 29, 3, 4, "project_kernel<32, 1, true, 4>"),
    (32, 31, 3, 16, "project_kernel<32, 1, true, 16>"),
    # project_mfma_kernel<CT, true, G, FULL> (n*m <= 64 without 1..8 left-over columns, or dim % 32 != 0)
    (128, 16, 1, 2, "project_mfma_kernel<1, true, 2, true>"),
    (64, 12, 1, 4, "project_mfma_kernel<1, true, 4, true>"),
    (256, 10, 1, 7, "project_mfma_kernel<1, true, 16, true>"),
    (144, 8, 1, 1, "project_mfma_kernel<1, true, 2, false>"),
    (48, 4, 2, 3, "project_mfma_kernel<1, true, 4, false>"),
    (80, 6, 2, 6, "project_mfma_kernel<1, true, 16, false>"),
    (128, 16, 2, 2, "project_mfma_kernel<2, true, 2, true>"),
    (32, 13, 2, 3, "project_mfma_kernel<2, true, 4, true>"),
    (128, 14, 2, 8, "project_mfma_kernel<2, true, 16, true>"),
    (112, 9, 2, 1, "project_mfma_kernel<2, true, 2, false>"),
    (176, 10, 3, 4, "project_mfma_kernel<2, true, 4, false>"),
    (144, 11, 2, 11, "project_mfma_kernel<2, true, 16, false>"),
    (128, 16, 3, 1, "project_mfma_kernel<3, true, 2, true>"),
    (96, 21, 2, 4, "project_mfma_kernel<3, true, 4, true>"),
    (256, 23, 2, 9, "project_mfma_kernel<3, true, 16, true>"),
    (208, 12, 3, 2, "project_mfma_kernel<3, true, 2, false>"),
    (48, 20, 2, 3, "project_mfma_kernel<3, true, 4, false>"),
    (240, 15, 3, 6, "project_mfma_kernel<3, true, 16, false>"),
    (128, 16, 4, 2, "project_mfma_kernel<4, true, 2, true>"),
    (160, 15, 4, 4, "project_mfma_kernel<4, true, 4, true>"),
    (64, 31, 2, 5, "project_mfma_kernel<4, true, 16, true>"),
    (80, 25, 2, 0, "project_mfma_kernel<4, true, 2, false>"),
    (144, 13, 4, 3, "project_mfma_kernel<4, true, 4, false>"),
    (16, 29, 2, 16, "project_mfma_kernel<4, true, 16, false>"),
    # project_mfma4_kernel<CT, NG, true, G> (1..8 left-over columns on 4x4x1 MFMAs, dim % 32 == 0, dim <= 512)
    (128, 2, 1, 1, "project_mfma4_kernel<0, 1, true, 2>"),
    (64, 4, 1, 3, "project_mfma4_kernel<0, 1, true, 16>"),
    (64, 6, 1, 2, "project_mfma4_kernel<0, 2, true, 2>"),
    (256, 8, 1, 5, "project_mfma4_kernel<0, 2, true, 16>"),
    (128, 9, 2, 2, "project_mfma4_kernel<1, 1, true, 2>"),
    (32, 19, 1, 7, "project_mfma4_kernel<1, 1, true, 16>"),
    (128, 11, 2, 2, "project_mfma4_kernel<1, 2, true, 2>"),
    (512, 12, 2, 4, "project_mfma4_kernel<1, 2, true, 16>"),
    (128, 17, 2, 2, "project_mfma4_kernel<2, 1, true, 2>"),
    (96, 12, 3, 3, "project_mfma4_kernel<2, 1, true, 16>"),
    (192, 13, 3, 1, "project_mfma4_kernel<2, 2, true, 2>"),
    (128, 20, 2, 9, "project_mfma4_kernel<2, 2, true, 16>"),
    (64, 25, 2, 2, "project_mfma4_kernel<3, 1, true, 2>"),
    (128, 17, 3, 3, "project_mfma4_kernel<3, 1, true, 16>"),
    (256, 14, 4, 0, "project_mfma4_kernel<3, 2, true, 2>"),
    (32, 27, 2, 11, "project_mfma4_kernel<3, 2, true, 16>"),
]

# every query-side form cascade_plan can pick by default (m <= 31, g <= m, g <= 16: a G = 16 form needs
# m >= 5, so project_kernel<4, 2, true, 16> cannot be selected)
_MC_NT = [(mc, 2) for mc in (4, 8, 12, 16, 20, 24)] + [(28, 1), (32, 1)]
REACHABLE_QUERY_FORMS = (
    {"project_kernel<%d, %d, true, %d>" % (mc, nt, G) for mc, nt in _MC_NT for G in (4, 16) if (mc, G) != (4, 16)}
    | {"project_mfma_kernel<%d, true, %d, %s>" % (ct, G, f) for ct in (1, 2, 3, 4) for G in (2, 4, 16)
       for f in ("true", "false")}
    | {"project_mfma4_kernel<%d, %d, true, %d>" % (ct, ng, G) for ct in range(4) for ng in (1, 2) for G in (2, 16)})


def database_form(query_form):
    """The database-side instantiation that runs beside a query-side one: IS_QUERY false, GMAX 1."""
    name, args = query_form[:-1].split("<")
    a = args.split(", ")
    q = 1 if name == "project_mfma_kernel" else 2   # <CT, IS_QUERY, GMAX, FULL>; the others <.., .., IS_QUERY, GMAX>
    a[q:q + 2] = ["false", "1"]
    return "%s<%s>" % (name, ", ".join(a))


DATABASE_FORMS = {database_form(f) for f in REACHABLE_QUERY_FORMS}

# every probe instantiation; KNOB_PROBE_FORMS are those that only a knob reaches (SPECTAVI_CASCADE_RU=2)
KNOB_PROBE_FORMS = {"probe_refine_kernel<1, 2>"}
PROBE_FORMS = KNOB_PROBE_FORMS | (
    {"probe_table_kernel<1, 8, 7, true, true>", "probe_table_kernel<1, 8, 7, true, false>",
     "probe_table_kernel<1, 8, 7, false, false>", "probe_table_kernel<2, 4, 6, false, false>"}
    | {"probe_refine_kernel<%d, %d>" % cr for cr in ((1, 4), (2, 4), (4, 2), (8, 1), (16, 1))})


def case_id(case):
    return "%s-%dd-m%dn%dg%d" % ((case[4],) + tuple(case[:4]))


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
