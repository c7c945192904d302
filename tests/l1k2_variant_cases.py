"""The L1 2-NN case table: one or more shapes per kernel instantiation of l1k2.hip, each chosen so
that the library's own plan (spv_l1k2_plan) selects that instantiation, and the data recipe that
puts every case on the edges where a multi-query kernel goes wrong.

Used by tests/test_l1k2_variants_gpu.py (the cases against the oracle) and by the CPU-only
coverage check in tests/test_abi.py (the plans of the cases against the instantiated set)."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# The instantiations l1k2_run launches (spectavi_amd/csrc/l1k2.hip), all named by l1k2_plan: the
# row width is one of the table `TileWidths`, launch_tile_q picks Q in {1, 2, 4} for D4 <= 16 and
# {1, 2} above (dim_pad = 4 * D4, max_q_for); widths above 256 go to l1k2_wide_kernel<1> / <2>; the
# merge kernel takes the plan's merge_lanes: 1 lane per query for <= 4 slices, 8 for <= 32, 64 beyond
# (merge_form below restates it: spv_l1k2_plan does not report it).  As (dim_pad, q, wide) and merge forms:
TILE_WIDTHS = (32, 48, 64, 80, 96, 112, 128, 144, 160, 192, 256)
INSTANTIATED = ({(w, q, False) for w in TILE_WIDTHS for q in ((1, 2, 4) if w <= 64 else (1, 2))}
                | {("wide", 1, True), ("wide", 2, True)})
MERGE_FORMS = {1, 8, 64}

# Database rows: 16384 + 37 and 65536 + 27 keep the plan's slice count at 256 / 1024 (so Q > 1 is
# chosen) while the last 64-row slice is ragged.  Query rows 1024k + 1 (Q = 4), 512k + 1 (Q = 2):
# the last query block holds a single live query, in lane group q = 0 (the min(qi, N - 1) clamp of
# the other lane groups and the guarded store).
XQ2, XQ4 = 16384 + 37, 65536 + 27

# (xrows, yrows, dim, hi, kind, target): values uniform in [0, hi) ("sift": real descriptors, see
# make_case); target = (dim_pad or "wide", q) the plan must pick.  dims 16, 176, 208, 240 are padded
# by pad_rows_kernel to the next instantiated width.
CASES = [
    # Q = 1 at every width, and the three merge forms (4 / 16 / 47 slices)
    (200, 77, 16, 3, "uniform", (32, 1)),        # merge<1>
    (1000, 300, 48, 256, "uniform", (48, 1)),    # merge<8>
    (3000, 500, 64, 2, "uniform", (64, 1)),      # merge<64>
    (333, 100, 80, 256, "uniform", (80, 1)),
    (500, 129, 96, 3, "uniform", (96, 1)),
    (700, 257, 112, 256, "uniform", (112, 1)),
    (1000, 300, 128, 2, "uniform", (128, 1)),
    (600, 200, 144, 256, "uniform", (144, 1)),
    (900, 100, 160, 256, "uniform", (160, 1)),
    (700, 300, 176, 256, "uniform", (192, 1)),
    (500, 100, 208, 3, "uniform", (256, 1)),
    (300, 100, 272, 256, "uniform", ("wide", 1)),
    (200, 130, 512, 2, "uniform", ("wide", 1)),
    # Q = 4 (dim_pad <= 64)
    (XQ4, 1025, 16, 3, "uniform", (32, 4)),
    (XQ4, 1025, 32, 256, "uniform", (32, 4)),
    (XQ4, 1025, 48, 2, "uniform", (48, 4)),
    (XQ4, 1025, 64, 256, "uniform", (64, 4)),
    # Q = 2 at dim_pad <= 64
    (XQ2, 1537, 32, 3, "uniform", (32, 2)),
    (XQ2, 1537, 48, 256, "uniform", (48, 2)),
    (XQ2, 1537, 64, 2, "uniform", (64, 2)),
    # Q = 2 at dims 80..256
    (XQ2, 2049, 80, 256, "uniform", (80, 2)),
    (XQ2, 2049, 96, 3, "uniform", (96, 2)),
    (XQ2, 2049, 112, 256, "uniform", (112, 2)),
    (XQ2, 2049, 128, 2, "uniform", (128, 2)),
    (XQ2, 2049, 144, 3, "uniform", (144, 2)),
    (XQ2, 2049, 144, 256, "sift", (144, 2)),     # SIFT table normalised to 144 columns
    (XQ2, 2049, 160, 256, "uniform", (160, 2)),
    (XQ2, 2049, 176, 3, "uniform", (192, 2)),
    (XQ2, 2049, 192, 256, "uniform", (192, 2)),
    (XQ2, 2049, 208, 256, "uniform", (256, 2)),
    (XQ2, 2049, 240, 2, "uniform", (256, 2)),
    (XQ2, 2049, 256, 256, "uniform", (256, 2)),
    # wide rows, two queries per lane: a ragged 16-byte end after whole 128-byte chunks
    (4096 + 37, 2049, 400, 256, "uniform", ("wide", 2)),
    (4096 + 37, 2049, 1040, 3, "uniform", ("wide", 2)),
]


def case_id(case):
    xrows, yrows, dim, hi, kind, (w, q) = case
    return "%dx%dx%d-%s%d-%s-q%d" % (xrows, yrows, dim, kind, hi, w, q)


def plan_key(plan):
    """(dim_pad or "wide", q, wide) of a device.l1k2_plan() dict, as in INSTANTIATED."""
    return ("wide" if plan["wide"] else plan["dim_pad"], plan["q"], plan["wide"])


def merge_form(plan):
    return 1 if plan["slices"] <= 4 else 8 if plan["slices"] <= 32 else 64


def _sift_u8(rows, rng):
    """The golden SIFT table (132 columns) normalised as the reference pipeline does
    (normalize_to_ubyte_and_multiple_16_dim: 144 columns), tiled to `rows` rows with every other
    row perturbed by a few units: unperturbed rows repeat every 1168 rows (exact copies in
    different slices)."""
    from spectavi_amd import feature
    t = np.load(os.path.join(GOLDEN, "sift_sur_ogre_table.npz"))["table"]
    u = (feature.normalize_to_ubyte_and_multiple_16_dim(t) + 128).astype(np.int16)
    out = u[rng.permutation(len(u))][np.arange(rows) % len(u)]
    noisy = rng.random(rows) < 0.5
    out[noisy] += rng.integers(-3, 4, (int(noisy.sum()), u.shape[1])).astype(np.int16)
    return np.clip(out, 0, 255).astype(np.uint8)


def make_case(case):
    """(x, y, dups): the case's data.  dups lists query rows k that were also written into two
    database rows in different slices (one in the first slice, one in the ragged last one): the
    query at the end of the last block, one in the middle and the first."""
    xrows, yrows, dim, hi, kind, _ = case
    rng = np.random.default_rng([xrows, yrows, dim, hi, kind == "sift"])
    if kind == "sift":
        x, y = _sift_u8(xrows, rng), _sift_u8(yrows, rng)
    else:
        x = rng.integers(0, hi, (xrows, dim), dtype=np.uint8)
        y = rng.integers(0, hi, (yrows, dim), dtype=np.uint8)
    dups = []
    if xrows >= 128:
        for j, k in enumerate(sorted({yrows - 1, yrows // 2, 0})):
            a, b = 3 + 17 * j, xrows - 1 - j
            x[a] = y[k]
            x[b] = y[k]
            dups.append(k)
    return x, y, dups


def expected_dup_rows(x, y, k):
    """The two lowest database rows identical to query k (ascending index breaks the distance-0 tie)."""
    return np.flatnonzero((x == y[k]).all(axis=1))[:2]
