"""The collections tests/test_cascade_batch_plan.py (host only) and tests/test_cascade_batch_gpu.py share, and the
data recipe: the ingredients of cascade_variant_cases.cascade_data -- planted near-copies, non-integer rows,
all-zero rows, every third hyperplane column rounded to an integer -- spread over the sets of a collection.
Below them, the collections built to reach one path of cascade_batch.hip each (tests/test_cascade_batch_edge_cases.py,
host only, and tests/test_cascade_batch_edges_gpu.py)."""
import numpy as np

NINE = [0, 1, 2, 63, 64, 65, 257, 513, 1000]          # rows of the nine-set collection
ALL81 = [(a, b) for a in range(9) for b in range(9)]   # every ordered pair, self pairs included
NINE_SHAPE = (128, 6, 2, 2)                            # dim, m, n, g

# three sets -- two work items and a ragged third, less than one item, one item and a row -- and five pairs: every
# set as query and as database, a self pair
FEW_ROWS = [130, 33, 65]
FEW = [(0, 1), (1, 2), (2, 0), (1, 1), (0, 2)]
# (dim, m, n, g): non-power-of-two widths, two chunks per lane (dim > 128), m above any bucket-bit cap, g = 0 and
# g = 16, and the three projection families
EDGES = [(16, 29, 2, 16), (48, 4, 2, 3), (80, 25, 2, 0), (128, 9, 2, 2), (144, 8, 9, 6), (256, 24, 3, 6), (32, 31, 3, 16)]

# pair bookkeeping: the first and the last set empty, repeated pairs, pairs in descending order
BOOK_ROWS = [0, 70, 33, 0]
BOOK = [(2, 1), (1, 2), (2, 1), (3, 1), (1, 0), (1, 3), (0, 1), (2, 2), (1, 1), (1, 2)]
DESCENDING = sorted(set(BOOK), reverse=True)


def seg_of(rows):
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


def hash_dict(dim, m, n, g, seed=7):
    """Hyperplanes with every third column rounded to integers, so that projections tie in magnitude or are zero."""
    d = np.random.default_rng([dim, m, n, g, seed, 1]).standard_normal((n, dim, m)).astype(np.float32)
    d[:, :, ::3] = np.round(d[:, :, ::3])
    return d


def collection(rows, dim, m, n, g, seed=7):
    """(packed float32 [sum(rows), dim], seg_off, dict): integer rows in [-128, 128); half of them near-copies (+-2
    per component) of rows anywhere in the collection, so every pair of sets shares planted neighbours; a tenth
    non-integer; every 97th and every 89th row all zero."""
    rng = np.random.default_rng([dim, m, n, g, seed, len(rows)])
    total = int(sum(rows))
    x = rng.integers(-128, 128, (total, dim)).astype(np.float32)
    if total:
        k = total // 2
        dst, src = rng.choice(total, k, replace=False), rng.integers(0, total, k)
        x[dst] = np.clip(x[src] + rng.integers(-2, 3, (k, dim)), -128, 127)
        frac = rng.choice(total, max(1, total // 10), replace=False)
        x[frac] += rng.uniform(-0.49, 0.49, (len(frac), dim)).astype(np.float32)
        x[::97] = 0.0
        x[3::89] = 0.0
    return x, seg_of(rows), hash_dict(dim, m, n, g, seed)


def image(x):
    """The uint8 refine image of float32 rows: (int(trunc v) + 128) & 255."""
    return ((np.trunc(x).astype(np.int64) + 128) & 255).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# The collections of tests/test_cascade_batch_edge_cases.py (host only: each reaches the path it names) and
# tests/test_cascade_batch_edges_gpu.py (the same collections against the oracle).  Every builder returns
# (x, seg, d, pairs, g).
# ---------------------------------------------------------------------------------------------------------------
def both_ways(nsets, self_pair):
    """Every set as query and as database of every other one, and one set against itself."""
    return [(a, b) for a in range(nsets) for b in range(nsets) if a != b] + [(self_pair, self_pair)]


# bucket bits at the 4096 | 4097 rows edge: (rows of the largest set, m, the hb the plan must name)
BITS_EDGE = [(4096, 20, 12), (4097, 20, 13), (4097, 13, 13)]
BITS_EDGE_DIM = 16


def bits_edge(big, m):
    x, seg, d = collection([257, 513, big], BITS_EDGE_DIM, m, 2, 2)
    return x, seg, d, both_ways(3, 2), 2


# hb invariance: one pair of small sets alone, beside 4097 rows, beside 70000 rows: (bystander rows, hb)
BYSTANDERS = [(0, 12), (4097, 13), (70000, 17)]
INVARIANCE_SHAPE = (16, 20, 2, 2)
INVARIANCE_PAIRS = [(0, 1), (1, 0), (1, 1)]


def invariance(bystander):
    """The sets 0 and 1 are the same rows whatever the bystander (set 2, never in a pair) holds."""
    dim, m, n, g = INVARIANCE_SHAPE
    x, _, d = collection([257, 130], dim, m, n, g)
    extra = np.random.default_rng([bystander, 3]).integers(-128, 128, (bystander, dim)).astype(np.float32)
    return np.concatenate([x, extra]), seg_of([257, 130, bystander]), d, INVARIANCE_PAIRS, g


# the memory cap: 65534 bucket tables pass 1 GiB at 12 bits
CAP_SETS = 32767
CAP_SHAPE = (16, 24, 2, 2)
CAP_BIG = {0: 300, 1: 100, 16383: 257, 32765: 130, 32766: 193}   # set number: rows


def cap():
    """32767 sets of 0, 1 or 2 rows (runs of up to 40 empty sets among them) but for the five of CAP_BIG, which
    hold near-copies (+-1) of each other's rows.  Pairs: every ordered pair of the five, self pairs included, then
    tiny and empty sets on either side of a pair."""
    dim, m, n, g = CAP_SHAPE
    rng = np.random.default_rng([CAP_SETS, dim, m, 5])
    rows = rng.choice([0, 1, 2], CAP_SETS, p=[.3, .4, .3])
    for start in rng.integers(2, CAP_SETS - 50, 200):
        if not 16300 < start < 16400:
            rows[start:start + rng.integers(2, 41)] = 0
    for s, r in CAP_BIG.items():
        rows[s] = r
    rows[[2, 16382, 16384, 32764]] = [0, 2, 0, 1]   # the neighbours of the five: empty, full, empty, one row
    seg = seg_of(rows)
    total = int(seg[-1])
    x = rng.integers(-128, 128, (total, dim)).astype(np.float32)
    big = sorted(CAP_BIG)
    for s in big[1:]:      # half of each later big set: near-copies of rows of the one before it
        k = CAP_BIG[s] // 2
        prev = big[big.index(s) - 1]
        src = seg[prev] + rng.integers(0, CAP_BIG[prev], k)
        x[seg[s]:seg[s] + k] = np.clip(x[src] + rng.integers(-1, 2, (k, dim)), -128, 127)
    tiny = np.nonzero(rows == 1)[0]
    two = np.nonzero(rows == 2)[0]
    for s in tiny[::7]:    # some one-row sets: a near-copy of a row of set 0
        x[seg[s]] = np.clip(x[rng.integers(0, CAP_BIG[0])] + rng.integers(-1, 2, dim), -128, 127)
    empty = np.nonzero(rows == 0)[0]
    pairs = [(a, b) for a in big for b in big]
    pairs += [(int(s), 0) for s in tiny[:70:7]] + [(0, int(s)) for s in tiny[:21:7]]
    pairs += [(int(two[0]), 1), (16383, int(two[-1])), (int(two[-1]), 16383), (int(two[5]), int(two[5])), (16382, 16383),
              (int(tiny[-1]), 32766), (32764, 32765), (32766, 32764)]
    pairs += [(int(empty[0]), 0), (0, int(empty[0])), (32765, 16384), (16384, 32765), (2, 2), (int(empty[-1]), int(tiny[3])),
              (int(tiny[3]), int(empty[-1]))]
    return x, seg, hash_dict(dim, m, n, g), pairs, g


# the full-code filter: hb = 12 < m = 24.  With one table the candidates of the mixed bucket are a query's only ones:
# with two, the second table's bucket of a single code holds the same rows again
FILTER_SHAPE = (128, 24, 2, 2)
FILTER_TABLES = [2, 1]
FILTER_ROWS = [33, 300, 40]
FILTER_PAIRS = [(2, 1), (1, 2)]


def codes_of(x, d, g=0):
    """The oracle's database codes of rows x, uint32 [n, rows]."""
    from oracle import oracle as o
    n, _, m = d.shape
    return o.nn_cascading_hash(x, x[:1], m, n, g, d, debug=True)[4]


def mixed_bucket(n=2, hb=12):
    """Set 1: 150 near-copies of a row A and 150 of a row B, interleaved row by row, where the table-0 codes of A
    and B agree in the low hb bits and differ above, and every copy has its parent's code in every table.  Set 2:
    20 further copies of each, interleaved too.  Set 0: 33 plain rows.  n: the tables, FILTER_SHAPE's or one."""
    dim, m, _, g = FILTER_SHAPE
    draw, _, d = collection([2000], dim, m, n, g)
    code = codes_of(draw, d)
    low = code[0] & ((1 << hb) - 1)
    by_low = np.lexsort((code[0], low))
    rng = np.random.default_rng([dim, m, hb, 9])
    for i, j in zip(by_low[:-1], by_low[1:]):
        if low[i] != low[j] or (code[:, i] == code[:, j]).any():
            continue
        copies = []
        for parent in (i, j):
            c = np.clip(draw[parent] + rng.integers(-2, 3, (400, dim)), -128, 127).astype(np.float32)
            c = c[(codes_of(c, d) == code[:, parent:parent + 1]).all(axis=0)]
            copies.append(c[:170])
        if len(copies[0]) == len(copies[1]) == 170:
            break
    else:
        raise AssertionError("no two rows of the draw share the low %d bits of their table-0 code" % hb)
    a, b = copies
    x, seg, _ = collection(FILTER_ROWS, dim, m, n, g)
    x[seg[1]:seg[2]:2], x[seg[1] + 1:seg[2]:2] = a[:150], b[:150]
    x[seg[2]:seg[3]:2], x[seg[2] + 1:seg[3]:2] = a[150:], b[150:]
    return x, seg, d, FILTER_PAIRS, g


LONG_HIT = np.arange(10) * 25 + 3   # the rows of set 2 that equal the repeated row


def long_bucket(shape):
    """test_a_bucket_longer_than_the_lds_list's collection: set 1 is 1500 copies of one row, ten rows of set 2 too."""
    dim, m, n, g = shape
    x, seg, d = collection([300, 1500, 257], dim, m, n, g)
    x[seg[1]:seg[2]] = x[seg[1]]
    x[seg[2] + LONG_HIT] = x[seg[1]]
    return x, seg, d, [(2, 1), (1, 0)], g


# the probes' buckets fit the 512-entry list one by one, not together: hb = m = 4, 16 buckets of a 2000-row set
SUM_SHAPE = (48, 4, 2, 2)
SUM_ROWS = [2000, 100]
SUM_PAIRS = [(1, 0), (0, 1)]
LIST_CAP = 512


def bucket_sum():
    x, seg, d = collection(SUM_ROWS, *SUM_SHAPE)
    return x, seg, d, SUM_PAIRS, SUM_SHAPE[3]


# past one grid of rows: 2048 workgroups of 256 rows rank and fill 524288 packed rows per trip
GRID_ROWS = 2048 * 256
STRIDE_ROWS = [GRID_ROWS - 50, 700, 300]
STRIDE_SHAPE = (16, 20, 2, 2)
STRIDE_PAIRS = [(2, 1), (1, 2), (2, 2), (1, 1), (2, 0)]


def stride():
    """Set 1 straddles packed row 524288 (50 rows before it), set 2 lies past it and holds +-1 near-copies of
    set-1 rows chosen at random: the first 300 of 400 drawn whose parent set the oracle finds a candidate in."""
    from oracle import oracle as o
    dim, m, n, g = STRIDE_SHAPE
    x, seg, d = collection(STRIDE_ROWS, dim, m, n, g)
    rng = np.random.default_rng([dim, m, 13])
    src = seg[1] + rng.integers(0, STRIDE_ROWS[1], 400)
    copies = np.clip(np.trunc(x[src]) + rng.integers(-1, 2, (400, dim)), -128, 127).astype(np.float32)
    found = o.nn_cascading_hash(x[seg[1]:seg[2]], copies, m, n, g, d)[2] >= 1
    x[seg[2]:] = copies[found][:STRIDE_ROWS[2]]
    return x, seg, d, STRIDE_PAIRS, g


# every projection form: set boundaries inside the 256-row projection tiles of 528 rows, three workgroups
FORMS_ROWS = [130, 33, 65, 300]
FORMS_PAIRS = FEW + [(3, 0), (0, 3)]
