"""The collections tests/test_cascade_batch_plan.py (host only) and tests/test_cascade_batch_gpu.py share, and the
data recipe: the ingredients of cascade_variant_cases.cascade_data -- planted near-copies, non-integer rows,
all-zero rows, every third hyperplane column rounded to an integer -- spread over the sets of a collection."""
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
