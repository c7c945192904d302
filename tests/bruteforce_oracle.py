"""numpy statement of the exact p-norm k-NN contract of nn_bruteforce / nn_bruteforcei
(include/spectavi_amd.h), written from that contract.

Per (query y_i, database row x_j): s = 0, then for c = 0..dim-1 in order s = s + t_c, every
operation rounded on its own.  numpy's float32 elementwise arithmetic is correctly rounded and
unfused, np.sqrt on float32 is correctly rounded, and np.power on float64 is the C library's pow,
so the vectorised form below (over a chunk of queries x the whole database, a Python loop over the
columns) is that arithmetic.  Selection: the k smallest (dist, idx) pairs, lexicographic, with
missing neighbours as idx 2**64-1 and dist +inf / INT_MAX."""
import numpy as np

NONE_IDX = np.uint64(2**64 - 1)
INT_MAX = np.int32(2**31 - 1)


def p_kind(p):
    """The branch of the contract that p (a C float, widened to double) takes."""
    pd = float(np.float32(p))
    return 1 if pd == 1.0 else 2 if pd == 2.0 else 0.5 if pd == 0.5 else None


def term(d, p, is_int):
    """t(d) of one column: d is float32 (for int rows, float32(int32(x - y)))."""
    kind = p_kind(p)
    if kind == 1:
        t = np.abs(d)
    elif kind == 2:
        t = d * d
    elif kind == 0.5:
        t = np.sqrt(np.abs(d))
    else:
        t = np.power(np.abs(d).astype(np.float64), float(np.float32(p)))
        if not is_int:
            t = t.astype(np.float32)
    if is_int:
        return np.trunc(t).astype(np.int64).astype(np.int32)
    return t


def distances(x, y, p, is_int=False):
    """dist[i, j] of query y[i] to database row x[j] (float32, or int32 for int rows)."""
    x = np.asarray(x)
    y = np.asarray(y)
    xrows, dim = x.shape
    yrows = y.shape[0]
    out = np.zeros((yrows, xrows), np.int32 if is_int else np.float32)
    for c in range(dim):
        if is_int:
            diff = (x[None, :, c].astype(np.int64) - y[:, None, c].astype(np.int64)).astype(np.int32)
            d = diff.astype(np.float32)
        else:
            with np.errstate(over="ignore"):   # finite x - y may overflow to +-inf: inside the contract
                d = x[None, :, c].astype(np.float32) - y[:, None, c].astype(np.float32)
        with np.errstate(over="ignore", invalid="ignore"):
            out = out + term(d, p, is_int)
    return out


def select(dist, k, is_int=False):
    """Per row of dist [yrows, xrows]: the k smallest (dist, idx) pairs, ascending, padded."""
    yrows, xrows = dist.shape
    idx = np.full((yrows, k), NONE_IDX, np.uint64)
    out = np.full((yrows, k), INT_MAX if is_int else np.float32(np.inf), dist.dtype)
    cols = np.arange(xrows)
    kk = min(k, xrows)
    if kk == 0:
        return idx, out
    for i in range(yrows):
        row = dist[i]
        if xrows > 4 * kk:  # only rows up to the kk-th smallest distance can be selected
            kth = np.partition(row, kk - 1)[kk - 1]
            cand = np.flatnonzero(row <= kth) if not np.isnan(kth) else cols
        else:
            cand = cols
        order = cand[np.lexsort((cand, row[cand]))][:kk]
        idx[i, :kk] = order
        out[i, :kk] = row[order]
    return idx, out


def nn_bruteforce(x, y, p, k, is_int=False, chunk=256):
    """(idx uint64 [yrows,k], dist float32 / int32 [yrows,k]) of the contract."""
    y = np.asarray(y)
    yrows = y.shape[0]
    idx = np.empty((yrows, k), np.uint64)
    dist = np.empty((yrows, k), np.int32 if is_int else np.float32)
    for lo in range(0, yrows, chunk):
        hi = min(yrows, lo + chunk)
        idx[lo:hi], dist[lo:hi] = select(distances(x, y[lo:hi], p, is_int), k, is_int)
    return idx, dist
