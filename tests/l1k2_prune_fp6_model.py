"""A plain numpy statement of the FP6 form of the wide bound kernel (l1k2_prune_wide6_kernel of l1k2_prune.hip), beside
tests/l1k2_prune_wide_model.py, whose geometry and protocol it keeps unchanged:

  * the table: 256 x 5 integers k, the e2m3 values k/8; G(a, b) = k(a) . k(b), p and m are integers in units of 1/64 and
    a pair is ruled out iff 128 m - sum G > p thr, strictly, exactly as with the int8 tables.  So the decisions of a run
    are tests/l1k2_prune_wide_model.run with (k, p, m) as its table, and nothing of it is copied here;
  * the bit packing of a feature row (l1k2_feature6_kernel): what only this form has.

Row layout.  A 128-byte row becomes 512 bytes.  Chunk u = 2 s + g (k-step s of 64, lane half g) holds component u / 4 of
dimensions 32 (u % 4) .. + 31 as 32 six-bit codes, packed little-endian into 24 bytes.  Its first 16 bytes are bytes
16 u .. 16 u + 15 of the row, its last 8 bytes lie at 320 + 32 (s / 2) + 16 g + 8 (s % 2); bytes 480 .. 511 are zero."""
import numpy as np

from tests import l1k2_prune_wide_model as wm
from tests.l1k2_prune_model import prepare  # noqa: F401  (for callers: it takes any table width)

RANK = 5
E2M3 = tuple(range(16)) + tuple(range(16, 32, 2)) + tuple(range(32, 64, 4))   # the magnitudes k of the grid
ROW_BYTES = 512
CHUNKS = 20
TAIL = 320


def code_of(k):
    """The 6-bit e2m3 code (sign, two exponent bits, three mantissa bits) of the grid value k/8, elementwise."""
    k = np.asarray(k, dtype=np.int64)
    mag = np.abs(k)
    assert np.isin(mag, E2M3).all()
    code = np.where(mag < 16, mag, np.where(mag < 32, mag // 2 + 8, mag // 4 + 16))
    return np.where(k < 0, code | 32, code)


def value_of(code):
    """k of a 6-bit code: the inverse of code_of (0 and -0 both give 0)."""
    code = np.asarray(code, dtype=np.int64)
    c = code & 31
    k = np.where(c < 16, c, np.where(c < 24, 2 * (c - 8), 4 * (c - 16)))
    return np.where(code & 32, -k, k)


def tail_offset(s, g):
    return TAIL + 32 * (s >> 1) + 16 * g + 8 * (s & 1)


def pack_rows(rows, k):
    """uint8 [n, 512]: the feature rows of uint8 rows [n, 128] under the table k [256, 5]."""
    rows = np.asarray(rows, dtype=np.uint8)
    n = len(rows)
    out = np.zeros((n, ROW_BYTES), np.uint8)
    codes = code_of(k)                                              # [256, 5]
    for u in range(CHUNKS):
        c = codes[rows[:, 32 * (u % 4):32 * (u % 4) + 32], u // 4]  # [n, 32]
        bits = ((c[:, :, None] >> np.arange(6)) & 1).astype(np.uint8).reshape(n, 192)
        chunk = np.packbits(bits, axis=1, bitorder="little")        # [n, 24]
        out[:, 16 * u:16 * u + 16] = chunk[:, :16]
        t = tail_offset(u >> 1, u & 1)
        out[:, t:t + 8] = chunk[:, 16:]
    return out


def unpack_rows(feat):
    """int64 [n, 640]: the k of every operand element of feature rows [n, 512], in K order (k-step, lane half, element)."""
    n = len(feat)
    out = np.zeros((n, CHUNKS, 32), np.int64)
    for u in range(CHUNKS):
        t = tail_offset(u >> 1, u & 1)
        chunk = np.concatenate([feat[:, 16 * u:16 * u + 16], feat[:, t:t + 8]], axis=1)
        bits = np.unpackbits(chunk, axis=1, bitorder="little").reshape(n, 32, 6)
        out[:, u] = value_of((bits.astype(np.int64) << np.arange(6)).sum(axis=2))
    return out.reshape(n, CHUNKS * 32)


def feature_offsets(xrows, yrows, slices):
    """(byte offset of the database features, of the query features) in the workspace of a dim-128 call: behind the partial
    keys (16 bytes per query and slice), every piece rounded up to 256 bytes (L1K2Plan of common.h)."""
    part = -(-(max(yrows, 1) * slices * 16) // 256) * 256
    return part, part + xrows * ROW_BYTES


def check_table(k, p, m):
    """The checks of make_bound6, in int64: the grid, the inequality on all 65 536 pairs with m attained, the 2^24 bounds."""
    k = np.asarray(k, dtype=np.int64)
    assert k.shape == (256, RANK) and np.isin(np.abs(k), E2M3).all()
    a = np.arange(256, dtype=np.int64)
    G = k @ k.T
    slack = p * np.abs(a[:, None] - a[None, :]) - (m - G)
    assert slack.min() == 0, int(slack.min())
    assert 128 * abs(m) < 2 ** 24 and p * 128 * 255 < 2 ** 24 and 128 * int(np.abs(G).max()) < 2 ** 24
    return float((m - G.mean()) / p)


def run(x, y, table, blocks, share, schedule="up", pre=None, per_tile=None):
    """tests/l1k2_prune_wide_model.run with the FP6 table (k, p, m): (idx, dist, (bounded, survivors, fallback))."""
    return wm.run(x, y, table, blocks, share, schedule, pre, per_tile)
