"""Named, seeded value classes for nn_bruteforce / nn_bruteforcei over the finite float32 and the
int32 domain of the contract (include/spectavi_amd.h), and the table of cases built from them.

Every class is a function (rng, rows, dim) -> array [rows, dim]; database and queries of a case are
one draw of xrows + yrows rows, cut in two, so classes with per-column structure (`mixed`) give both
sides the same columns.  All float values are finite, so every class is inside the contract; the int
classes assert the header's domain (no int32 overflow in x - y, in a term or in a partial sum).

What each class is for:
  huge    |d| ~ 1e19: d*d ~ 1e38, the p = 2 sums overflow to +inf; p = 1, 0.5 stay finite
  max     |v| in [1e38, 3.4e38] with random signs: x - y overflows to +-inf, distances are +inf and tie
  subn    multiples of 2**-149: every difference is subnormal; p = 2 underflows to exactly 0, all tie
  under   |d| ~ 1e-20 is normal, d*d ~ 1e-40 is subnormal
  mixed   column scales over 16 decades: small terms are absorbed, in summation order
  offset  1e6 + 0.1 randn: differences are exact multiples of 2**-4, many repeated distances
  zeros   a mix of +0.0 and -0.0: every distance is +0
  i_big_* int rows whose differences / terms pass 2**24, where float32 no longer holds every integer
"""
from collections import namedtuple

import numpy as np

XROWS = 97   # three full 32-row groups and a ragged one
YROWS = 70   # a partial query block
KS = (2, 8, 17)   # one per list length KB of bf_tile_kernel

# bf_tile_kernel<INT, PK, KB> (spectavi_amd/csrc/bruteforce.hip): the p branch and the list length
P_KIND = {1.0: 0, 2.0: 1, 0.5: 2}


def k_bucket(k):
    return 2 if k <= 2 else 8 if k <= 8 else 64


EXACT_INSTANTIATIONS = {(i, pk, kb) for i in (False, True) for pk in (0, 1, 2) for kb in (2, 8, 64)}


# ---- float32 classes ----------------------------------------------------------------------------
def huge(rng, rows, dim):
    return (rng.standard_normal((rows, dim)) * 1e19).astype(np.float32)


def vmax(rng, rows, dim):
    return (rng.choice([-1.0, 1.0], (rows, dim)) * rng.uniform(1e38, 3.4e38, (rows, dim))).astype(np.float32)


def subn(rng, rows, dim):
    return (rng.integers(-40, 41, (rows, dim)) * 2.0 ** -149).astype(np.float32)


def under(rng, rows, dim):
    return (rng.standard_normal((rows, dim)) * 1e-20).astype(np.float32)


def mixed(rng, rows, dim):
    return (rng.standard_normal((rows, dim)) * 10.0 ** rng.integers(-8, 9, (1, dim))).astype(np.float32)


def offset(rng, rows, dim):
    return (1e6 + rng.standard_normal((rows, dim)) * 0.1).astype(np.float32)


def zeros(rng, rows, dim):
    return np.where(rng.random((rows, dim)) < 0.5, 0.0, -0.0).astype(np.float32)


def randn(rng, rows, dim):
    return rng.standard_normal((rows, dim)).astype(np.float32)


# ---- int32 classes ------------------------------------------------------------------------------
def int_terms64(diff, p):
    """trunc(float32 op(float32(diff))) of the contract as int64, without the cast to int32 (diff: int64
    values that fit int32)."""
    d = diff.astype(np.float32)
    t = np.abs(d) if p == 1.0 else d * d if p == 2.0 else np.sqrt(np.abs(d))
    return np.trunc(t).astype(np.int64)


def int_domain_ok(x, y, p):
    """The header's int domain, recomputed in int64 for every (query, database row) pair: x - y, every
    term and every partial sum fit in int32."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    lim = 2 ** 31 - 1
    s = np.zeros((y.shape[0], x.shape[0]), np.int64)
    for c in range(x.shape[1]):
        diff = x[None, :, c] - y[:, None, c]
        if diff.size and (diff.min() < -lim - 1 or diff.max() > lim):
            return False
        t = int_terms64(diff, p)
        s = s + t   # terms are >= 0: the partial sums only grow, int64 cannot overflow at dim <= 2048
        if t.size and (t.max() > lim or s.max() > lim):
            return False
    return True


def int_domain_bound_ok(x, y, p):
    """A cheap sufficient condition for int_domain_ok (rows x dim work instead of pairs x dim): the terms
    grow with |x - y|, so the widest difference each column allows bounds every pair's sum."""
    a = np.concatenate([np.asarray(x, np.int64), np.asarray(y, np.int64)])
    if a.shape[0] == 0:
        return True
    span = a.max(0) - a.min(0)
    if span.max() > 2 ** 31 - 1:
        return False
    t = int_terms64(span, p)
    return bool(t.max() <= 2 ** 31 - 1 and t.sum() <= 2 ** 31 - 1)


def int_uniform(span_of_dim, p):
    def gen(rng, rows, dim):
        span = span_of_dim[dim]
        a = rng.integers(-span, span, (rows, dim)).astype(np.int32)
        assert int_domain_ok(a, a, p), "int32 overflow: outside the contract's domain"
        return a
    return gen


ValueClass = namedtuple("ValueClass", "name gen is_int ps dims")

CLASSES = [
    ValueClass("huge", huge, False, (1.0, 2.0, 0.5), (7, 40)),
    ValueClass("max", vmax, False, (1.0, 2.0, 0.5), (7, 40)),
    ValueClass("subn", subn, False, (1.0, 2.0, 0.5), (7, 40)),
    ValueClass("under", under, False, (2.0,), (7, 40)),
    ValueClass("mixed", mixed, False, (1.0, 2.0, 0.5), (7, 40)),
    ValueClass("offset", offset, False, (1.0, 2.0, 0.5), (4, 40)),
    ValueClass("zeros", zeros, False, (1.0, 2.0, 0.5), (1, 40)),
    ValueClass("i_big_p1", int_uniform({1: 2 ** 29, 7: 2 ** 27}, 1.0), True, (1.0,), (1, 7)),
    ValueClass("i_big_p2", int_uniform({1: 20000, 4: 10000, 40: 3000}, 2.0), True, (2.0,), (1, 4, 40)),
    ValueClass("i_big_half", int_uniform({40: 2 ** 29}, 0.5), True, (0.5,), (40,)),
]
BY_NAME = {c.name: c for c in CLASSES}

Case = namedtuple("Case", "cls is_int p k dim")


def case_id(c):
    return "%s-p%g-k%d-dim%d" % (c.cls, c.p, c.k, c.dim)


def _table():
    out = []
    for vc in CLASSES:
        for n, p in enumerate(vc.ps):
            if len(vc.ps) == 1:   # a class made for one p: every k at every dim
                pairs = [(k, dim) for dim in vc.dims for k in KS]
            else:                 # every k, the dims taken in turn (shifted from one p to the next)
                pairs = [(k, vc.dims[(j + n) % len(vc.dims)]) for j, k in enumerate(KS)]
            out += [Case(vc.name, vc.is_int, p, k, dim) for k, dim in pairs]
    return out


CASES = _table()
REACHED = {(c.is_int, P_KIND[c.p], k_bucket(c.k)) for c in CASES}


def make(cls, dim, xrows=XROWS, yrows=YROWS, seed=0):
    """(x [xrows, dim], y [yrows, dim]) of a class: one seeded draw, the same for every p and k."""
    names = [c.name for c in CLASSES]
    rng = np.random.default_rng([11, names.index(cls), dim, xrows, yrows, seed])
    a = BY_NAME[cls].gen(rng, xrows + yrows, dim)
    return np.ascontiguousarray(a[:xrows]), np.ascontiguousarray(a[xrows:])


def case_data(c):
    return make(c.cls, c.dim)


def describe(dist, k):
    """What a float32 distance matrix [yrows, xrows] reaches: the shares of +inf, zero and subnormal
    distances, and of queries whose k-th and (k+1)-th smallest distances are equal."""
    d = np.asarray(dist, np.float32)
    srt = np.sort(d, axis=1)
    tiny = np.float32(2.0 ** -126)
    return {"inf": float(np.isposinf(d).mean()), "zero": float((d == 0).mean()),
            "subnormal": float(((d != 0) & (np.abs(d) < tiny)).mean()), "nan": float(np.isnan(d).mean()),
            "kth_tie": float((srt[:, k - 1] == srt[:, k]).mean()) if d.shape[1] > k else 0.0}
