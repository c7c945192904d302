"""Tracks that tests/test_tracks_triangulate_gpu.py's scenes never form: numpy only.  The scenes, the model and the
criteria are tests/tracks_triangulate_model.py's.

(a) mismatched: every observation redrawn in the frame, so that sigma4 is of sigma3's size and the solver's inverse
    iteration (contraction rho = (sigma4 / sigma3)^2 a step, 8 steps, agreement to 1e-13) gives way to its Jacobi.
(b) rank_deficient: the same observation over and over (rank 2), the rows of one set (rank 3: the camera centre),
    two observations in turn (an ordinary track).
(c) the `edges` scene of the GPU tests with all cameras times a power of two or -1.
(d) the same scene with a NaN or +inf observation, or a camera with a NaN entry, in a usable member of six tracks."""
import numpy as np

from tests import tracks_triangulate_model as ttm

L0 = 16
SETTINGS = (L0, 0, 10 ** 9)
EDGE_LONG = [L0 - 1, L0, L0 + 1, 63, 64, 65, 129, 1000]
_cache = {}


def scene(seed, noise, lengths, distinct=True):
    """tests/test_tracks_triangulate_gpu.py's `scene` on the wide cameras."""
    rng = np.random.default_rng(seed)
    cams = ttm.wide_cameras(rng, 40)
    Xw = ttm.points(rng, len(lengths))
    geom, seg = ttm.observe(rng, cams, Xw, noise)
    off, mem = ttm.make_tracks(rng, lengths, len(cams), distinct)
    return dict(cams=cams, geom=geom, seg=seg, off=off, mem=mem, Xw=Xw, lengths=np.array(lengths), rng=rng)


def args(sc):
    return sc["geom"], sc["seg"], sc["cams"], sc["off"], sc["mem"]


def with_model(sc, max_error):
    sc["mo"] = ttm.model(*args(sc), max_error=max_error, qr_route=True)
    long_ = sc["lengths"] > 64
    sc["long_c"] = float(sc["mo"]["qr_excess"][long_].max()) if long_.any() else 0.0
    return sc


def form_tolerance(sc):
    """test_length_edges's bound on |X - X'| between the two forms of the kernel."""
    S = sc["mo"]["S"]
    return (64 * ttm.EPS * S[:, 0] * sc["mo"]["nused"] / 2) / (S[:, 2] - S[:, 3]) + 1e-15


# ---- (a) ------------------------------------------------------------------------------------------------------------
MISMATCH_LENGTHS = [3, 4, 5, 8, 16, 17, 64, 65, 129]


def mismatched():
    if "mismatched" not in _cache:
        sc = scene(31, 0.0, MISMATCH_LENGTHS * 40, distinct=False)
        rng = sc["rng"]
        sc["geom"][:, 0] = rng.uniform(0, 1280, len(sc["geom"]))
        sc["geom"][:, 1] = rng.uniform(0, 960, len(sc["geom"]))
        _cache["mismatched"] = with_model(sc, np.inf)
    return _cache["mismatched"]


def contraction(mo):
    """rho = (sigma4 / sigma3)^2 per track."""
    return (mo["S"][:, 3] / mo["S"][:, 2]) ** 2


# ---- (b) ------------------------------------------------------------------------------------------------------------
RANK_LENGTHS = (3, 17, 65)
TURN_LENGTHS = (17, 65)


def rank_deficient():
    """One call: tracks 0-2 repeat one observation, 3-5 hold different rows of one set, 6-7 alternate between two
    observations and 8-9 are the two-member tracks of those.  Exact observations (float32 rounding alone), so that the
    weights of the two observations do not move the null vector by more than the direction tolerance."""
    if "rank" not in _cache:
        sc = scene(32, 0.0, [2] * 70)
        mem, lengths = [], []
        for i, m in enumerate(RANK_LENGTHS):
            mem += [(5 + i, i)] * m
            lengths.append(m)
        for i, m in enumerate(RANK_LENGTHS):
            mem += [(11 + i, r) for r in range(m)]
            lengths.append(m)
        pairs = [((20, 7), (21, 7)), ((30, 9), (2, 9))]
        for (a, b), m in zip(pairs, TURN_LENGTHS):
            mem += [a if k % 2 == 0 else b for k in range(m)]
            lengths.append(m)
        for a, b in pairs:
            mem += [a, b]
            lengths.append(2)
        sc["mem"] = np.array(mem, np.int32)
        sc["off"] = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
        sc["lengths"] = np.array(lengths)
        _cache["rank"] = with_model(sc, np.inf)
    return _cache["rank"]


def camera_centre(P):
    v = np.linalg.svd(P)[2][3]
    return ttm.canonical_sign(v / np.linalg.norm(v))


# ---- (c), (d): the `edges` scene --------------------------------------------------------------------------------------
SCALES = (-40, -1, 3, 40)
FAR_SCALES = (445, -445)
POISON_LANE, POISON_WAVE = (2, 3, 5), (17, 65, 129)
POISON_KINDS = ("nan observation", "inf observation", "nan camera")


def edges():
    if "edges" not in _cache:
        lengths = EDGE_LONG + [2, 3, 4, 5] * 63 + [2, 3, 4]
        _cache["edges"] = with_model(scene(23, 0.5, lengths, distinct=False), 6.0)
    return _cache["edges"]


def scaled_cameras(sc, k=0, sign=1.0):
    return dict(sc, cams=sign * np.ldexp(sc["cams"], k))


def poisoned(kind):
    """(clean, dirty, tracks): the `edges` scene with a set 40 of its own (set 0's rows under set 0's camera), one
    member of each chosen track moved to it where the camera is poisoned; `dirty` has the poison, `clean` the same
    call without it."""
    sc = edges()
    lengths = sc["lengths"]
    tracks = [int(np.flatnonzero(lengths == m)[0]) for m in POISON_LANE + POISON_WAVE]
    npts = int(sc["seg"][1])
    geom = np.concatenate([sc["geom"], sc["geom"][:npts]])
    seg = np.concatenate([sc["seg"], [sc["seg"][-1] + npts]]).astype(np.int64)
    cams = np.concatenate([sc["cams"], sc["cams"][:1]])
    mem = sc["mem"].copy()
    clean = dict(sc, geom=geom, seg=seg, cams=cams, mem=mem)
    dirty = dict(clean, geom=geom.copy(), cams=cams.copy())
    for t in tracks:
        i = int(sc["off"][t]) + 1                       # the track's second member
        if kind == "nan camera":
            mem[i] = (40, t)
        else:
            row = int(seg[mem[i, 0]] + mem[i, 1])
            others = np.delete(np.arange(len(mem)), np.arange(sc["off"][t], sc["off"][t + 1]))
            assert not np.any(seg[mem[others, 0]] + mem[others, 1] == row), "the row is this track's alone"
            dirty["geom"][row, 1 if kind == "nan observation" else 0] = np.nan if kind == "nan observation" else np.inf
    if kind == "nan camera":
        dirty["cams"][40, 1, 2] = np.nan
    return clean, dirty, tracks


def nused_of(sc):
    usable = ttm.usable_members(sc["seg"], len(sc["seg"]) - 1, sc["mem"], None)
    return np.add.reduceat(usable.astype(np.int32), sc["off"][:-1]).astype(np.int32)
