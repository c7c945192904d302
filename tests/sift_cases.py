"""Shared inputs and the table comparison of the SIFT tests."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def sur_ogre():
    """(image float32 [233, 310], vlfeat's table float32 [1168, 132])."""
    im = np.load(os.path.join(GOLDEN, "sift_sur_ogre_image.npz"))["im"].astype(np.float32)
    table = np.load(os.path.join(GOLDEN, "sift_sur_ogre_table.npz"))["table"]
    return im, table


def smooth_random(seed, h, w, passes=3):
    """Uniform noise in [0, 255) smoothed by `passes` circular [1 1 1]/3 passes along each axis."""
    r = np.random.default_rng(seed).random((h, w)) * 255
    for _ in range(passes):
        r = (r + np.roll(r, 1, 0) + np.roll(r, -1, 0)) / 3
        r = (r + np.roll(r, 1, 1) + np.roll(r, -1, 1)) / 3
    return r.astype(np.float32)


def castle(name):
    """240 x 320 crop of the reference's castle photograph `name` ("01", "02"): grey uint8 values, 17-19 % of
    them saturated sky (exactly 255)."""
    return np.load(os.path.join(GOLDEN, "sift_castle_%s.npz" % name))["im"].astype(np.float32)


def white_noise(seed, h, w, binary=False):
    """Independent uint8 pixels; `binary`: only 0 and 255."""
    rng = np.random.default_rng(seed)
    if binary:
        return (rng.integers(0, 2, (h, w)) * 255).astype(np.float32)
    return rng.integers(0, 256, (h, w)).astype(np.float32)


def grey_levels(im, levels=4):
    """`im` (0..255) reduced to `levels` equally spaced grey values: wide exactly flat regions."""
    step = 256 // levels
    return (np.floor(im / step) * (255 // (levels - 1))).astype(np.float32)


def stretch_clip(im):
    """Contrast doubled about 128 and clipped: saturated regions at both ends."""
    return np.clip(2 * im - 128, 0, 255).astype(np.float32)


def edge_and_corner(h=96, w=128):
    """A vertical step edge down the whole image (responses that only the edge score can reject), a bright
    rectangle (four corners) and a dark slanted wedge whose edges run between the pixel centres."""
    im = np.full((h, w), 40, np.float32)
    im[:, (2 * w) // 3:] = 200
    im[h // 5:h // 2, w // 8:w // 3] = 230
    y, x = np.mgrid[0:h, 0:w]
    im[(y > (2 * h) // 3) & (x - w // 6 < 2 * (y - (2 * h) // 3)) & (x > w // 6)] = 5
    return im


def checkerboard(h=96, w=128, cell=8):
    y, x = np.mgrid[0:h, 0:w]
    return (((y // cell + x // cell) % 2) * 255).astype(np.float32)


BLOBS = ((30, 30, 3.0), (80, 40, 5.0), (60, 75, 8.0), (110, 80, 2.0))  # x, y, sigma


def blobs(h=96, w=128, amplitude=200.0):
    """Gaussian blobs of amplitude 200 on black at BLOBS: the normalised-Laplacian peak of a Gaussian blob
    of width sigma lies at its centre, at scale sigma."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    im = np.zeros((h, w))
    for cx, cy, sg in BLOBS:
        im += amplitude * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2 * sg * sg))
    return im.astype(np.float32)


def blob_matches(table):
    """Per blob of BLOBS: (distance of the nearest keypoint to the centre, its sigma / blob sigma)."""
    out = []
    for cx, cy, sg in BLOBS:
        d = np.hypot(table[:, 0].astype(np.float64) - cx, table[:, 1].astype(np.float64) - cy)
        near = np.flatnonzero(d <= 0.5)
        ratios = table[near, 2].astype(np.float64) / sg
        ok = near[(ratios >= 2.0 ** (-1.0 / 3)) & (ratios <= 2.0 ** (1.0 / 3))]
        i = ok[np.argmin(d[ok])] if len(ok) else (np.argmin(d) if len(d) else None)
        out.append((float("inf"), float("nan")) if i is None else (float(d[i]), float(table[i, 2]) / sg))
    return out


def assert_blobs_found(table, what):
    """Every blob has a keypoint within 0.5 px of its centre whose sigma is within one scale step (a factor
    2^(1/3)) of the blob's: the normalised Laplacian of a Gaussian blob peaks at the centre, at scale sigma."""
    for (cx, cy, sg), (d, r) in zip(BLOBS, blob_matches(table)):
        print("%s: blob (%g, %g, sigma %g): centre error %.3f px, sigma ratio %.3f" % (what, cx, cy, sg, d, r))
        assert d <= 0.5, "%s: no keypoint within 0.5 px of the blob at (%g, %g): nearest %.3f" % (what, cx, cy, d)
        assert 2.0 ** (-1.0 / 3) <= r <= 2.0 ** (1.0 / 3), "%s: blob sigma %g found at ratio %.3f" % (what, sg, r)


def _ogre():
    return sur_ogre()[0]


# Widths whose octave widths (2w, w, w >> 1 at a height of 40) lie on a block (256 columns per block) or
# wave (64 columns per step from column 1, so w - 2 = 64 k) seam, or one to either side of it.
SEAM_HEIGHT = 40
SEAM_OCTAVE_WIDTHS = {31: (62, 31), 32: (64, 32, 16), 33: (66, 33, 16), 63: (126, 63, 31), 64: (128, 64, 32),
                      65: (130, 65, 32), 127: (254, 127, 63), 128: (256, 128, 64), 129: (258, 129, 64),
                      255: (510, 255, 127), 256: (512, 256, 128), 257: (514, 257, 128)}
# (h, w): min(h, w) on either side of a step of the octave count, and the number of octaves
OCTAVE_STEP_SHAPES = {(15, 21): 1, (16, 21): 2, (17, 21): 2, (45, 31): 2, (45, 32): 3, (45, 33): 3}
THIN = {"thin-8x8192": (8, 8192), "thin-8192x8": (8192, 8), "thin-16x8191": (16, 8191)}
NO_ROWS = {"flat-3x8192": (3, 8192), "flat-8192x3": (8192, 3),            # six-row octave: nothing survives
           "no-interior-1x8192": (1, 8192), "no-interior-8192x1": (8192, 1)}  # two-row octave: no DoG interior

SMALL_RANGE = ("ogre/255", "ogre*1e-3")
PLATEAU = ("ogre-stretch-clip", "ogre-4-levels", "binary-noise", "u8-noise", "castle-01", "castle-02")
STRUCTURE = ("edge-corner", "checkerboard", "blobs")


def _cases():
    c = [("ogre/255", lambda: _ogre() / np.float32(255)),
         ("ogre*1e-3", lambda: _ogre() * np.float32(1e-3)),
         ("ogre*257", lambda: _ogre() * np.float32(257)),
         ("-ogre", lambda: -_ogre()),
         ("ogre-128", lambda: _ogre() - np.float32(128)),
         ("ogre-stretch-clip", lambda: stretch_clip(_ogre())),
         ("ogre-4-levels", lambda: grey_levels(_ogre())),
         ("binary-noise", lambda: white_noise(11, 96, 128, binary=True)),
         ("u8-noise", lambda: white_noise(12, 96, 128)),
         ("castle-01", lambda: castle("01")),
         ("castle-02", lambda: castle("02")),
         ("edge-corner", edge_and_corner),
         ("checkerboard", checkerboard),
         ("blobs", blobs)]
    seed = 100
    for group in (THIN, NO_ROWS):
        for name, (h, w) in group.items():
            seed += 1
            c.append((name, lambda s=seed, h=h, w=w: smooth_random(s, h, w)))
    for (h, w) in OCTAVE_STEP_SHAPES:
        seed += 1
        c.append(("min-side-%dx%d" % (h, w), lambda s=seed, h=h, w=w: smooth_random(s, h, w)))
    for w in SEAM_OCTAVE_WIDTHS:
        seed += 1
        c.append(("seam-%dx%d" % (SEAM_HEIGHT, w), lambda s=seed, w=w: smooth_random(s, SEAM_HEIGHT, w)))
    for (h, w) in ((127, 129), (255, 257)):
        seed += 1
        c.append(("seam-%dx%d" % (h, w), lambda s=seed, h=h, w=w: smooth_random(s, h, w)))
    return c


CASES = _cases()            # (name, image builder): deterministic float32 images
CASE_NAMES = [n for n, _ in CASES]


def case_image(name):
    return dict(CASES)[name]()


def ulp_diff(a, b):
    """Distance in float32 units in the last place (both finite, same sign assumed by the caller)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


def assert_tables_match(got, want, what="", ulp=0):
    """The same rows; x, y, sigma, angle at most `ulp` float32 units apart (0: bit-equal); descriptors
    equal."""
    assert got.dtype == np.float32 and got.ndim == 2 and got.shape[1] == 132, (what, got.shape, got.dtype)
    assert got.shape == want.shape, "%s: %d rows, expected %d" % (what, got.shape[0], want.shape[0])
    if got.shape[0] == 0:
        return
    d = ulp_diff(got[:, :4], want[:, :4])
    assert d.max() <= ulp, "%s: frame rows %s differ by up to %d ulp" % (what, np.nonzero(d.max(1) > ulp)[0][:8], d.max())
    bad = np.nonzero(~np.all(got[:, 4:] == want[:, 4:], axis=1))[0]
    assert bad.size == 0, "%s: descriptor rows %s differ" % (what, bad[:8])


def orientation_counts(table):
    """Rows per keypoint (x, y, sigma)."""
    if len(table) == 0:
        return np.zeros(0, np.int64)
    _, counts = np.unique(table[:, :3], axis=0, return_counts=True)
    return counts
