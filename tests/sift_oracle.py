"""numpy statement of the sift_filter contract (include/spectavi_amd.h): vlfeat's vl_sift_* with every
setting at its default, restated step by step in the float / double widths vlfeat uses.

The scale space, DoG, extremum test and gradients are vectorised over pixels; refinement, orientation
and the descriptor run per keypoint.  Every float sum is accumulated in the order vlfeat accumulates it:
the convolution taps in p-ascending order, the histograms in raster order per bin (np.add.at is
unbuffered and applies its indices in order), the norms in index order.  numpy follows NEP 50, so a
float32 operand stays float32 next to a Python float; every double step converts with float() first."""
import math

import numpy as np

F32 = np.float32
FLT_EPS = float(np.finfo(np.float32).eps)
DBL_EPS = float(np.finfo(np.float64).eps)
TWO_PI_F = F32(2 * math.pi)
S = 3
OMIN = -1
SIGMAK = 2.0 ** (1.0 / S)
SIGMA0 = 1.6 * SIGMAK
DSIGMA0 = SIGMA0 * math.sqrt(1.0 - 1.0 / (SIGMAK * SIGMAK))
EXPN_TAB = np.array([math.exp(-k * (25.0 / 256)) for k in range(257)], np.float64)


def noctaves(wid, hgt):
    return max(int(math.floor(math.log2(min(wid, hgt)))) - OMIN - 3, 1)


def octave_shape(wid, hgt, o):
    return (hgt << 1, wid << 1) if o < 0 else (hgt >> o, wid >> o)


def gauss_taps(sigma):
    """(W, taps float32 [2W+1]) of the smoothing by sigma (double)."""
    W = max(int(math.ceil(4.0 * sigma)), 1)
    taps = np.empty(2 * W + 1, np.float32)
    acc = F32(0)
    for j in range(2 * W + 1):
        d = F32(F32(j - W) / F32(sigma))
        taps[j] = F32(math.exp(-0.5 * float(d * d)))
        acc = F32(acc + taps[j])
    return W, (taps / acc).astype(np.float32)


def smooth(im, sigma):
    """Vertical pass then horizontal pass; each output acc += in[clamp(p)] * tap over p ascending."""
    W, taps = gauss_taps(sigma)

    def pass_rows(a):  # convolve along axis 0
        n = a.shape[0]
        acc = np.zeros_like(a)
        y = np.arange(n)
        for j in range(2 * W + 1):
            p = np.clip(y - W + j, 0, n - 1)
            acc = acc + a[p] * taps[2 * W - j]
        return acc

    return pass_rows(pass_rows(im).T).T.copy()


def upsample(im):
    """x then y: out[2i] = a[i], out[2i+1] = (a[i] + a[i+1]) * 0.5f; the last two samples are a[n-1]."""
    def rows(a):
        n = a.shape[1]
        out = np.empty((a.shape[0], 2 * n), np.float32)
        out[:, 0::2] = a
        out[:, 1:2 * n - 2:2] = (a[:, :-1] + a[:, 1:]) * F32(0.5)
        out[:, 2 * n - 1] = a[:, n - 1]
        return out
    return rows(rows(im).T).T.copy()


def octaves(im):
    """Yields (o, levels float32 [6, h, w]) for every octave."""
    hgt, wid = im.shape
    base = None
    for o in range(OMIN, OMIN + noctaves(wid, hgt)):
        h, w = octave_shape(wid, hgt, o)
        if o == OMIN:
            sa = SIGMA0 * SIGMAK ** -1
            sb = 0.5 * 2.0 ** (-OMIN)
            lev0 = smooth(upsample(im), math.sqrt(sa * sa - sb * sb))
        else:
            lev0 = base[::2, ::2][:h, :w].copy()
        levels = [lev0]
        for s in range(0, S + 2):
            levels.append(smooth(levels[-1], DSIGMA0 * SIGMAK ** s))
        L = np.stack(levels)
        base = L[2 + 1]  # level s = 2
        yield o, L


def extrema(D):
    """Candidates (s, y, x) of D [5, h, w] (index = s + 1) in scan order: s, then y, then x."""
    _, h, w = D.shape
    c = D[1:4, 1:h - 1, 1:w - 1]
    gt = c >= 0
    lt = c <= 0
    for ds in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if ds == dy == dx == 0:
                    continue
                n = D[1 + ds:4 + ds, 1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
                gt &= c > n
                lt &= c < n
    s, y, x = np.nonzero(gt | lt)
    return s, y + 1, x + 1


def refine(D, s, x, y, w, h, report=None):
    """vlfeat's refinement of one candidate: None or (xn, yn, sn, integer s).  `report` (a dict) receives
    what happened: moved (the sample point left the candidate's pixel), and for a rejected candidate
    which tests it failed: value, edge (the score), offset, bounds."""
    b = [0.0, 0.0, 0.0]
    dx = dy = 0
    x0, y0 = x, y
    for _ in range(5):
        x += dx
        y += dy
        P = D[s + 1]

        def at(ix, iy, isd):
            return D[s + 1 + isd, y + iy, x + ix]
        c = float(P[y, x])
        Dx = 0.5 * float(at(1, 0, 0) - at(-1, 0, 0))
        Dy = 0.5 * float(at(0, 1, 0) - at(0, -1, 0))
        Ds = 0.5 * float(at(0, 0, 1) - at(0, 0, -1))
        Dxx = float(at(1, 0, 0) + at(-1, 0, 0)) - 2.0 * c
        Dyy = float(at(0, 1, 0) + at(0, -1, 0)) - 2.0 * c
        Dss = float(at(0, 0, 1) + at(0, 0, -1)) - 2.0 * c
        Dxy = 0.25 * float(at(1, 1, 0) + at(-1, -1, 0) - at(-1, 1, 0) - at(1, -1, 0))
        Dxs = 0.25 * float(at(1, 0, 1) + at(-1, 0, -1) - at(-1, 0, 1) - at(1, 0, -1))
        Dys = 0.25 * float(at(0, 1, 1) + at(0, -1, -1) - at(0, -1, 1) - at(0, 1, -1))
        A = [[Dxx, Dxy, Dxs], [Dxy, Dyy, Dys], [Dxs, Dys, Dss]]
        b = [-Dx, -Dy, -Ds]
        for j in range(3):
            maxa, maxabsa, maxi = 0.0, 0.0, -1
            for i in range(j, 3):
                if abs(A[i][j]) > maxabsa:
                    maxa, maxabsa, maxi = A[i][j], abs(A[i][j]), i
            if maxabsa < float(F32(1e-10)):
                b = [0.0, 0.0, 0.0]
                break
            i = maxi
            for jj in range(j, 3):
                A[i][jj], A[j][jj] = A[j][jj], A[i][jj]
                A[j][jj] /= maxa
            b[i], b[j] = b[j], b[i]
            b[j] /= maxa
            for ii in range(j + 1, 3):
                t = A[ii][j]
                for jj in range(j, 3):
                    A[ii][jj] -= t * A[j][jj]
                b[ii] -= t * b[j]
        for i in (2, 1):
            t = b[i]
            for ii in range(i - 1, -1, -1):
                b[ii] -= t * A[ii][i]
        dx = (1 if (b[0] > 0.6 and x < w - 2) else 0) + (-1 if (b[0] < -0.6 and x > 1) else 0)
        dy = (1 if (b[1] > 0.6 and y < h - 2) else 0) + (-1 if (b[1] < -0.6 and y > 1) else 0)
        if dx == 0 and dy == 0:
            break
    val = c + 0.5 * (Dx * b[0] + Dy * b[1] + Ds * b[2])
    with np.errstate(divide="ignore", invalid="ignore"):
        score = float(np.float64((Dxx + Dyy) * (Dxx + Dyy)) / np.float64(Dxx * Dyy - Dxy * Dxy))
    xn, yn, sn = x + b[0], y + b[1], s + b[2]
    good = (abs(val) > 0 and score < 12.1 and score >= 0 and abs(b[0]) < 1.5 and abs(b[1]) < 1.5
            and abs(b[2]) < 1.5 and 0 <= xn <= w - 1 and 0 <= yn <= h - 1 and -1 <= sn <= S + 1)
    if report is not None:
        report.update(moved=(x, y) != (x0, y0), value=not abs(val) > 0, edge=not (score < 12.1 and score >= 0),
                      offset=not (abs(b[0]) < 1.5 and abs(b[1]) < 1.5 and abs(b[2]) < 1.5),
                      bounds=not (0 <= xn <= w - 1 and 0 <= yn <= h - 1 and -1 <= sn <= S + 1))
    return (xn, yn, sn, s) if good else None


def fast_resqrt(x):
    x = np.asarray(x, np.float32)
    xhalf = F32(0.5) * x
    y = (np.int32(0x5f3759df) - (x.view(np.int32) >> 1)).view(np.float32)
    y = y * (F32(1.5) - xhalf * y * y)
    y = y * (F32(1.5) - xhalf * y * y)
    return y


def fast_sqrt(x):
    x = np.asarray(x, np.float32)
    return np.where(x.astype(np.float64) < 1e-8, F32(0), x * fast_resqrt(x)).astype(np.float32)


def fast_atan2(y, x):
    ay = np.abs(y) + F32(FLT_EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(x >= 0, (x - ay) / (x + ay), (x + ay) / (ay - x)).astype(np.float32)
    a = np.where(x >= 0, F32(math.pi / 4), F32(3 * math.pi / 4)).astype(np.float32)
    a = a + (F32(0.1821) * r * r - F32(0.9675)) * r
    return np.where(y < 0, -a, a).astype(np.float32)


def mod2pi(x):
    x = np.array(x, np.float32, ndmin=1)
    while True:
        m = x > TWO_PI_F
        if not m.any():
            break
        x[m] -= TWO_PI_F
    while True:
        m = x < 0
        if not m.any():
            break
        x[m] += TWO_PI_F
    return x


def gradient_xy(L):
    """(gx, gy) float32 [h, w] of one level: central differences, one-sided at the border."""
    gx = np.empty_like(L)
    gy = np.empty_like(L)
    gx[:, 1:-1] = F32(0.5) * (L[:, 2:] - L[:, :-2])
    gx[:, 0] = L[:, 1] - L[:, 0]
    gx[:, -1] = L[:, -1] - L[:, -2]
    gy[1:-1] = F32(0.5) * (L[2:] - L[:-2])
    gy[0] = L[1] - L[0]
    gy[-1] = L[-1] - L[-2]
    return gx, gy


def gradient(L):
    """(mod, ang) float32 [h, w] of one level."""
    gx, gy = gradient_xy(L)
    mod = fast_sqrt(gx * gx + gy * gy)
    ang = mod2pi((fast_atan2(gy, gx).astype(np.float64) + 2 * math.pi).astype(np.float32))
    return mod, ang.reshape(L.shape)


def fast_expn(x):
    x = np.asarray(x, np.float64)
    big = x > 25.0
    t = np.where(big, 0.0, x) * (256 / 25.0)
    i = np.floor(t).astype(np.int64)
    r = t - i
    a, b = EXPN_TAB[i], EXPN_TAB[np.minimum(i + 1, 256)]
    return np.where(big, 0.0, a + r * (b - a))


def orientations(mod, ang, kx, ky, ksigma, o):
    """Up to four angles (double) in histogram-bin order."""
    h, w = mod.shape
    xper = 2.0 ** o
    x, y, sigma = float(kx) / xper, float(ky) / xper, float(ksigma) / xper
    xi, yi = int(x + 0.5), int(y + 0.5)
    sigmaw = 1.5 * sigma
    W = max(int(math.floor(3.0 * sigmaw)), 1)
    ys = np.arange(max(-W, -yi), min(W, h - 1 - yi) + 1)
    xs = np.arange(max(-W, -xi), min(W, w - 1 - xi) + 1)
    YS, XS = np.meshgrid(ys, xs, indexing="ij")
    dx = (xi + XS).astype(np.float64) - x
    dy = (yi + YS).astype(np.float64) - y
    r2 = dx * dx + dy * dy
    keep = (r2 < W * W + 0.6).ravel()
    r2 = r2.ravel()[keep]
    py, px = (yi + YS).ravel()[keep], (xi + XS).ravel()[keep]
    wgt = fast_expn(r2 / (2 * sigmaw * sigmaw))
    m = mod[py, px].astype(np.float64)
    fbin = 36 * ang[py, px].astype(np.float64) / (2 * math.pi)
    b = np.floor(fbin - 0.5).astype(np.int64)
    rb = fbin - b - 0.5
    idx = np.stack([(b + 36) % 36, (b + 1) % 36], 1).ravel()
    val = np.stack([(1 - rb) * m * wgt, rb * m * wgt], 1).ravel()
    hist = np.zeros(36, np.float64)
    np.add.at(hist, idx, val)
    hist = hist.tolist()
    for _ in range(6):
        prev, first = hist[35], hist[0]
        for i in range(35):
            newh = (prev + hist[i] + hist[i + 1]) / 3.0
            prev = hist[i]
            hist[i] = newh
        hist[35] = (prev + hist[35] + first) / 3.0
    maxh = 0.0
    for v in hist:
        maxh = max(maxh, v)
    angles = []
    for i in range(36):
        h0, hm, hp = hist[i], hist[(i - 1 + 36) % 36], hist[(i + 1) % 36]
        if h0 > 0.8 * maxh and h0 > hm and h0 > hp:
            di = -0.5 * (hp - hm) / (hp + hm - 2 * h0)
            angles.append(2 * math.pi * (i + di + 0.5) / 36)
            if len(angles) == 4:
                break
    return angles


def normalize(d):
    norm = F32(0)
    for v in d:
        norm = F32(norm + F32(v * v))
    norm = F32(fast_sqrt(norm) + F32(FLT_EPS))
    return (d / norm).astype(np.float32)


def descriptor(mod, ang, kx, ky, ksigma, o, angle0):
    """The 128 float32 values before quantisation."""
    h, w = mod.shape
    xper = 2.0 ** o
    x, y, sigma = float(kx) / xper, float(ky) / xper, float(ksigma) / xper
    xi, yi = int(x + 0.5), int(y + 0.5)
    st0, ct0 = math.sin(angle0), math.cos(angle0)
    SBP = 3.0 * sigma + DBL_EPS
    W = int(math.floor(math.sqrt(2.0) * SBP * 5 / 2.0 + 0.5))
    dys = np.arange(max(-W, 1 - yi), min(W, h - yi - 2) + 1)
    dxs = np.arange(max(-W, 1 - xi), min(W, w - xi - 2) + 1)
    out = np.zeros(128, np.float32)
    if len(dys) == 0 or len(dxs) == 0:
        return _normalize_twice(out)
    DY, DX = np.meshgrid(dys, dxs, indexing="ij")
    py, px = (yi + DY).ravel(), (xi + DX).ravel()
    m = mod[py, px]
    theta = mod2pi((ang[py, px].astype(np.float64) - angle0).astype(np.float32))
    dx = (px.astype(np.float64) - x).astype(np.float32).astype(np.float64)
    dy = (py.astype(np.float64) - y).astype(np.float32).astype(np.float64)
    nx = ((ct0 * dx + st0 * dy) / SBP).astype(np.float32)
    ny = ((-st0 * dx + ct0 * dy) / SBP).astype(np.float32)
    nt = ((F32(8) * theta).astype(np.float64) / (2 * math.pi)).astype(np.float32)
    win = fast_expn((nx * nx + ny * ny).astype(np.float64) / 8.0).astype(np.float32)
    bx = np.floor((nx.astype(np.float64) - 0.5).astype(np.float32)).astype(np.int64)
    by = np.floor((ny.astype(np.float64) - 0.5).astype(np.float32)).astype(np.int64)
    bt = np.floor(nt).astype(np.int64)
    rbx = (nx.astype(np.float64) - (bx + 0.5)).astype(np.float32)
    rby = (ny.astype(np.float64) - (by + 0.5)).astype(np.float32)
    rbt = (nt - bt.astype(np.float32)).astype(np.float32)
    wm = win * m
    idx, val = [], []
    for dbx in (0, 1):
        for dby in (0, 1):
            for dbt in (0, 1):
                ok = (bx + dbx >= -2) & (bx + dbx < 2) & (by + dby >= -2) & (by + dby < 2)
                wgt = wm * np.abs(F32(1 - dbx) - rbx) * np.abs(F32(1 - dby) - rby) * np.abs(F32(1 - dbt) - rbt)
                idx.append(np.where(ok, (by + dby + 2) * 32 + (bx + dbx + 2) * 8 + (bt + dbt) % 8, -1))
                val.append(wgt.astype(np.float32))
    # one bin receives at most one value per pixel, so pixel-major order is raster order per bin
    idx = np.stack(idx, 1).ravel()
    val = np.stack(val, 1).ravel()
    keep = idx >= 0
    np.add.at(out, idx[keep], val[keep])
    return _normalize_twice(out)


def _normalize_twice(d):
    d = normalize(d)
    d = np.where(d.astype(np.float64) > 0.2, F32(0.2), d).astype(np.float32)
    return normalize(d)


def keypoints(im):
    """Yields (o, levels, (x, y, sigma) float32, integer s) in vlfeat's order."""
    for o, L in octaves(im):
        h, w = L.shape[1:]
        D = L[1:] - L[:-1]
        xper = 2.0 ** o
        for s, y, x in zip(*extrema(D)):
            r = refine(D, int(s), int(x), int(y), w, h)
            if r is None:
                continue
            xn, yn, sn, si = r
            yield o, L, (F32(xn * xper), F32(yn * xper), F32(SIGMA0 * 2.0 ** (sn / S) * xper)), si


def sift(im):
    """float32 [nkp, 132]: x, y, sigma, angle, then (uint8) min(512 d, 255) per descriptor value."""
    im = np.ascontiguousarray(im, np.float32)
    if im.ndim != 2:
        raise TypeError("Only 2d images are supported.")
    rows = []
    grads, grad_key = None, None
    for o, L, (kx, ky, ks), si in keypoints(im):
        if grad_key != o:
            grads = [gradient(L[s + 1]) for s in range(3)]
            grad_key = o
        mod, ang = grads[si]
        for a in orientations(mod, ang, kx, ky, ks, o):
            d = descriptor(mod, ang, kx, ky, ks, o, a)
            q = np.minimum(F32(512) * d, F32(255)).astype(np.uint8).astype(np.float32)
            rows.append(np.concatenate([np.array([kx, ky, ks, F32(a)], np.float32), q]))
    return np.array(rows, np.float32).reshape(-1, 132)
