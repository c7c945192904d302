"""numpy statement of the image_pair_rectification contract (include/spectavi_amd.h): the fundamental
matrix of rule 1, the output shape, and the resampling of both images along their epipolar lines.

Every line is computed with explicit elementwise products and sums in the stated order (never `@`
or BLAS, whose order is not fixed), so its bits are the contract's bits; values are moved as uint64
(or uint8) views, so NaN payloads and -0.0 survive.  `literal` is a per-sample Python transcription
of the reference's Rectifier loop, against which the vectorised form is checked."""
import math

import numpy as np

INT_MIN = -2**31


def fundamental(P0, P1):
    """F = [P1 C]x P1 P0^T (P0 P0^T)^-1, C the unit null vector of P0 (rule 1; bits not contractual)."""
    P0 = np.asarray(P0, np.float64)
    P1 = np.asarray(P1, np.float64)
    C = np.linalg.svd(P0)[2][3]
    e = P1 @ C
    ex = np.array([[0., -e[2], e[1]], [e[2], 0., -e[0]], [-e[1], e[0], 0.]])
    return ex @ P1 @ P0.T @ np.linalg.inv(P0 @ P0.T)


def shape(wid, hgt, nchan, sf):
    """(output_rows, output_cols, rnx): the reference's expressions in double, truncated to int."""
    C = wid * nchan
    cols = int(sf * float(C) / float(nchan))
    extra = int(float(max(hgt, C)) / 2.)
    return hgt + 2 * extra, cols, int(sf * float(wid))


def dims(im):
    return (im.shape[0], im.shape[1], 1) if im.ndim == 2 else im.shape


def as_bits(im):
    im = np.ascontiguousarray(im)
    return im.view(np.uint64) if im.dtype.itemsize == 8 else im


def _sample(x, y, wid, hgt, bits, nchan):
    """Rule 5 on arrays x [n] / y [R, n]: (values [R, n, nchan] of bits' dtype, idx int32 [R, n])."""
    with np.errstate(invalid="ignore"):
        ok = (x > -1.) & (x < float(wid)) & (y > -1.) & (y < float(hgt))
    px = np.where(ok, x, 0.).astype(np.int64)  # truncation toward zero, on valid samples only
    py = np.where(ok, y, 0.).astype(np.int64)
    idx = np.where(ok, py * wid + px, -1)
    flat = bits.reshape(hgt * wid, nchan)
    vals = np.where(ok[..., None], flat[np.where(ok, idx, 0)], np.zeros((), bits.dtype))
    return vals, idx.astype(np.int32)


def rectify(F, im0, im1, sf):
    """Rules 2-6 given F: (r0, r1, ri0, ri1) uncropped, values as the images' dtype (float64 bits kept)."""
    hgt, wid, nchan = dims(im0)
    rows, cols, rnx = shape(wid, hgt, nchan, sf)
    extra = (rows - hgt) // 2
    F = np.asarray(F, np.float64)
    b0, b1 = as_bits(im0), as_bits(im1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        delta = (np.float64(wid - 1) - 0.) / np.float64(rnx - 1)
        x = 0. + np.arange(rnx, dtype=np.float64) * delta
        v = (np.arange(rows, dtype=np.int64) - extra).astype(np.float64)
        l0, l1, l2 = ((F[0, j] * 0. + F[1, j] * v) + F[2, j] for j in range(3))
        y0 = ((-l2)[:, None] - (l0[:, None] * x[None, :])) / l1[:, None]
        sx, sy = x[0], y0[:, 0]
        m0, m1, m2 = ((F[j, 0] * sx + F[j, 1] * sy) + F[j, 2] for j in range(3))
        y1 = ((-m2)[:, None] - (m0[:, None] * x[None, :])) / m1[:, None]
    n = min(rnx, cols)
    outs = []
    for y, bits in ((y0, b0), (y1, b1)):
        vals = np.zeros((rows, cols, nchan), bits.dtype)
        idx = np.full((rows, cols), -1, np.int32)
        vals[:, :n], idx[:, :n] = _sample(x[:n], y[:, :n], wid, hgt, bits, nchan)
        outs.append((vals, idx))
    (v0, i0), (v1, i1) = outs
    if nchan == 1:
        v0, v1 = v0[..., 0], v1[..., 0]
    if im0.dtype == np.float64:
        v0, v1 = v0.view(np.float64), v1.view(np.float64)
    return v0, v1, i0, i1


def crop(r0, r1, ri0, ri1):
    """The front-end's crop_invalid: the bounding box of the samples valid in either image."""
    y, x = np.where((ri0 != -1) | (ri1 != -1))
    if y.size == 0:
        raise ValueError("no valid sample")
    ys, xs = slice(y.min(), y.max() + 1), slice(x.min(), x.max() + 1)
    return r0[ys, xs, ...], r1[ys, xs, ...], ri0[ys, xs], ri1[ys, xs]


# ---- literal transcription of the reference's loop, one sample at a time ---------------------------
def _cvtt(x):
    """(int)x as x86's cvttsd2si computes it: truncation, INT_MIN for NaN and out-of-range values."""
    if math.isnan(x) or math.isinf(x):
        return INT_MIN
    t = math.trunc(x)
    return t if -2**31 <= t < 2**31 else INT_MIN


def _div(a, b):
    """IEEE double a / b (Python raises on / 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.float64(a) / np.float64(b))


def literal(F, im0, im1, sf):
    """Rectifier::resample (reference src/Camera.h:253-326) with Python floats, as the reference's loop
    writes it: each row's samples into a flat buffer from the row's start (so samples past output_cols
    spill into the next row, which is rewritten after), the index built from (int)x and (int)y."""
    hgt, wid, nchan = dims(im0)
    C = wid * nchan
    cols = int(sf * float(C) / float(nchan))
    extra = int(float(max(hgt, C)) / 2.)
    rows = hgt + 2 * extra
    nx = C // nchan
    rnx = int(sf * float(nx))
    F = [[float(F[r][c]) for c in range(3)] for r in range(3)]
    spill = nchan * max(rnx, 1)
    flat = [as_bits(im).reshape(-1).tolist() for im in (im0, im1)]
    rim = [[0] * (rows * cols * nchan + spill) for _ in range(2)]
    rid = [[-1] * (rows * cols + spill) for _ in range(2)]
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = _div(float(nx - 1) - 0., float(rnx - 1))
    xx = [0. + float(i) * delta for i in range(rnx)]

    def resample(img, line, target):
        l0, l1, l2 = line
        for i in range(rnx):
            x = xx[i]
            y = _div((-l2) - (l0 * x), l1)
            _x, _y = _cvtt(x), _cvtt(y)
            ok = 0 <= _x < wid and 0 <= _y < hgt
            rid[img][target * cols + i] = _y * wid + _x if ok else -1
            for c in range(nchan):
                rim[img][(target * cols + i) * nchan + c] = flat[img][(_y * wid + _x) * nchan + c] if ok else 0
        return _div((-l2) - (l0 * xx[0]), l1) if rnx else float("nan")

    for irow in range(-extra, hgt + extra):
        v = float(irow)
        line = [(F[0][j] * 0. + F[1][j] * v) + F[2][j] for j in range(3)]
        sy = resample(0, line, irow + extra)
        sx = xx[0]
        seed_line = [(F[j][0] * sx + F[j][1] * sy) + F[j][2] for j in range(3)]
        resample(1, seed_line, irow + extra)
    dt = np.uint64 if im0.dtype == np.float64 else im0.dtype
    vshape = (rows, cols) if nchan == 1 else (rows, cols, nchan)
    out = []
    for img in (0, 1):
        vals = np.array(rim[img][:rows * cols * nchan], dtype=dt).reshape(vshape)
        out.append(vals.view(np.float64) if im0.dtype == np.float64 else vals)
    return out[0], out[1], np.array(rid[0][:rows * cols], np.int32).reshape(rows, cols), \
        np.array(rid[1][:rows * cols], np.int32).reshape(rows, cols)
