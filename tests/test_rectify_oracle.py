"""CPU checks of image_pair_rectification: the numpy oracle (tests/rectify_oracle.py) against a literal
per-sample transcription of the reference's loop, the library's host-only shape and fundamental-matrix
functions against the oracle, argument rejection, and the exported symbols.  No GPU involved."""
import ctypes as ct
import os

import numpy as np
import pytest

from tests import rectify_oracle as ro

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def camera(rng, f=800., c=(40., 30.), t=(0., 0., 0.), rot=0.0):
    K = np.array([[f, 0., c[0]], [0., f, c[1]], [0., 0., 1.]])
    a = rng.standard_normal(3) * rot
    Ax = np.array([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]])
    R = np.linalg.qr(np.eye(3) + Ax)[0]
    R *= np.sign(np.diag(R))[None, :]
    return K @ np.hstack([R, np.asarray(t, np.float64)[:, None]])


def stereo(rng, baseline=(-0.2, 0.01, 0.005), **kw):
    return camera(rng, **kw), camera(rng, t=baseline, rot=0.02, **kw)


@pytest.mark.parametrize("hgt,wid,nchan,sf", [(7, 9, 1, 1.2), (9, 7, 1, 0.5), (6, 10, 3, 0.7), (5, 5, 3, 1.7),
                                              (8, 1, 1, 1.2), (3, 11, 2, 2.2), (10, 30, 3, 0.7)])
def test_oracle_equals_literal_loop(hgt, wid, nchan, sf):
    rng = np.random.default_rng([hgt, wid, nchan, int(sf * 10)])
    P0, P1 = stereo(rng, c=(wid / 2., hgt / 2.), f=20.)
    shp = (hgt, wid) if nchan == 1 else (hgt, wid, nchan)
    im0, im1 = rng.standard_normal(shp), rng.standard_normal(shp)
    im0.reshape(-1)[::7] = -0.0
    F = ro.fundamental(P0, P1)
    got = ro.rectify(F, im0, im1, sf)
    want = ro.literal(F, im0, im1, sf)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                              w.view(np.uint64) if w.dtype == np.float64 else w)
    if wid > 1:  # (wid = 1: rnx = 1, delta and x_0 are NaN, every sample is invalid)
        assert (got[2] >= 0).any() and (got[2] == -1).any()  # the case has valid and invalid samples
    else:
        assert (got[2] == -1).all() and (got[3] == -1).all()


def test_oracle_equals_literal_loop_edge_lines():
    """Lines through inf / NaN: a baseline along y (vertical lines) and F with zero entries."""
    rng = np.random.default_rng(5)
    P0, P1 = stereo(rng, baseline=(0., -0.3, 0.), c=(4., 3.), f=10.)
    im0, im1 = rng.standard_normal((6, 8)), rng.standard_normal((6, 8))
    for F in (ro.fundamental(P0, P1), np.diag([0., 1., 1.]), np.array([[0., 0., 1.], [0., 0., 0.], [1., 0., 0.]])):
        got, want = ro.rectify(F, im0, im1, 1.2), ro.literal(F, im0, im1, 1.2)
        for g, w in zip(got, want):
            assert np.array_equal(g.view(np.uint64) if g.dtype == np.float64 else g,
                                  w.view(np.uint64) if w.dtype == np.float64 else w)


def test_shape_equals_rule_2():
    from spectavi_amd import mvg
    from spectavi_amd._lib import SpectaviError
    mismatched = 0
    for sf in (0.5, 0.7, 1.0, 1.2, 2.2):
        for nchan in (1, 3):
            for wid in range(1, 4097):
                for hgt in (1, 1080):
                    want = ro.shape(wid, hgt, nchan, sf)
                    if want[1] < 1 or want[2] < 1:
                        with pytest.raises(SpectaviError):
                            mvg.rectification_shape(wid, hgt, nchan, sf)
                        continue
                    assert mvg.rectification_shape(wid, hgt, nchan, sf) == want, (wid, hgt, nchan, sf)
                    mismatched += want[1] != want[2]
    assert mismatched > 0  # the rnx != output_cols cases are among them
    assert ro.shape(30, 20, 3, 0.7)[1:] == (20, 21) and ro.shape(90, 20, 3, 0.7)[1:] == (63, 62)


def test_fundamental_agrees_with_oracle():
    """Equal up to scale and sign, relative 1e-9 (max-abs normalised) on well-conditioned stereo pairs."""
    from spectavi_amd import mvg
    rng = np.random.default_rng(11)
    for trial in range(50):
        P0, P1 = stereo(rng, baseline=rng.standard_normal(3) * 0.3, c=(960., 540.), f=1000. + 500 * trial)
        if trial % 2:
            P0 = camera(rng, t=rng.standard_normal(3), rot=0.3, c=(960., 540.))
        got, want = mvg.rectification_fundamental(P0, P1), ro.fundamental(P0, P1)
        got, want = got / np.abs(got).max(), want / np.abs(want).max()
        k = np.argmax(np.abs(want))
        got *= np.sign(got.flat[k]) * np.sign(want.flat[k])
        assert np.abs(got - want).max() < 1e-9, trial


def test_fundamental_degenerate_cameras():
    from spectavi_amd import mvg
    rng = np.random.default_rng(12)
    P0, P1 = stereo(rng)
    assert np.array_equal(mvg.rectification_fundamental(P0, P0), np.zeros((3, 3)))       # shared centre
    assert np.array_equal(mvg.rectification_fundamental(P0, 3 * P0), np.zeros((3, 3)))
    for bad in (np.vstack([P0[:2], P0[:1]]), np.vstack([P0[:2], np.zeros((1, 4))]), np.full((3, 4), np.nan)):
        assert np.isnan(mvg.rectification_fundamental(bad, P1)).all()


def test_invalid_arguments():
    from spectavi_amd import mvg
    from spectavi_amd._lib import clib, SPV_ERR_INVALID, SpectaviError
    out = np.zeros(3, np.int32)
    for args in ((0, 5, 1, 1.2), (5, 0, 1, 1.2), (5, 5, 0, 1.2), (5, 5, 1, 0.), (5, 5, 1, -1.), (5, 5, 1, np.nan),
                 (5, 5, 1, np.inf), (1, 5, 1, 0.5), (3, 5, 3, 0.3), (65536, 32768, 1, 1.), (2**30, 1, 3, 1.)):
        assert mvg._spv_rectify_shape(*args, out) == SPV_ERR_INVALID, args
        with pytest.raises(SpectaviError):
            mvg.rectification_shape(*args)
    assert out.tolist() == [0, 0, 0]
    # the reference symbol rejects before any device work: nothing allocated, status INVALID
    P = np.zeros((3, 4))
    im = np.zeros((4, 4))
    r0, r1 = mvg.NdArray(), mvg.NdArray()
    ri0, ri1 = mvg.NdArray(dtype="int32"), mvg.NdArray(dtype="int32")
    mvg._image_pair_rectification(P, P, im, im, 4, 4, 1, 0.1, ct.byref(r0), ct.byref(r1), ct.byref(ri0), ct.byref(ri1))
    assert clib.spv_last_status() == SPV_ERR_INVALID and not r0.m_data and not ri1.m_data
    with pytest.raises(SpectaviError):
        mvg.image_pair_rectification(P, P, im, im, sampling_factor=0.1)
    # the device form checks its arguments before any launch.  A private function object (clib[name]):
    # the shared prototype takes F as a float64 array, here F and the images are raw addresses and NULL
    dev = clib["spv_rectify_device"]
    dev.restype = ct.c_int
    dev.argtypes = [ct.c_void_p] * 3 + [ct.c_int] * 4 + [ct.c_double] + [ct.c_void_p] * 5
    F = np.zeros(9)
    assert dev(F.ctypes.data, None, None, 0, 4, 4, 1, 1.2, None, None, None, None, None) == SPV_ERR_INVALID
    assert dev(F.ctypes.data, 8, 8, 7, 4, 4, 1, 1.2, 8, 8, 8, 8, None) == SPV_ERR_INVALID  # unknown dtype
    assert dev(F.ctypes.data, 8, 8, 0, 4, 4, 1, 0.1, 8, 8, 8, 8, None) == SPV_ERR_INVALID  # rnx = 0
    assert dev(F.ctypes.data, 4, 8, 0, 4, 4, 1, 1.2, 8, 8, 8, 8, None) == SPV_ERR_INVALID  # misaligned fp64


def test_frontend_type_errors():
    from spectavi_amd import mvg
    P = np.zeros((3, 4))
    with pytest.raises(TypeError):
        mvg.image_pair_rectification(P, P, np.zeros((4, 5)), np.zeros((5, 4)))
    with pytest.raises(TypeError):
        mvg.image_pair_rectification(P, P, np.zeros((4, 5, 3)), np.zeros((4, 5)))
    with pytest.raises(TypeError):
        mvg.image_pair_rectification(np.zeros((3, 3)), P, np.zeros((4, 5)), np.zeros((4, 5)))


def test_frontend_signature():
    import inspect
    from spectavi_amd import mvg
    sig = inspect.signature(mvg.image_pair_rectification)
    assert list(sig.parameters) == ["P0", "P1", "im0", "im1", "sampling_factor", "crop_invalid"]
    assert [p.default for p in sig.parameters.values()][4:] == [1.2, True]
    assert len(mvg._image_pair_rectification.argtypes) == 12


def test_every_symbol_the_reference_mvg_binds_is_exported():
    """The five C symbols that the reference's spectavi/mvg.py binds at import (listed here, the
    reference is not read): with all of them exported, it imports against this library alone."""
    from spectavi_amd._lib import clib
    for name in ("image_pair_rectification", "ransac_fitter", "seven_point_algorithm", "dlt_triangulate",
                 "dlt_reprojection_error"):
        assert hasattr(clib, name), name
    for name in ("spv_rectify_shape", "spv_rectify_fundamental", "spv_rectify_device"):
        assert hasattr(clib, name), name
