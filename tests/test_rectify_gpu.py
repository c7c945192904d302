"""image_pair_rectification on the GPU (mvg.image_pair_rectification through the host-pointer C-ABI,
device.image_pair_rectification with resident tensors) against the numpy statement of the contract,
tests/rectify_oracle.py, driven by the library's own F: values compared bit for bit (as uint64 for
float64), indices exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rectify_oracle as ro

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The kernel instantiations rectify_run launches (spectavi_amd/csrc/rectify.hip): rectify_kernel<T> with
# T = uint64_t for float64 images (values moved as bits) and uint8_t for 8-bit ones (device form only).
INSTANTIATED = {"rectify_kernel<unsigned long>", "rectify_kernel<unsigned char>"}
KERNEL_OF = {np.float64: "rectify_kernel<unsigned long>", np.uint8: "rectify_kernel<unsigned char>"}


def camera(f, c, R=np.eye(3), t=(0., 0., 0.)):
    K = np.array([[f, 0., c[0]], [0., f, c[1]], [0., 0., 1.]])
    return K @ np.hstack([R, np.asarray(t, np.float64)[:, None]])


def rot(rng, s):
    a = rng.standard_normal(3) * s
    A = np.array([[0., -a[2], a[1]], [a[2], 0., -a[0]], [-a[1], a[0], 0.]])
    q = np.linalg.qr(np.eye(3) + A)[0]
    return q * np.sign(np.diag(q))[None, :]


def pair(rng, hgt, wid, baseline=(-0.25, 0.01, 0.02), f=None):
    f = f or 1.1 * max(hgt, wid)
    c = (wid / 2. + 3.3, hgt / 2. - 1.7)
    return camera(f, c), camera(f, c, rot(rng, 0.01), baseline)


def image(rng, hgt, wid, nchan, dtype=np.float64, specials=True):
    shp = (hgt, wid) if nchan == 1 else (hgt, wid, nchan)
    if dtype == np.uint8:
        return rng.integers(0, 256, shp, dtype=np.uint8)
    im = rng.standard_normal(shp) * 100
    if specials:  # NaN payloads, -0.0, +-inf: copied, never computed
        bits = im.reshape(-1).view(np.uint64)
        bits[::5] = 0x7FF8DEADBEEF0001
        bits[1::7] = 0xFFF0000000000F0F
        bits[2::11] = 0x8000000000000000
        bits[3::13] = 0xFFF0000000000000
    return im


def bits(a):
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want):
    for name, g, w in zip(("r0", "r1", "ri0", "ri1"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (name, g.shape, w.shape, g.dtype, w.dtype)
        bad = np.argwhere(bits(g) != bits(w))
        assert bad.size == 0, "%s differs at %s: got %s want %s" % (name, bad[:3].tolist(), g[tuple(bad[0])],
                                                                    w[tuple(bad[0])])


def device_run(P0, P1, im0, im1, sf):
    import torch
    from spectavi_amd import device
    t0, t1 = torch.from_numpy(im0).cuda(), torch.from_numpy(im1).cuda()
    out = device.image_pair_rectification(P0, P1, t0, t1, sampling_factor=sf)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def self_check(im, r, ri):
    nchan = 1 if im.ndim == 2 else im.shape[2]
    ok = ri >= 0
    assert np.array_equal(bits(r.reshape(-1, nchan)[ok.reshape(-1)]), bits(im.reshape(-1, nchan)[ri[ok]]))
    assert not bits(r.reshape(-1, nchan)[~ok.reshape(-1)]).any()


def check_case(P0, P1, im0, im1, sf, expect_valid=None):
    """host ABI (crop off and on) == device form == oracle on the library's F; returns the oracle result."""
    from spectavi_amd import mvg
    F = mvg.rectification_fundamental(P0, P1)
    want = ro.rectify(F, im0, im1, sf)
    if im0.dtype == np.float64:
        assert_same(mvg.image_pair_rectification(P0, P1, im0, im1, sampling_factor=sf, crop_invalid=False), want)
    assert_same(device_run(P0, P1, im0, im1, sf), want)
    for im, r, ri in ((im0, want[0], want[2]), (im1, want[1], want[3])):
        self_check(im, r, ri)
    nvalid = int((want[2] >= 0).sum() + (want[3] >= 0).sum())
    if expect_valid is not None:
        assert (nvalid > 0) == expect_valid
    if im0.dtype == np.float64:
        if nvalid:
            assert_same(mvg.image_pair_rectification(P0, P1, im0, im1, sampling_factor=sf), ro.crop(*want))
        else:
            with pytest.raises(ValueError):
                mvg.image_pair_rectification(P0, P1, im0, im1, sampling_factor=sf)
    return want


# (name, hgt, wid, nchan, sf, camera kind, dtypes) -- the kernel instantiations each case reaches are
# KERNEL_OF[dtype] for its dtypes
CASES = [
    ("stereo_gray", 120, 200, 1, 1.2, "stereo", (np.float64, np.uint8)),
    ("stereo_rgb", 90, 130, 3, 1.2, "stereo", (np.float64, np.uint8)),
    ("stereo_downsample", 100, 150, 1, 0.5, "stereo", (np.float64,)),
    ("baseline_y", 64, 96, 1, 1.2, "vertical", (np.float64, np.uint8)),
    ("baseline_y_exact", 64, 96, 3, 1.2, "vertical_exact", (np.float64,)),
    ("identical", 40, 50, 1, 1.2, "identical", (np.float64, np.uint8)),
    ("rank_deficient", 40, 50, 3, 1.2, "rank_deficient", (np.float64,)),
    ("wid1_rnx1", 9, 1, 1, 1.2, "stereo", (np.float64, np.uint8)),
    ("rnx1_inf_delta", 9, 2, 1, 0.5, "stereo", (np.float64,)),
    ("sf07_rgb_w30", 20, 30, 3, 0.7, "stereo", (np.float64, np.uint8)),
    ("sf07_rgb_w90", 20, 90, 3, 0.7, "stereo", (np.float64, np.uint8)),
    ("ragged_77x131", 77, 131, 1, 1.3, "stereo", (np.float64,)),
    ("tall", 301, 47, 1, 2.2, "stereo", (np.float64, np.uint8)),
    ("wide", 33, 517, 2, 1.0, "stereo", (np.float64,)),
]


def test_case_table_reaches_every_instantiation():
    assert {KERNEL_OF[d] for c in CASES for d in c[6]} == INSTANTIATED


def test_kernel_coverage_lists_the_instantiations():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_coverage.py"), "--list",
                          "--files", "rectify.hip"], check=True, capture_output=True, text=True).stdout
    listed = {ln.strip() for ln in out.splitlines() if ln.startswith("  ")}
    assert listed == INSTANTIATED, out


def cameras(kind, rng, hgt, wid):
    if kind == "stereo":
        return pair(rng, hgt, wid)
    if kind == "vertical":  # steep lines: y far outside the image on most samples
        return pair(rng, hgt, wid, baseline=(0.02, -0.3, 0.))
    if kind == "vertical_exact":  # |l_1| tiny against l_0 x: y far out of range but on a few samples
        return pair(rng, hgt, wid, baseline=(0., -0.3, 0.))
    P0, P1 = pair(rng, hgt, wid)
    if kind == "identical":
        return P0, P0.copy()
    if kind == "rank_deficient":
        return np.vstack([P0[:2], P0[:1] * 2.]), P1
    raise ValueError(kind)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_case(case):
    name, hgt, wid, nchan, sf, kind, dtypes = case
    rng = np.random.default_rng([hgt, wid, nchan, int(sf * 10)])
    P0, P1 = cameras(kind, rng, hgt, wid)
    expect = {"identical": False, "rank_deficient": False, "vertical_exact": None}.get(
        kind, wid > 1 and int(sf * wid) > 1)
    for dt in dtypes:
        im0, im1 = image(rng, hgt, wid, nchan, dt), image(rng, hgt, wid, nchan, dt)
        if dt == np.uint8:  # same values as float64: same indices, values equal the float64 ones cast
            f0, f1 = im0.astype(np.float64), im1.astype(np.float64)
            u = check_case(P0, P1, im0, im1, sf, expect)
            f = device_run(P0, P1, f0, f1, sf)
            assert np.array_equal(u[2], f[2]) and np.array_equal(u[3], f[3])
            assert np.array_equal(u[0], f[0].astype(np.uint8)) and np.array_equal(u[1], f[1].astype(np.uint8))
            assert np.array_equal(u[0].astype(np.float64), f[0]) and np.array_equal(u[1].astype(np.float64), f[1])
        else:
            check_case(P0, P1, im0, im1, sf, expect)


def test_baseline_y_reaches_huge_and_nonfinite_y():
    """A vertical baseline makes the lines vertical: l_1 ~ 0, y huge or inf / NaN (from 0/0) on some rows."""
    from spectavi_amd import mvg
    rng = np.random.default_rng(7)
    P0, P1 = pair(rng, 64, 96, baseline=(0., -0.3, 0.))
    F = mvg.rectification_fundamental(P0, P1)
    F0 = F.copy()
    F0[:, 1] = 0.  # l_1 = 0 exactly on every row: y = +-inf or NaN
    im0, im1 = image(rng, 64, 96, 1), image(rng, 64, 96, 1)
    # through the device form with F given directly
    import torch
    from spectavi_amd import device
    from spectavi_amd._lib import clib, check
    t0, t1 = torch.from_numpy(im0).cuda(), torch.from_numpy(im1).cuda()
    rows, cols, _ = mvg.rectification_shape(96, 64, 1, 1.2)
    outs = [torch.empty((rows, cols), dtype=torch.float64, device="cuda") for _ in range(2)]
    outs += [torch.empty((rows, cols), dtype=torch.int32, device="cuda") for _ in range(2)]
    for FF in (F, F0):
        with device._on_device_of(t0, t1) as stream:
            check(clib.spv_rectify_device(np.ascontiguousarray(FF.reshape(-1)), t0.data_ptr(), t1.data_ptr(), 0, 96,
                                          64, 1, 1.2, *[o.data_ptr() for o in outs], stream))
        torch.cuda.synchronize()
        assert_same(tuple(o.cpu().numpy() for o in outs), ro.rectify(FF, im0, im1, 1.2))
    assert (ro.rectify(F0, im0, im1, 1.2)[2] == -1).all()


def test_1080p_gray_and_rgb():
    """The benchmark's shape: 1920 x 1080, sf = 1.2, gray and 3-channel, float64 and uint8."""
    rng = np.random.default_rng(1080)
    P0, P1 = pair(rng, 1080, 1920)
    for nchan in (1, 3):
        im0, im1 = image(rng, 1080, 1920, nchan, specials=False), image(rng, 1080, 1920, nchan, specials=False)
        want = check_case(P0, P1, im0, im1, 1.2, True)
        assert (want[2] >= 0).mean() > 0.05 and (want[3] >= 0).mean() > 0.05
        u0, u1 = image(rng, 1080, 1920, nchan, np.uint8), image(rng, 1080, 1920, nchan, np.uint8)
        from spectavi_amd import mvg
        assert_same(device_run(P0, P1, u0, u1, 1.2), ro.rectify(mvg.rectification_fundamental(P0, P1), u0, u1, 1.2))


def test_profile_name():
    import torch
    from spectavi_amd import device
    rng = np.random.default_rng(3)
    P0, P1 = pair(rng, 32, 48)
    device.profile_reset()
    device.profile_enable(True)
    device_run(P0, P1, image(rng, 32, 48, 1), image(rng, 32, 48, 1), 1.2)
    device.profile_enable(False)
    n, ms = device.profile_read("rectify")
    assert n == 1 and ms > 0
    torch.cuda.synchronize()
