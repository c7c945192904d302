"""SIFT on the GPU against vlfeat's recorded table and the numpy oracle (tests/sift_oracle.py).

Bar: the same rows in the same order, every value bit-equal (x, y, sigma, angle and descriptors).  The
contract allows one float32 ulp on a frame value where the device's sin / cos / pow differ from the C
library's in the last bit; none of these cases needs it."""
import numpy as np
import pytest

from tests import sift_oracle as so
from tests.sift_cases import assert_tables_match, orientation_counts, smooth_random, sur_ogre

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def feature():
    from spectavi_amd import feature
    return feature


def test_vlfeat_parity_sur_ogre(feature):
    im, golden = sur_ogre()
    table = feature.sift_filter(im)
    assert table.shape == (1168, 132) and table.dtype == np.float32
    assert np.allclose(table[:, :4], golden[:, :4])
    assert np.array_equal(table[:, 4:], golden[:, 4:])


def test_sur_ogre_matches_oracle_and_has_four_orientations(feature):
    im, _ = sur_ogre()
    want = so.sift(im)
    got = feature.sift_filter(im)
    assert_tables_match(got, want, "sur-ogre")
    assert orientation_counts(got).max() == 4


@pytest.mark.parametrize("h,w,seed", [(17, 23, 1), (64, 64, 2), (233, 310, 3), (480, 641, 1)])
def test_random_images_match_oracle(feature, h, w, seed):
    im = smooth_random(seed, h, w)
    want = so.sift(im)
    assert len(want) > 0
    assert_tables_match(feature.sift_filter(im), want, "%dx%d" % (h, w))


def test_border_keypoints_match_oracle(feature):
    """Keypoints within 1.5 px of the right or bottom edge (64x64 seed 1, 480x641 seed 1)."""
    for (h, w) in ((64, 64), (480, 641)):
        im = smooth_random(1, h, w)
        want = so.sift(im)
        assert ((want[:, 0] > w - 1.5) | (want[:, 1] > h - 1.5)).any()
        assert_tables_match(feature.sift_filter(im), want, "border %dx%d" % (h, w))


def test_constant_image_gives_no_rows(feature):
    t = feature.sift_filter(np.full((100, 120), 42, np.float32))
    assert t.shape == (0, 132) and t.dtype == np.float32


def test_single_octave_image(feature):
    im = smooth_random(1, 12, 15)
    assert so.noctaves(15, 12) == 1
    want = so.sift(im)
    assert len(want) > 0
    assert_tables_match(feature.sift_filter(im), want, "12x15")


@pytest.mark.parametrize("h,w", [(1, 1), (1, 40), (2, 3), (5, 2)])
def test_tiny_images(feature, h, w):
    im = smooth_random(4, h, w, passes=0)
    assert_tables_match(feature.sift_filter(im), so.sift(im), "%dx%d" % (h, w))


def test_host_device_and_batch_forms_agree(feature):
    import torch
    from spectavi_amd import device
    ims = [smooth_random(5, 64, 80), np.full((30, 40), 3, np.float32), sur_ogre()[0], smooth_random(6, 17, 23)]
    host = [feature.sift_filter(im) for im in ims]
    assert len(host[1]) == 0 and all(len(t) > 0 for t in host[:1] + host[2:])
    batch = feature.sift_filter_batch(ims, nthread=3)
    dev = [device.sift(torch.from_numpy(im).cuda()).cpu().numpy() for im in ims]
    for i, (a, b, c) in enumerate(zip(host, batch, dev)):
        assert a.shape == b.shape == c.shape, i
        assert a.tobytes() == b.tobytes() == c.tobytes(), i


def test_device_table_feeds_split_and_normalize():
    import torch
    from spectavi_amd import device
    im, _ = sur_ogre()
    t = device.sift(torch.from_numpy(im).cuda())
    geom, desc = device.split_sift_table(t)
    assert geom.shape == (1168, 4) and desc.shape == (1168, 128)
    assert torch.equal(desc.to(torch.float32).cpu(), t[:, 4:].cpu())
    out = device.normalize(t)
    assert out.shape == (1168, 144)


def test_striped_follows_reference_stitching(feature):
    """(height, nthread, buffer_size): the reference's defaults at a small size, no overlap at all, a height
    that nthread does not divide (a short last stripe), and more threads than rows (one-row stripes)."""
    for hgt, nthread, buf in ((200, 4, 20), (200, 4, 0), (203, 4, 20), (12, 16, 20), (12, 16, 0)):
        im = smooth_random(7, hgt, 150)
        got = feature.sift_filter_striped(im, nthread=nthread, buffer_size=buf)
        split = int(np.ceil(hgt / float(nthread)))
        parts, seen = [], {}
        for iy in range(0, hgt, split):
            lo, hi = iy, min(iy + split, hgt)
            b0, b1 = max(lo - buf, 0), min(hi + buf + 1, hgt)
            if (b0, b1) not in seen:
                seen[(b0, b1)] = so.sift(im[b0:b1])
            t = seen[(b0, b1)].copy()
            t[:, 1] += b0
            parts.append(t[(t[:, 1] > lo) & (t[:, 1] < hi)])
        want = np.vstack(parts)
        assert len(parts) == min(nthread, hgt) and (len(want) > 0) == (not (hgt == 12 and buf == 0))  # two-row stripes: no rows
        assert_tables_match(got, want, "striped %d rows, nthread %d, buffer %d" % (hgt, nthread, buf))


def test_batch_of_no_images(feature):
    assert feature.sift_filter_batch([]) == [] and feature.sift_filter_batch([], nthread=3) == []
    assert [t.shape for t in feature.sift_filter_batch([np.full((9, 9), 1, np.float32)], nthread=8)] == [(0, 132)]


def test_overflow_reports_true_count(feature):
    from spectavi_amd._lib import SPV_ERR_INVALID, SpectaviError
    im, _ = sur_ogre()
    table, n = feature.sift_table(im, 2000)
    assert n == 1168
    full = feature.sift_filter(im)
    assert np.array_equal(table[:n], full)
    with pytest.raises(SpectaviError) as e:
        feature.sift_table(im, 100)
    assert e.value.status == 5 and "1168" in str(e.value)
    with pytest.raises(SpectaviError) as e:
        feature.sift_table(im, -1)
    assert e.value.status == SPV_ERR_INVALID


def test_device_capacity_overflow_keeps_true_count():
    import torch
    from spectavi_amd import device
    im, _ = sur_ogre()
    x = torch.from_numpy(im).cuda()
    table = torch.zeros((10, 132), dtype=torch.float32, device="cuda")
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    device.sift_into(x, table, count)
    assert int(count.item()) == 1168
    full = device.sift(x)
    assert torch.equal(table, full[:10])


def test_bad_sizes_raise(feature):
    import ctypes as ct
    from spectavi_amd._lib import SpectaviError, clib
    with pytest.raises(TypeError):
        feature.sift_filter(np.zeros((2, 2, 2), np.float32))
    with pytest.raises(SpectaviError):
        feature.sift_filter(np.zeros((0, 5), np.float32))
    with pytest.raises(SpectaviError):
        feature.sift_filter(np.zeros((9000, 1), np.float32))
    out = feature.NdArray(dtype="float32")
    f = clib.spv_sift_filter
    im = np.zeros((4, 4), np.float32)
    assert f(im.ctypes.data, 4, -4, ct.byref(out)) == 1
    assert f(None, 4, 4, ct.byref(out)) == 1


def test_second_pass_gives_the_same_bits(feature):
    """A first table guess below the true count runs the pipeline again into an exact table."""
    from spectavi_amd._lib import clib
    im, _ = sur_ogre()
    want, n = feature.sift_table(im, 4096)
    assert n == 1168
    try:
        assert clib.spv_sift_set_first_capacity(10) == 0
        got = feature.sift_filter(im)
        batch = feature.sift_filter_batch([im, smooth_random(5, 64, 80)])
    finally:
        clib.spv_sift_set_first_capacity(0)
    assert got.tobytes() == want[:n].tobytes()
    assert batch[0].tobytes() == want[:n].tobytes()
    assert batch[1].tobytes() == feature.sift_filter(smooth_random(5, 64, 80)).tobytes()


def test_second_pass_releases_the_first_table(feature):
    """The short first table (here 14 000 rows, 7.4 MB) goes back to the pool: after the pool is
    emptied, three calls leave the device's free memory where one call left it."""
    import torch
    from spectavi_amd._lib import clib
    im = smooth_random(1, 480, 641)
    try:
        assert clib.spv_sift_set_first_capacity(14000) == 0
        assert len(feature.sift_filter(im)) == 14272
        torch.cuda.synchronize()
        clib.spv_release_cached_memory()
        free0 = torch.cuda.mem_get_info()[0]
        for _ in range(3):
            assert len(feature.sift_filter(im)) == 14272
        clib.spv_release_cached_memory()
        free1 = torch.cuda.mem_get_info()[0]
    finally:
        clib.spv_sift_set_first_capacity(0)
    assert free0 - free1 < 4 << 20, "device memory fell by %d bytes over three second-pass calls" % (free0 - free1)
    assert clib.spv_sift_set_first_capacity(-1) != 0
