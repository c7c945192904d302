"""Writes sift_sur_ogre_image.npz: the reference's SIFT test image (data/sift-test/sur-ogre.npz, float64
grey values 2..255, all integers) stored losslessly as uint8.  sift_sur_ogre_table.npz is vlfeat's own
table for it (data/sift-test/sur-ogre.sift).

Run from the repo root:  SPECTAVI_REFERENCE_TREE=<reference checkout> python tests/golden/make_sift_image.py
"""
import os

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))


def main():
    src = os.path.join(os.environ["SPECTAVI_REFERENCE_TREE"], "data", "sift-test", "sur-ogre.npz")
    im = np.load(src)["im"]
    u8 = im.astype(np.uint8)
    assert np.array_equal(u8.astype(im.dtype), im), "the image is not integer-valued in 0..255"
    np.savez_compressed(os.path.join(OUT, "sift_sur_ogre_image.npz"), im=u8)


if __name__ == "__main__":
    main()
