"""Writes sift_castle_01.npz and sift_castle_02.npz: 240 x 320 grey uint8 crops of the reference's two
castle photographs (data/castle/01.jpg, 02.jpg, decoded and reduced to grey by PIL).  Each crop is the
16-aligned window of that size with the most saturated pixels (sky burnt out to exactly 255, 17-19 % of
the crop) beside masonry and foliage: exact DoG ties and zeros next to real structure.

Run from the repo root:  SPECTAVI_REFERENCE_TREE=<reference checkout> python tests/golden/make_sift_castle.py
No test runs this.
"""
import os

import numpy as np
from PIL import Image

OUT = os.path.dirname(os.path.abspath(__file__))
CROPS = {"01": (432, 0), "02": (368, 0)}  # top-left (row, column) of each 240 x 320 window
H, W = 240, 320


def main():
    for name, (y, x) in CROPS.items():
        src = os.path.join(os.environ["SPECTAVI_REFERENCE_TREE"], "data", "castle", name + ".jpg")
        grey = np.asarray(Image.open(src).convert("L"))
        crop = np.ascontiguousarray(grey[y:y + H, x:x + W])
        assert crop.shape == (H, W) and crop.dtype == np.uint8
        assert (crop == 255).mean() > 0.05, "the crop holds no saturated sky"
        np.savez_compressed(os.path.join(OUT, "sift_castle_%s.npz" % name), im=crop)


if __name__ == "__main__":
    main()
