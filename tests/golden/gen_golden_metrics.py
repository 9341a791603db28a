"""Generate tests/golden/ssim_maps.npz: the REFERENCE's own utils.rgb_ssim(img, gt, max_val=1, return_map=True) on the image
pairs of tests/metrics_cases.py.  The file holds reference outputs only (one float64 map per pair, under the pair's name); the
inputs come from seeds.  Runs only where the reference tree is present.

    python tests/golden/gen_golden_metrics.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import metrics_cases  # noqa: E402
from oracle import install_stubs  # noqa: E402


def main():
    utils = install_stubs.import_reference("utils")
    maps = {}
    for name in metrics_cases.PAIRS:
        img, gt = metrics_cases.pair(name)
        m = utils.rgb_ssim(img, gt, max_val=1, return_map=True)
        assert m.dtype == np.float64 and m.shape == (img.shape[0] - 10, img.shape[1] - 10, 3), (name, m.dtype, m.shape)
        maps[name] = m
        print("%-14s frame %3d x %3d  mean ssim %.12f" % (name, img.shape[0], img.shape[1], m.mean()))
    out = os.path.join(HERE, "ssim_maps.npz")
    np.savez_compressed(out, **maps)
    print("wrote %s (%d bytes)" % (out, os.path.getsize(out)))


if __name__ == "__main__":
    main()
