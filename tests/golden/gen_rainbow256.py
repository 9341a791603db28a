"""Writes rainbow256.npy: uint8 [256,3], what the reference's depth video gets for each of the 256 entries of matplotlib's `rainbow`
colour map -- utils.to8b(plt.get_cmap('rainbow')(x)[..., :3]) at the centre x = (i + 0.5) / 256 of entry i (run_render.py:314-315).
Needs matplotlib (written with 3.10.8, numpy 2.2.6); the package builds the same table without it (video.rainbow_table), and
tests/test_video_cases.py holds the two equal.  Run from this directory:  python gen_rainbow256.py"""
import os

import matplotlib
matplotlib.use("Agg")
import matplotlib.pyplot as plt
import numpy as np

to8b = lambda x: (255*np.clip(x,0,1)).astype(np.uint8)

if __name__ == "__main__":
    x = (np.arange(256) + 0.5) / 256
    table = to8b(plt.get_cmap('rainbow')(x)[..., :3])
    assert table.shape == (256, 3) and table.dtype == np.uint8
    np.save(os.path.join(os.path.dirname(os.path.abspath(__file__)), "rainbow256.npy"), table)
    print("rainbow256.npy written,", table.nbytes, "bytes")
