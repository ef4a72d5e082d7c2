"""Largest relative difference per output between two `bench.py --dump-outputs` directories: max |a - b| / max |a|."""
import glob
import os
import sys

import numpy as np

a, b = sys.argv[1], sys.argv[2]
for f in sorted(glob.glob(os.path.join(a, "*.npy"))):
    x, y = np.load(f), np.load(os.path.join(b, os.path.basename(f)))
    if x.shape != y.shape:
        print("%-28s shapes differ %s %s" % (os.path.basename(f), x.shape, y.shape))
        continue
    sc = np.abs(x).max() if x.size else 0.0
    print("%-28s %.3e" % (os.path.basename(f), (np.abs(x - y).max() / sc) if sc > 0 else 0.0))
    if x.size <= 12:                                    # the scalars (objective, residuals, iterations, rank, status): both sides
        print("    ", np.array2string(x.ravel(), precision=12), "|", np.array2string(y.ravel(), precision=12))
