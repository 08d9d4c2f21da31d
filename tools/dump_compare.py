"""Compare `bench.py --dump-outputs` directories: max abs and relative Frobenius difference of every array.
usage: python3 tools/dump_compare.py LABEL=DIR_A:DIR_B [LABEL=DIR_A:DIR_B ...]"""
import sys

import numpy as np

for spec in sys.argv[1:]:
    label, dirs = spec.split("=", 1)
    da, db = dirs.split(":")
    for name in ("loss", "params"):
        a, b = (np.load(f"{d}/{name}.npy").astype(np.float64) for d in (da, db))
        d = np.abs(a - b)
        line = f"{label:18s} {name:7s} max abs {d.max():.3e}  rel Frobenius {np.linalg.norm(a - b) / np.linalg.norm(a):.3e}"
        if name == "loss":
            line += f"  values {a[0]:.9g} {b[0]:.9g}"
        print(line)
