#!/usr/bin/env python3
"""Digest of a `bench.py --dump-outputs DIR` directory: one line per array (shape, dtype, finiteness, max |x|, sha256 of the bytes).
Two builds computed the same bits exactly when their digests are equal line for line.
usage: tools/dump_digest.py DIR [OTHER_DIGEST_FILE]   (with a second argument: also compares and prints IDENTICAL / DIFFERENT per array;
exit status 1 on any difference)"""
import glob
import hashlib
import os
import sys

import numpy as np


def digest(d):
    out = {}
    for f in sorted(glob.glob(os.path.join(d, "*.npy"))):
        x = np.load(f)
        out[os.path.basename(f)] = (f"{str(x.shape):22s} {x.dtype} finite {bool(np.isfinite(x).all())} max|x| {float(np.abs(x).max()):.6e} "
                                    f"sha256 {hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()}")
    return out


def main():
    mine = digest(sys.argv[1])
    if not mine:
        sys.exit(f"{sys.argv[1]}: no .npy files")
    other = {}
    if len(sys.argv) > 2:
        for line in open(sys.argv[2]):
            if line.startswith("  ") and ".npy" in line:
                name, rest = line.strip().split(None, 1)
                other[name] = rest.rsplit("  ", 1)[0].strip() if rest.endswith(("IDENTICAL", "DIFFERENT")) else rest.strip()
    same = 0
    for name, d in mine.items():
        verdict = ""
        if len(sys.argv) > 2:
            ok = other.get(name) == d
            same += ok
            verdict = "  IDENTICAL" if ok else "  DIFFERENT"
        print(f"  {name:28s} {d}{verdict}")
    if len(sys.argv) > 2:
        print(f"  -> {same} of {len(mine)} arrays bit-identical")
        return 0 if same == len(mine) == len(other) else 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
