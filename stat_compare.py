#!/usr/bin/env python3
"""
Frechet distance between two feature-statistics files (stat_generate.py's npz, or the reference's): the counterpart of the
reference's stat_compare.py, same two positional arguments.  float64 throughout; the matrix square root comes from symmetric
eigendecompositions (no scipy).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from vq_voice_swap_amd.stats import frechet_distance  # noqa: E402


def arg_parser():
    p = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("stat_1", type=str)
    p.add_argument("stat_2", type=str)
    return p


def main(argv=None):
    args = arg_parser().parse_args(argv)
    stat1 = np.load(args.stat_1)
    stat2 = np.load(args.stat_2)
    print(frechet_distance(stat1["mean"], stat1["cov"], stat2["mean"], stat2["cov"]))


if __name__ == "__main__":
    main()
