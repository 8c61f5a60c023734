"""The exact reference of the column statistics for the tests: per column, the correctly rounded sum (math.fsum) and the
correctly rounded sum of squares (summed as exact fractions, rounded once by float())."""
import math
from fractions import Fraction

import numpy as np


def exact_column_sums(idx, val, n):
    """correctly rounded exact column sums and sums of squares (math.fsum; squares as exact fractions)"""
    cols = [[] for _ in range(n)]
    for j, v in zip(idx.tolist(), val.tolist()):
        cols[j].append(v)
    s = np.array([math.fsum(c) for c in cols])
    sq = np.array([float(sum((Fraction(v) * Fraction(v) for v in c), Fraction(0))) for c in cols])
    return s, sq
