"""Oracle of rd_grad_norm (include/resdepth_hip_optim.h), written from its definition in fp64 numpy."""
import numpy as np


def grad_stats(g):
    """(sum of squares of the finite elements in fp64, number of non-finite elements) of the RAW gradient"""
    g = np.asarray(g, np.float32)
    fin = np.isfinite(g)
    return float((g[fin].astype(np.float64) ** 2).sum()), float((~fin).sum())
