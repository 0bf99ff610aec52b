"""A numpy fp64 oracle of include/resdepth_hip_dist.h: sort, then the header's rule operation for operation.  numpy does not
contract a multiplication and an addition into one rounding, so the values equal the device's bit for bit.

The device ranks by the 64-bit keys of its radix select, where -0.0 lies below +0.0; numpy's sort calls the two equal and keeps
either.  The oracle therefore sorts the keys.  That only matters for a mode-0 quantile that lands on a zero."""
import numpy as np

SIGN = np.uint64(1 << 63)


def keys_of(v):
    """the order-preserving unsigned keys of fp64 values (key_of in csrc/rd_stats.hip)"""
    b = np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)
    return np.where(b >> np.uint64(63) != 0, ~b, b | SIGN)


def values_of(k):
    k = np.ascontiguousarray(k, dtype=np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~SIGN, ~k).view(np.float64)


def ranked(r, mode):
    """the members in the device's rank order: mode 0 ranks r, mode 1 ranks |r|"""
    v = np.abs(r) if mode else np.asarray(r, dtype=np.float64)
    return values_of(np.sort(keys_of(v)))


def quantile_sorted(v, q):
    """Q of the header from ranked values v (c = len(v)); NaN for an empty set"""
    c = len(v)
    if c == 0:
        return np.float64(np.nan)
    h = np.float64(c - 1) * np.float64(q)              # one multiplication
    lo = np.floor(h)
    g = h - lo                                         # exact
    lo = int(lo)
    if g == 0:
        return np.float64(v[lo])
    d = np.float64(v[lo + 1]) - np.float64(v[lo])      # three separately rounded operations
    p = np.float64(g) * d
    return np.float64(v[lo]) + p


def quantile(r, q, mode):
    return quantile_sorted(ranked(r, mode), q)


def share(r, tau):
    """W of the header: members with |r| <= tau over members, both counted; NaN for an empty set"""
    r = np.asarray(r, dtype=np.float64)
    if r.size == 0:
        return np.float64(np.nan)
    return np.float64(int((np.abs(r) <= tau).sum())) / np.float64(r.size)


def members(r, cls, need, thr):
    """the members of a set: class byte holds all `need` bits, |r| <= thr when thr > 0"""
    ok = (np.asarray(cls).astype(np.int64) & need) == need
    if thr > 0:
        ok &= np.abs(r) <= thr
    return np.asarray(r, dtype=np.float64)[ok]


def row(r, levels, modes, taus):
    """one output row of rd_residual_dist_*: count, quantiles, shares of the members r"""
    sorted_by_mode = {m: ranked(r, m) for m in set(modes)}
    return np.array([np.float64(len(r))] + [quantile_sorted(sorted_by_mode[m], q) for q, m in zip(levels, modes)]
                    + [share(r, t) for t in taus], dtype=np.float64)
