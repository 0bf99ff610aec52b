"""A numpy model of the split2h operand split (csrc/rd_mfma_dev.h: scale_bexp, split2h_pair), no GPU needed.

x1 = rn16(s x), x2 = rn16(s x - x1) with s a power of two per TENSOR that maps the tensor's maximum into [2^14, 2^15).  np.float16
keeps subnormals, as the MFMA does, and rounds to nearest even once, as v_fma_mix does (s x and s x - x1 are exact in float64).
What this file pins: the two regimes of the split's error, the three-product error of one multiply, the 2^-9-class loss of an
element far below its tensor's maximum that the guard (slot word 1) exists for, and the host decoding of that word."""
import numpy as np
import pytest

from resdepth_amd import _lib


def scale_of(amax: float) -> float:
    """scale_bexp: 2^(268 - biased exponent of amax) as a biased fp32 exponent, clamped at 254"""
    bexp = int(np.array([amax], dtype=np.float32).view(np.uint32)[0]) >> 23
    return 2.0 ** (min(268 - bexp, 254) - 127)


def split(x, s):
    sx = np.asarray(x, dtype=np.float32).astype(np.float64) * s
    x1 = sx.astype(np.float16).astype(np.float64)
    x2 = (sx - x1).astype(np.float16).astype(np.float64)
    return sx, x1, x2


def product3(a, b, sa, sb):
    """the three kept products a1 b1 + a1 b2 + a2 b1 (exact in float64), scaled back"""
    _, a1, a2 = split(a, sa)
    _, b1, b2 = split(b, sb)
    return (a1 * b1 + a1 * b2 + a2 * b1) / (sa * sb)


def tensor(g, n, amax_exp=0):
    x = (g.standard_normal(n) * 2.0 ** amax_exp).astype(np.float32)
    x[0] = np.float32(2.0 ** amax_exp * 3.7)          # a definite maximum
    return x


@pytest.mark.parametrize("amax_exp", [-40, -12, 0, 9, 60])
def test_scale_puts_the_maximum_into_the_top_binade_of_fp16(amax_exp):
    g = np.random.default_rng(1)
    x = tensor(g, 4096, amax_exp)
    s = scale_of(float(np.abs(x).max()))
    top = float(np.abs(x).max()) * s
    assert 2.0 ** 14 <= top < 2.0 ** 15
    _, x1, _ = split(x, s)
    assert np.isfinite(x1).all() and np.abs(x1).max() <= 65504.0


@pytest.mark.parametrize("amax_exp", [-20, 0, 7])
def test_split_error_two_regimes_and_zeros(amax_exp):
    g = np.random.default_rng(2)
    amax = 3.7 * 2.0 ** amax_exp
    s = scale_of(amax)
    # log-uniform magnitudes from the maximum down to 2^-45 below it, random signs, plus exact zeros
    mag = amax * 2.0 ** -g.uniform(0, 45, 200000)
    x = (np.sign(g.standard_normal(mag.size)) * mag).astype(np.float32)
    x[:64] = 0.0
    x[64] = np.float32(amax)
    sx, x1, x2 = split(x, s)
    err = np.abs(sx - x1 - x2)
    assert (x1[:64] == 0).all() and (x2[:64] == 0).all(), "exact zeros stay zero"
    # always: 2^-22 relative while the second term is normal, 2^-25 absolute (half a subnormal step) once it is not
    assert (err <= np.maximum(2.0 ** -22 * np.abs(sx), 2.0 ** -25)).all()
    # first regime: within 2^-17 of the maximum the bound is relative (the 2^-25 floor is <= 2^-22 |s x| from |s x| >= 2^-3 on)
    big = np.abs(x) >= 2.0 ** -17 * amax
    assert (err[big] <= 2.0 ** -22 * np.abs(sx[big])).all()
    # between 2^-18 and 2^-17 of the maximum: the header's 2^-22 holds up to a factor two (|s x| may be as small as 2^-4)
    mid = np.abs(x) >= 2.0 ** -18 * amax
    assert (err[mid] <= 2.0 ** -21 * np.abs(sx[mid])).all()
    # second regime: absolute in scaled units, i.e. 2^-25 / s <= 2^-39 amax in the element's own units
    small = ~mid
    assert small.sum() > 1000
    assert (err[small] <= 2.0 ** -25).all()
    assert (err[small] / s <= 2.0 ** -39 * amax).all()
    # far enough below, an element flushes to zero entirely (both terms), at about 2^-39 amax
    gone = np.abs(sx) < 2.0 ** -25
    assert gone.sum() > 0 and (x1[gone] == 0).all() and (x2[gone] == 0).all()


def test_three_product_error_of_one_multiply():
    g = np.random.default_rng(3)
    a = tensor(g, 200000, 0)
    b = tensor(g, 200000, -9)
    sa, sb = scale_of(float(np.abs(a).max())), scale_of(float(np.abs(b).max()))
    ab = a.astype(np.float64) * b.astype(np.float64)
    e = np.abs(product3(a, b, sa, sb) - ab)
    amax_a, amax_b = float(np.abs(a).max()), float(np.abs(b).max())
    first = (np.abs(a) >= 2.0 ** -17 * amax_a) & (np.abs(b) >= 2.0 ** -17 * amax_b)
    assert first.mean() > 0.99
    assert (e[first] <= 3 * 2.0 ** -22 * np.abs(ab[first])).all()
    # everywhere: the relative part plus 2^-39 amax(a) |b| + 2^-39 amax(b) |a| -- the product of the two
    # absolute errors (<= 2^-50 amax(a) amax(b) 2^-28) is covered by the relative part's slack
    bound = 3 * 2.0 ** -22 * np.abs(ab) + 2.0 ** -39 * (amax_a * np.abs(b) + amax_b * np.abs(a))
    assert (e <= bound).all()
    # the measured typical error is far below the bound (random rounding directions)
    assert float(np.median(e[first] / np.abs(ab[first]))) < 2.0 ** -23


@pytest.mark.parametrize("below,lo,hi", [(30, 2.0 ** -11, 2.0 ** -8), (24, 2.0 ** -17, 2.0 ** -14), (20, 2.0 ** -21, 2.0 ** -18)])
def test_element_far_below_its_tensors_maximum_loses_precision(below, lo, hi):
    """The failure the guard exists for: a batch mate at 2^-30 of its tensor's maximum is known to ~2^-9 (2^14 u per product);
    2^-24 and 2^-20 are in between.  The GPU tests (mates30 / half30 / mates20) must see this unless the launch falls back."""
    g = np.random.default_rng(4)
    big = tensor(g, 4096, 0)
    amax = float(np.abs(big).max())
    # magnitudes in [1, 2) x 2^-below x amax, random signs
    small = (np.sign(g.standard_normal(100000)) * g.uniform(1.0, 2.0, 100000) * 2.0 ** -below * amax).astype(np.float32)
    s = scale_of(amax)
    sx, x1, x2 = split(small, s)
    rel = np.abs(sx - x1 - x2) / np.abs(sx)
    assert lo <= float(rel.max()) <= hi, float(rel.max())
    # with its own scale (what a per-image slot or the six-product fallback amounts to) the same element is 2^-22-exact
    s_own = scale_of(float(np.abs(small).max()))
    sx, x1, x2 = split(small, s_own)
    assert (np.abs(sx - x1 - x2) <= np.maximum(2.0 ** -22 * np.abs(sx), 2.0 ** -25)).all()
    assert float((np.abs(sx - x1 - x2) / np.abs(sx)).max()) <= 2.0 ** -21


# ---- the slot words (include/resdepth_hip.h, csrc/rd_mfma_dev.h: amax_commit / quant_select) -----------------------------------
def commit_model(x, block):
    """What the producer blocks leave in a zeroed slot when block b covers x[b*block:(b+1)*block] (contiguous) and commits to
    line b & 15: word 0 = max bits(|block max|), word 1 = max ~bits(block max) over blocks with a non-zero maximum."""
    words = np.zeros((16, 32), dtype=np.uint32)
    for b in range(0, (x.size + block - 1) // block):
        m = np.float32(np.abs(x[b * block:(b + 1) * block]).max())
        bits = int(np.array([m], dtype=np.float32).view(np.uint32)[0])
        words[b & 15, 0] = max(words[b & 15, 0], bits)
        if bits:
            words[b & 15, 1] = max(words[b & 15, 1], ~bits & 0xFFFFFFFF)
    return words.reshape(-1).view(np.int32)


def test_slot_decoding_and_the_guard():
    g = np.random.default_rng(5)
    assert _lib.slot_decode(np.zeros(512, np.int32)) == (0.0, None)
    assert not _lib.slot_takes_three_products(np.zeros(512, np.int32))
    x = g.standard_normal(64 * 1024).astype(np.float32)
    w = commit_model(x, 1024)
    top, low = _lib.slot_decode(w)
    blocks = np.abs(x.reshape(64, 1024)).max(axis=1)
    assert top == float(np.abs(x).max()) and low == float(blocks.min())
    assert _lib.slot_takes_three_products(w)
    # all-zero blocks (a masked tile, a dead ReLU region) do not count
    x[5 * 1024:9 * 1024] = 0.0
    assert _lib.slot_decode(commit_model(x, 1024))[1] == float(np.delete(blocks, range(5, 9)).min())
    assert _lib.slot_takes_three_products(commit_model(x, 1024))
    # a batch mate 2^-30 below (one contiguous half): the guard fires; at 2^-16 it does not; the threshold is 2^17
    for f, ok in ((2.0 ** -30, False), (2.0 ** -20, False), (2.0 ** -16, True)):
        y = x.copy()
        y[32 * 1024:] *= np.float32(f)
        assert _lib.slot_takes_three_products(commit_model(y, 1024)) == ok, f
    y = np.zeros(4096, np.float32)
    y[0], y[2048] = 2.0 ** 17, 1.0
    assert _lib.slot_takes_three_products(commit_model(y, 1024))
    y[2048] = np.nextafter(np.float32(1.0), np.float32(0.0))
    assert not _lib.slot_takes_three_products(commit_model(y, 1024))
    # channel-wise small values inside every block are invisible to the guard (documented: 2^-39 amax absolute)
    z = g.standard_normal((1024, 64)).astype(np.float32)
    z[:, :4] *= np.float32(2.0 ** -24)
    assert _lib.slot_takes_three_products(commit_model(z.reshape(-1), 1024))
    # an infinite maximum: six products (non-finite semantics)
    z = x.copy()
    z[7] = np.inf
    assert not _lib.slot_takes_three_products(commit_model(z, 1024))
