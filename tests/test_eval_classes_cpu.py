"""Class-partitioned evaluation, CPU side: the numpy restatement (tests/eval_classes_ref.py) against fixtures from the
reference's evaluate_performance, and its dilation against scipy."""
import numpy as np
import pytest

import eval_classes_ref as R
from conftest import load_npz


def test_restatement_reproduces_reference_evaluate_performance():
    g = load_npz("g18_eval.npz")
    for i in range(int(g["n"])):
        args, thr = R.golden_case(g, i)
        rb, ra, classes = R.classify(**args)
        calls = g[f"c{i}/calls"]
        got = R.evaluate_calls(rb, ra, classes, thr)
        assert got.shape == calls.shape, (i, got.shape, calls.shape)
        np.testing.assert_allclose(got, calls, rtol=1e-12, atol=1e-12, equal_nan=True)
        assert list(g[f"c{i}/classes"]) == [c for c in R.CLASSES if c in classes]
        n = ra.size
        for c in g[f"c{i}/classes"]:
            want = np.unpackbits(g[f"c{i}/rmask_{c}"])[:n].reshape(ra.shape).astype(bool)
            np.testing.assert_array_equal(~classes[str(c)][1], want, err_msg=f"case {i} class {c}")
        np.testing.assert_array_equal(ra[classes["all"][1]], g[f"c{i}/rall"])


def test_numpy_dilation_matches_scipy():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(5)
    for shape in [(1, 1), (1, 40), (40, 1), (33, 57)]:
        for p in (0.02, 0.3):
            m = rng.rand(*shape) < p
            m[0, 0] = m[-1, -1] = True
            for k in (1, 2, 3, 5):
                np.testing.assert_array_equal(R.dilate(m, k), ndimage.binary_dilation(m, iterations=k), err_msg=str((shape, p, k)))
