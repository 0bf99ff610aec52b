"""Evaluation of all pair planes of a sweep, CPU side: the numpy restatement (tests/eval_pairs_ref.py) against the fixture
from the reference's evaluate_performance / get_statistics (g22), the side header include/resdepth_hip_eval.h against its
bindings and the library's exports, and the coverage ledger of tests/test_eval_planes_contract_gpu.py."""
import os
import re

import numpy as np

import eval_classes_ref as R
import eval_pairs_ref as PR
from conftest import load_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_reproduces_the_reference_per_pair_and_pooled():
    g = load_npz("g22_pairs_eval.npz")
    kw = PR.g22_case(g)
    want = PR.restate(**kw)
    assert want["classes"] == [str(c) for c in g["classes"]] == R.CLASSES
    n_planes = kw["pairs"].shape[0]
    assert n_planes == 3
    for p in range(n_planes):
        calls = g[f"p{p}/calls"]                         # the reference's call order: per class, before then after
        got = np.stack([want["before"], want["pairs"][p]], axis=1).reshape(-1, 14)
        assert got.shape == calls.shape
        np.testing.assert_allclose(got, calls, rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=f"pair {p}")
    np.testing.assert_allclose(want["pooled"], g["pooled/calls"], rtol=1e-12, atol=1e-12, equal_nan=True)
    # the fixture is what its docstring says: planes with nodata pixels of their own, and a pool larger than any plane
    nod = kw["pairs"] == kw["nodata"]
    assert all((nod[p] & ~nod[q]).any() for p in range(3) for q in range(3) if p != q)
    counts = want["pairs"][:, :, 0]
    np.testing.assert_array_equal(want["pooled"][:, 0], counts.sum(axis=0))
    assert len({tuple(c) for c in counts}) == 3


def _declared():
    text = open(os.path.join(ROOT, "include", "resdepth_hip_eval.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    return text, set(re.findall(r"\b(rd_\w+)\s*\(", text))


def test_eval_header_and_bindings_agree():
    """include/resdepth_hip_eval.h declares what _lib.SIGNATURES_EVAL binds, and the library exports it"""
    from resdepth_amd import _lib, evaluation
    text, declared = _declared()
    assert declared == set(_lib.SIGNATURES_EVAL) == {"rd_eval_classify_planes", "rd_residual_stats_pooled_ws_bytes",
                                                      "rd_residual_stats_pooled"}
    for name, (_, args) in _lib.SIGNATURES_EVAL.items():
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text, flags=re.S).group(1)
        assert len(args) == len(params.split(",")), name
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name)
    assert lib.rd_version() >= 113
    main = open(os.path.join(ROOT, "include", "resdepth_hip.h")).read()
    assert '#include "resdepth_hip_eval.h"' in main
    for name in declared:                                # declared in the side header only, bound in SIGNATURES_EVAL only
        assert not re.search(r"\b%s\s*\(" % name, main)
        assert name not in _lib.SIGNATURES and name not in _lib.SIGNATURES_PAIRS and name not in _lib.SIGNATURES_TTA
    defs = dict(re.findall(r"#define (RD_\w+) (\d+)", text))
    assert int(defs["RD_EVAL_MAX_PLANES"]) == evaluation.MAX_PLANES == 16
    assert int(defs["RD_CLS_VALID_EXTRA"]) == evaluation.VALID_EXTRA
    assert not evaluation.VALID_EXTRA & (evaluation.VALID_BEFORE | evaluation.VALID_AFTER | sum(evaluation.CLASS_BITS.values()))


def test_every_function_of_the_eval_header_has_a_memory_contract_case():
    """the ledger of tests/test_eval_planes_contract_gpu.py needs no GPU"""
    import test_eval_planes_contract_gpu as T
    T.ledger_check()
    assert len(T.CASES) >= 10
