"""CPU checks of the prediction restatement (tests/predict_ref.py) on its two independent consequences, the reference's
test-noise quirk, and the presence of the prediction surface (GPRF.train_predictor, the C ABI's predictor calls)."""
import os
import re

import numpy as np

from conftest import ROOT
from oracle.vector_tree import GPCov
from predict_ref import PredictorRef, exact_posterior

NV = 0.01
COV = GPCov([1.0], [0.3, 0.3], "euclidean", "se")


def _data(n=90, t=12, seed=3):
    rng = np.random.RandomState(seed)
    X = rng.rand(n, 2)
    Y = rng.randn(n, 4)
    Xs = rng.rand(t, 2)
    return X, Y, Xs


def _tree_kernel(A, B):
    from predict_ref import _tree
    return _tree(COV).kernel_matrix(A, B, False)


def test_one_block_is_the_exact_gp():
    """one block, test_noise_var = noise_var: prior and messages cancel down to the exact GP posterior"""
    X, Y, Xs = _data()
    p = PredictorRef(X, Y, [np.arange(len(X))], {}, lambda Z: [np.arange(len(Z))], COV, NV)
    mean, cov = p(Xs, test_noise_var=NV)
    em, ec = exact_posterior(X, Y, Xs, COV, NV)
    assert np.max(np.abs(mean - em)) <= 1e-10 * np.max(np.abs(em))
    assert np.max(np.abs(cov - ec)) <= 1e-10 * np.max(np.abs(ec))


def test_empty_blocks_contribute_nothing():
    X, Y, Xs = _data()
    b = [np.arange(0, 45), np.arange(45, 90)]
    nd = {0: {1}, 1: {0}}
    p = PredictorRef(X, Y, b, nd, None, COV, NV)
    m0, c0 = p.predict_from(Xs, [0, 1], NV)
    b2 = [b[0], np.zeros(0, np.int64), b[1]]
    p2 = PredictorRef(X, Y, b2, {0: {1, 2}, 1: {0}, 2: {0}}, None, COV, NV)
    m1, c1 = p2.predict_from(Xs, [0, 1, 2], NV)
    assert np.array_equal(m0, m1) and np.array_equal(c0, c1)


def test_test_noise_quirk():
    """Kss carries the MODEL's noise_var whenever test_noise_var > 0 (gprf.py:652-653) while the prior carries
    test_noise_var; with test_noise_var = 0 neither has noise"""
    X, Y, Xs = _data()
    p = PredictorRef(X, Y, [np.arange(len(X))], {}, lambda Z: [np.arange(len(Z))], COV, NV)
    K0 = _tree_kernel(Xs, Xs)
    Ks = _tree_kernel(Xs, X)
    K = _tree_kernel(X, X) + NV * np.eye(len(X))
    S = Ks @ np.linalg.solve(K, Ks.T)
    mu = Ks @ np.linalg.solve(K, Y)
    I = np.eye(len(Xs))
    for tnv, kss_noise in ((0.5 * NV, NV), (3.0 * NV, NV), (0.0, 0.0)):
        Kss = K0 + kss_noise * I
        P = np.linalg.inv(K0 + tnv * I) + np.linalg.inv(Kss - S) - np.linalg.inv(Kss)
        want_c = np.linalg.inv(P)
        want_m = want_c @ np.linalg.solve(Kss - S, mu)
        mean, cov = p(Xs, test_noise_var=tnv)
        assert np.max(np.abs(cov - want_c)) <= 1e-8 * np.max(np.abs(want_c)), tnv
        assert np.max(np.abs(mean - want_m)) <= 1e-8 * np.max(np.abs(want_m)), tnv
    # the quirk is visible: with test_noise_var != noise_var the result is NOT the exact posterior with test noise
    mean, cov = p(Xs, test_noise_var=0.5 * NV)
    _, ec = exact_posterior(X, Y, Xs, COV, NV)
    assert np.max(np.abs(cov - (ec - 0.5 * NV * I))) > 1e-6


def test_prediction_surface_exists():
    from gprf_amd import _capi
    from gprf_amd.gprf import GPRF
    from gprf_amd.predict import Predictor, prediction_error  # noqa: F401
    assert callable(getattr(GPRF, "train_predictor", None))
    assert callable(getattr(Predictor, "predict_blocks", None)) and callable(getattr(Predictor, "close", None))
    text = open(os.path.join(ROOT, "include", "gprf_hip.h")).read()
    for name in ("gprf_predictor_create", "gprf_predictor_destroy", "gprf_predict"):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _capi.SIGNATURES
    assert "gprf.py:593-672" in text
