"""Prediction from a fitted GPRF: ``GPRF.train_predictor(test_cov=None, Y=None)`` (reference ``gprf.py:593-672``) and the
error measures the reference's analysis scores it with (``prediction_error``, ``gprfopt.py:121-170``).

The predictor is a snapshot taken on the device (``gprf_predictor_create``): every block's ``W = U^-T`` (``K^-1 = W^T W``),
``alpha = K^-1 Y`` and points.  One ``predict`` / ``predict_blocks`` call is one library call (``gprf_predict``), however
many test blocks it covers.  The reference's version reads attributes of its nonstationary variant on the way; for the
stationary model the arithmetic is: the training kernel with ``noise_var`` on the diagonal (``gprf.py:333-343``), the
messages from the model's own covariance, ``nv = noise_var`` — include/gprf_hip.h has the formulas.
"""
import numpy as np

from . import _capi


class Predictor(object):
    """What ``GPRF.train_predictor`` returns: callable as ``predict(Xstar, test_noise_var=0.0, local=False)``."""

    def __init__(self, gprf, test_cov=None, Y=None):
        cov = gprf.cov
        if test_cov is None:
            test_cov = cov
        elif (test_cov.dfn_str, test_cov.wfn_str) != (cov.dfn_str, cov.wfn_str):
            # (the prior is evaluated by the library's compiled kernel instantiation of the model: DESIGN.md section 8)
            raise ValueError("test_cov must use the model's distance and kernel (%s, %s)" % (cov.dfn_str, cov.wfn_str))
        self._prior_theta = np.concatenate([[float(test_cov.wfn_params[0])],
                                            np.asarray(test_cov.dfn_params, dtype=np.float64).ravel()])
        X = np.ascontiguousarray(gprf.X, dtype=np.float64)
        self._impl = _capi.Predictor(gprf._ctx, X, Y)
        # the snapshot's host half: how test points find their blocks and which blocks neighbour them (gprf.py:627-640)
        self.block_fn = gprf.block_fn
        self.n_blocks = gprf.n_blocks
        self.neighbor_dict = {i: frozenset(s) for i, s in gprf.neighbor_dict.items()}
        self.dx, self.dy = X.shape[1], gprf.Y.shape[1]

    def _test_blocks(self, Xstar):
        if self.block_fn is None:
            raise ValueError("prediction needs the GPRF's block_fn to place the test points")
        blocks = self.block_fn(Xstar)
        if len(blocks) != self.n_blocks:
            raise ValueError("block_fn returned %d blocks for the test points, the model has %d" % (len(blocks), self.n_blocks))
        return blocks

    def _sources(self, i):
        return sorted({i} | set(self.neighbor_dict.get(i, ())))

    def __call__(self, Xstar, test_noise_var=0.0, local=False):
        """gprf.py:603-672: (mean t x dy, cov t x t) at the t <= 512 rows of Xstar, from every block that receives a test
        point and the neighbours of those.  ``local`` is accepted and ignored, as in the reference."""
        Xstar = np.ascontiguousarray(Xstar, dtype=np.float64).reshape(-1, self.dx)
        t = Xstar.shape[0]
        if t > _capi.PRED_MAX_T:
            raise ValueError("predict takes at most %d test points per call (got %d); see predict_blocks" % (_capi.PRED_MAX_T, t))
        if t == 0:
            return np.zeros((0, self.dy)), np.zeros((0, 0))
        src = set()
        for i, idxs in enumerate(self._test_blocks(Xstar)):
            if len(idxs):
                src.update(self._sources(i))
        means, covs = self._impl.predict(Xstar, [np.arange(t)], [sorted(src)], self._prior_theta, test_noise_var)
        return means[0], covs[0]

    def predict_blocks(self, Xtest, test_noise_var=0.0):
        """Every non-empty test block g of block_fn(Xtest) predicted from {g} and its neighbours — the loop of
        gprfopt.py:125-146 — in one library call.  -> (test_blocks, means, covs): the blocks' row index arrays into Xtest
        and, for each, its mean (t x dy) and covariance (t x t)."""
        Xtest = np.ascontiguousarray(Xtest, dtype=np.float64).reshape(-1, self.dx)
        blocks = [np.asarray(b, dtype=np.int64) for b in self._test_blocks(Xtest)]
        gi = [i for i, b in enumerate(blocks) if len(b)]
        test_blocks = [blocks[i] for i in gi]
        if not gi:
            return [], [], []
        means, covs = self._impl.predict(Xtest, test_blocks, [self._sources(i) for i in gi], self._prior_theta, test_noise_var)
        return test_blocks, means, covs

    def close(self):
        self._impl.close()


def _gaussian_ll(Y, M, C):
    """gprfopt.py:127-134 (analysis on one returned block, not the hot path)"""
    ntest, yd = Y.shape
    P = np.linalg.inv(C)
    R = Y - M
    ll = -.5 * np.sum(P * np.dot(R, R.T))
    ll -= .5 * yd * np.linalg.slogdet(C)[1]
    ll -= .5 * yd * ntest * np.log(2 * np.pi)
    return ll


def prediction_error(gprf, Xtest, Ytest, Ytrain, test_noise_var):
    """gprfopt.py:121-170 -> (smse, msll_block, msll_diag): every test block predicted from its own block and neighbours
    (one predict_blocks call), standardised against a constant predictor fitted to the training targets Ytrain."""
    p = gprf.train_predictor()
    try:
        blocks, means, covs = p.predict_blocks(Xtest, test_noise_var=test_noise_var)
    finally:
        p.close()
    Ytest = np.asarray(Ytest, dtype=np.float64)
    ll_block = ll_diag = se_block = 0.0
    for idxs, PM, PC in zip(blocks, means, covs):
        Yt = Ytest[idxs]
        ll_block += _gaussian_ll(Yt, PM, PC)
        ll_diag += _gaussian_ll(Yt, PM, np.diag(np.diag(PC)))
        se_block += np.sum((Yt - PM) ** 2)
    ntest, yd = Ytest.shape
    Ymean = np.mean(Ytrain, axis=0)
    smse = se_block / np.sum((Ytest - Ymean) ** 2)
    Ystd = np.std(Ytrain, axis=0)
    # sum_i log N(Ytest[:, i]; Ymean[i], Ystd[i]^2)  (scipy.stats.norm(...).logpdf in the reference)
    ll_baseline = np.sum(-0.5 * np.log(2 * np.pi * Ystd ** 2) - (Ytest - Ymean) ** 2 / (2 * Ystd ** 2))
    mll_baseline = ll_baseline / (ntest * yd)
    return smse, ll_block / (ntest * yd) - mll_baseline, ll_diag / (ntest * yd) - mll_baseline
