"""Numpy restatement of kernelized observations (the reference's GPRF(kernelized=True), gaussian_llgrad_kernel,
gprf.py:674-736, under the unit loop and Bethe weights of gprf.py:206-296) — test infrastructure only.  Units, weights,
local=False and subset_llgrad are the oracle's (oracle.gprf_ref.GPRFRef); only a unit's arithmetic differs.  For a unit with
rows idx (pairs: i-rows first), YYu = YY[idx][:, idx], K = k(X, X) + nv I, P = K^-1, B = P YYu P:

    ll = -1/2 sum P o YYu - 1/2 dy logdet K - 1/2 dy m log 2 pi
    gX[p, i] = sum_q (B - dy P)[p, q] dk(x_p, x_q)/dx_p[i]       (row derivative, zero diagonal)
    gC[t] = 1/2 sum (B - dy P) o dK/dtheta_t

``inv`` selects the arithmetic: "inv" (np.linalg.inv / slogdet, as the reference) or "chol" (the device's route: K = L L^T,
W = L^-1, P = W^T W, logdet = 2 sum log diag L).  The spread between the two is the rounding floor the GPU tests are bounded by.
With YY = Y Y^T and dy = Y.shape[1] this is the dense evaluation (GPRFRef.llgrad) up to rounding."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle.gprf_ref import GPRFRef


def check_symmetric(YY):
    YY = np.asarray(YY, dtype=np.float64)
    if YY.ndim != 2 or YY.shape[0] != YY.shape[1]:
        raise ValueError("YY must be square")
    if not np.array_equal(YY, YY.T):
        raise ValueError("YY must be exactly symmetric; pass 0.5*(YY+YY.T)")
    return YY


class KernelizedRef(GPRFRef):

    def __init__(self, X, YY, dy, block_fn, cov, noise_var, inv="inv", **kwargs):
        if dy is None or int(dy) != dy or dy < 1:
            raise ValueError("dy must be an integer >= 1")
        self.YY = check_symmetric(YY)
        self.dy = int(dy)
        self.how = inv
        super(KernelizedRef, self).__init__(X, None, block_fn, cov, noise_var, **kwargs)

    def llgrad_unary(self, i, **kwargs):
        idxs = np.asarray(self.block_idxs[i], dtype=np.int64)
        return self.gaussian_llgrad_kernel(self.X[idxs], self.YY[np.ix_(idxs, idxs)], **kwargs)

    def llgrad_joint(self, i, j, **kwargs):
        idx = np.concatenate([np.asarray(self.block_idxs[i], dtype=np.int64), np.asarray(self.block_idxs[j], dtype=np.int64)])
        return self.gaussian_llgrad_kernel(self.X[idx], self.YY[np.ix_(idx, idx)], **kwargs)

    def _prec(self, K):
        if self.how == "inv":
            return np.linalg.inv(K), np.linalg.slogdet(K)[1]
        L = np.linalg.cholesky(K)
        W = solve_triangular(L, np.eye(K.shape[0]), lower=True)
        return np.dot(W.T, W), 2.0 * np.sum(np.log(np.diag(L)))

    def gaussian_llgrad_kernel(self, X, YY, grad_X=False, grad_cov=False):
        n, dx = X.shape
        dy = self.dy
        ncov = 2 + len(self.cov.dfn_params)
        if n == 0:
            return 0.0, (np.zeros(X.shape) if grad_X else np.zeros(())), (np.zeros((ncov,)) if grad_cov else np.zeros(()))
        K = self.kernel(X)
        prec, logdet = self._prec(K)
        M = np.dot(np.dot(prec, YY), prec) - dy * prec
        ll = -.5 * np.sum(prec * YY)
        ll += -.5 * dy * logdet
        ll += -.5 * dy * n * np.log(2 * np.pi)
        gradX, gradC = np.zeros(()), np.zeros(())
        if grad_X:
            gradX = np.zeros((n, dx))
            for i in range(dx):
                gradX[:, i] = np.sum(M * self._dK_all_rows(X, i), axis=1)
        if grad_cov:
            gradC = np.zeros((ncov,))
            for t in range(ncov):
                gradC[t] = .5 * np.sum(M * self.dKdi(X, t))
        return ll, gradX, gradC
