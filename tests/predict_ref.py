"""Numpy restatement of GPRF prediction (the reference's train_predictor / predict, gprf.py:593-672) for the stationary
model, written from the algebra — test infrastructure only.  Kernel values come from the oracle's kernel
(oracle.vector_tree.VectorTree.kernel_matrix).

    prior_cov = k_test(X*, X*) + test_noise_var I,  P = inv(prior_cov),  b = 0
    for every source block i (the blocks receiving a test point, and their neighbours):
        K* = k(X*, X_i),  Kss = k(X*, X*) (+ noise_var I only when test_noise_var > 0)
        mean_i = K* K_i^-1 Y_i,  cov_i = Kss - K* K_i^-1 K*^T      (K_i = k(X_i, X_i) + noise_var I)
        P += inv(cov_i) - inv(Kss),  b += inv(cov_i) mean_i
    cov = inv(P),  mean = cov b

``inv`` selects the arithmetic: "lu" (np.linalg.inv and solve, as the reference) or "chol" (the device's route: every
inverse through a Cholesky factor, K_i^-1 applied as W^T W with W = L_i^-1, cov_i = Kss - V^T V with V = W K*^T); the
spread between the two is the rounding floor the GPU tests are bounded by.  ``kernel_ulps`` > 0 perturbs every kernel value by
a random relative amount of up to that many ulps (symmetrically where the two point sets coincide): the floor that comes
from the kernel values themselves, which the device evaluates with its own exp / haversine forms."""
import numpy as np
from scipy.linalg import cho_factor, cho_solve

from oracle.vector_tree import VectorTree


def _inv(A, how):
    if how == "lu":
        return np.linalg.inv(A)
    c = cho_factor(A, lower=True)
    return cho_solve(c, np.eye(A.shape[0]))


def _tree(cov, kernel_ulps=0, seed=0):
    tree = VectorTree(None, 1, cov.dfn_str, cov.dfn_params, cov.wfn_str, cov.wfn_params)
    if kernel_ulps:
        rng = np.random.RandomState(seed)
        exact = tree.kernel_matrix

        def perturbed(X1, X2, distance_only):
            K = exact(X1, X2, distance_only)
            E = rng.uniform(-1.0, 1.0, K.shape)
            if X1 is X2:
                E = np.tril(E) + np.tril(E, -1).T
            return K * (1.0 + kernel_ulps * np.finfo(np.float64).eps * E)
        tree.kernel_matrix = perturbed
    return tree


class PredictorRef(object):

    def __init__(self, X, Y, block_idxs, neighbor_dict, block_fn, cov, noise_var, test_cov=None, inv="lu", kernel_ulps=0):
        self.tree = _tree(cov, kernel_ulps, 1)
        self.test_tree = _tree(test_cov if test_cov is not None else cov, kernel_ulps, 2)
        self.block_idxs = [np.asarray(b, dtype=np.int64) for b in block_idxs]
        self.neighbor_dict = neighbor_dict
        self.block_fn = block_fn
        self.noise_var = noise_var
        self.how = inv
        self.X = np.array(X, dtype=np.float64)
        self.alphas = []
        for idxs in self.block_idxs:
            Xi = self.X[idxs]
            K = self.tree.kernel_matrix(Xi, Xi, False) + np.eye(len(idxs)) * noise_var
            if not len(idxs):
                self.alphas.append(np.zeros((0, Y.shape[1])))
            elif inv == "lu":
                self.alphas.append(np.linalg.solve(K, Y[idxs]))
            else:
                W = np.linalg.inv(np.linalg.cholesky(K))
                self.alphas.append(W.T @ (W @ Y[idxs]))
        self.dy = Y.shape[1]

    def sources(self, test_blocks):
        src = set()
        for i, idxs in enumerate(test_blocks):
            if len(idxs):
                src.add(i)
                src.update(self.neighbor_dict.get(i, ()))
        return sorted(src)

    def predict_from(self, Xstar, sources, test_noise_var=0.0):
        t = Xstar.shape[0]
        prior = self.test_tree.kernel_matrix(Xstar, Xstar, False) + np.eye(t) * test_noise_var
        P = _inv(prior, self.how)
        b = np.zeros((t, self.dy))
        Kss = self.tree.kernel_matrix(Xstar, Xstar, False)
        if test_noise_var > 0:
            Kss = Kss + np.eye(t) * self.noise_var
        for i in sources:
            idxs = self.block_idxs[i]
            if len(idxs) == 0:
                continue
            Xi = self.X[idxs]
            Ks = self.tree.kernel_matrix(Xstar, Xi, False)
            K = self.tree.kernel_matrix(Xi, Xi, False) + np.eye(len(idxs)) * self.noise_var
            mean = Ks @ self.alphas[i]
            if self.how == "lu":
                cov = Kss - Ks @ np.linalg.solve(K, Ks.T)
            else:
                V = np.linalg.inv(np.linalg.cholesky(K)) @ Ks.T
                cov = Kss - V.T @ V
            prec = _inv(cov, self.how)
            P += prec - _inv(Kss, self.how)
            b += prec @ mean
        C = _inv(P, self.how)
        return C @ b, C

    def __call__(self, Xstar, test_noise_var=0.0, local=False):
        return self.predict_from(Xstar, self.sources(self.block_fn(Xstar)), test_noise_var)

    def predict_blocks(self, Xtest, test_noise_var=0.0):
        out = []
        for g, idxs in enumerate(self.block_fn(Xtest)):
            if len(idxs):
                src = sorted({g} | set(self.neighbor_dict.get(g, ())))
                out.append((np.asarray(idxs), ) + self.predict_from(Xtest[idxs], src, test_noise_var))
        return [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def exact_posterior(X, Y, Xstar, cov, noise_var):
    """the full GP: mean K*K^-1Y, covariance Kss + nv I - K*K^-1K*^T (Cholesky)"""
    tree = _tree(cov)
    K = tree.kernel_matrix(X, X, False) + np.eye(X.shape[0]) * noise_var
    Ks = tree.kernel_matrix(Xstar, X, False)
    c = cho_factor(K, lower=True)
    mean = Ks @ cho_solve(c, Y)
    covp = tree.kernel_matrix(Xstar, Xstar, False) + np.eye(Xstar.shape[0]) * noise_var - Ks @ cho_solve(c, Ks.T)
    return mean, covp
