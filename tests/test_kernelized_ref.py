"""CPU checks of the kernelized-observation restatement (tests/kernelized_ref.py): with YY = Y Y^T it is the dense evaluation
(oracle.gprf_ref.GPRFRef.llgrad) on C1 and on random shapes, empty blocks give 0, a non-symmetric YY is refused — and the
product's surface for the mode: the constructor's argument checks (which run before any device call) and the C ABI entry point."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, blocks_from_csr
from kernelized_ref import KernelizedRef
from oracle.gprf_ref import GPRFRef
from oracle.vector_tree import GPCov


def _rel(a, b):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(np.asarray(b))), 1e-300)


def _pair(X, Y, blocks, nbrs, cov, nv, how="inv"):
    dense = GPRFRef(X, Y, None, cov, nv, block_idxs=blocks, neighbors=nbrs)
    kz = KernelizedRef(X, np.dot(Y, Y.T), Y.shape[1], None, cov, nv, inv=how, block_idxs=blocks, neighbors=nbrs)
    return dense, kz


@pytest.mark.parametrize("how", ["inv", "chol"])
@pytest.mark.parametrize("local", [True, False])
def test_c1_equals_dense_evaluation(how, local):
    """C1 (n = 500, 4 blocks, 6 pairs, dy = 10): ll, gradX, gradC"""
    z = load_golden("c1_small.npz")
    th = z["theta"]
    blocks = blocks_from_csr(z["block_ptr"], z["block_pts"])
    nbrs = [tuple(int(v) for v in r) for r in z["neighbors"]]
    assert len(blocks) == 4 and len(nbrs) == 6
    cov = GPCov([th[1]], th[2:], "euclidean", "se")
    dense, kz = _pair(z["X_obs"], z["SY"], blocks, nbrs, cov, th[0], how)
    a = dense.llgrad(local=local, grad_X=True, grad_cov=True)
    b = kz.llgrad(local=local, grad_X=True, grad_cov=True)
    assert abs(a[0] - b[0]) <= 1e-11 * abs(a[0])
    assert _rel(b[1], a[1]) <= 1e-9
    assert _rel(b[2], a[2]) <= 1e-9


@pytest.mark.parametrize("seed,dx,dy,sizes", [(0, 1, 3, [7, 12, 5]), (1, 2, 17, [30, 1, 22, 9]), (2, 3, 70, [16, 33])])
def test_random_shapes_equal_dense_evaluation(seed, dx, dy, sizes):
    rng = np.random.RandomState(seed)
    n = sum(sizes)
    X = rng.rand(n, dx)
    Y = rng.randn(n, dy)
    perm = rng.permutation(n)
    blocks = np.split(perm, np.cumsum(sizes)[:-1])
    nbrs = [(i, j) for i in range(len(sizes)) for j in range(i) if (i + j) % 2 == 1]
    cov = GPCov([1.3], list(0.2 + 0.3 * rng.rand(dx)), "euclidean", "se")
    dense, kz = _pair(X, Y, blocks, nbrs, cov, 0.05)
    a = dense.llgrad(grad_X=True, grad_cov=True)
    b = kz.llgrad(grad_X=True, grad_cov=True)
    assert abs(a[0] - b[0]) <= 1e-11 * abs(a[0])
    assert _rel(b[1], a[1]) <= 1e-9 and _rel(b[2], a[2]) <= 1e-9
    # subset_llgrad (gprf.py:182-204) likewise
    assert abs(dense.subset_llgrad([0, 1]) - kz.subset_llgrad([0, 1])) <= 1e-11 * abs(dense.subset_llgrad([0, 1]))


def test_empty_blocks_give_zero():
    rng = np.random.RandomState(4)
    X, Y = rng.rand(40, 2), rng.randn(40, 5)
    cov = GPCov([1.0], [0.3, 0.3], "euclidean", "se")
    kz = KernelizedRef(X, np.dot(Y, Y.T), 5, None, cov, 0.01, block_idxs=[np.arange(40)], neighbors=[])
    ll, gX, gC = kz.gaussian_llgrad_kernel(X[:0], np.zeros((0, 0)), grad_X=True, grad_cov=True)
    assert ll == 0.0 and gX.shape == (0, 2) and not gX.any() and np.array_equal(gC, np.zeros(4))
    full = kz.llgrad(grad_X=True, grad_cov=True)
    kz2 = KernelizedRef(X, np.dot(Y, Y.T), 5, None, cov, 0.01, block_idxs=[np.arange(40), np.zeros(0, np.int64)],
                        neighbors=[(1, 0)])
    # block 1 is empty: the pair equals block 0, whose weight 1 - 1 = 0 cancels it — the total is unchanged
    with_empty = kz2.llgrad(grad_X=True, grad_cov=True)
    assert abs(with_empty[0] - full[0]) <= 1e-12 * abs(full[0])


def test_non_symmetric_YY_is_refused():
    rng = np.random.RandomState(5)
    X, Y = rng.rand(20, 2), rng.randn(20, 3)
    YY = np.dot(Y, Y.T)
    YY[3, 7] += 1e-12
    cov = GPCov([1.0], [0.3, 0.3], "euclidean", "se")
    with pytest.raises(ValueError, match=r"0.5\*\(YY\+YY.T\)"):
        KernelizedRef(X, YY, 3, None, cov, 0.01, block_idxs=[np.arange(20)], neighbors=[])


# ---- the product's surface (no device call: the argument checks come first) ----

def _product_args(n=20, dx=2):
    from gprf_amd import GPCov as PC
    rng = np.random.RandomState(6)
    X, Y = rng.rand(n, dx), rng.randn(n, 3)
    return X, np.dot(Y, Y.T), PC([1.0], [0.3] * dx, "euclidean", "se")


@pytest.mark.parametrize("dy", [None, 0, -3, 2.5, True, "4"])
def test_product_refuses_a_bad_dy(dy):
    from gprf_amd.gprf import GPRF
    X, YY, cov = _product_args()
    with pytest.raises(ValueError, match="dy"):
        GPRF(X, YY, None, cov, 0.01, kernelized=True, dy=dy, block_idxs=[np.arange(20)], neighbors=[])


def test_product_refuses_a_non_symmetric_YY():
    from gprf_amd.gprf import GPRF
    X, YY, cov = _product_args()
    YY = YY.copy()
    YY[0, 1] = np.nextafter(YY[0, 1], np.inf)
    with pytest.raises(ValueError, match=r"0.5\*\(YY\+YY.T\)"):
        GPRF(X, YY, None, cov, 0.01, kernelized=True, dy=3, block_idxs=[np.arange(20)], neighbors=[])
    with pytest.raises(ValueError, match="n x n"):
        GPRF(X, YY[:5], None, cov, 0.01, kernelized=True, dy=3, block_idxs=[np.arange(20)], neighbors=[])


@pytest.mark.parametrize("kw", [dict(shard=(0, 2)), dict(devices=[0, 0]), dict(nonstationary=True)])
def test_product_refuses_sharded_multi_device_and_nonstationary(kw):
    from gprf_amd.gprf import GPRF
    X, YY, cov = _product_args()
    with pytest.raises(NotImplementedError):
        GPRF(X, YY, None, cov, 0.01, kernelized=True, dy=3, block_idxs=[np.arange(20)], neighbors=[], **kw)


def test_c_abi_declares_and_binds_gprf_set_YY():
    from gprf_amd import _capi
    text = open(os.path.join(ROOT, "include", "gprf_hip.h")).read()
    assert re.search(r"int\s+gprf_set_YY\s*\(\s*gprf_ctx\s*\*\s*\w+\s*,\s*const\s+double\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)", text)
    assert "gprf_set_YY" in _capi.SIGNATURES
