"""GPRF prediction on the device (GPRF.train_predictor / predict / predict_blocks, gprf.py:593-672) against the numpy
restatement tests/predict_ref.py and, for one block, the exact GP posterior.

Tolerance.  The device inverts through Cholesky factors and applies K_i^-1 as W^T W (W = L_i^-1); the restatement, like the
reference, uses LU (np.linalg.inv / solve).  Both are rounded at about cond * eps.  Every check measures that floor on its
own inputs — the restatement with LU against the restatement on the device's Cholesky route (predict_ref, inv="chol") —
and bounds the device by ten times it (blocks: the worst block's spread), never looser than 1e-9 of max|mean| / max|cov| (`_bound`).  Spreads measured on
CPU on these inputs (max abs difference / max abs value; mean | cov):
  one block, n = 2000, t = 500:                       2.6e-12 | 4.3e-13  (exact posterior vs Cholesky route 2.2e-12 | 4.4e-13)
  north star, 100 blocks, no pairs / 342 pairs:       7.1e-13 | 4.4e-13,  7.1e-13 | 4.8e-13  (worst block)
  lld / matern32 stand-in catalogue, 15 blocks:       1.3e-15 | 2.2e-15  (worst block); with the kernel values 4 ulps apart
                                                      (kernel_ulps=4, the device's own exp / haversine forms) 6.4e-15 | 2.9e-15
  Y= and test_cov=, test_noise_var = 0:               5.5e-13 | 6.9e-13  (one group),  1.2e-12 | 1.5e-12  (worst block)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NV = 0.01


def _bound(spread, scale):
    return min(10.0 * max(spread, 1e-15 * scale), 1e-9 * scale)


def _rel(a, b):
    return np.max(np.abs(a - b)) / np.max(np.abs(a))


def _close(got, lu, alts, what):
    """|device - LU restatement| <= _bound(|LU - alternative restatement|); alts: the alternatives (arrays), or the spread
    itself, relative to max|LU|, measured over the whole test"""
    scale = np.max(np.abs(lu))
    spread = alts if np.isscalar(alts) else max(_rel(lu, a) for a in alts)
    err = np.max(np.abs(got - lu))
    assert err <= _bound(spread * scale, scale), "%s: err %.3e  spread %.3e  scale %.3e" % (what, err, spread * scale, scale)


def _close_blocks(got, ref, alts, what):
    """the blocks of predict_blocks: every block bounded by the worst block's spread"""
    spread = max(_rel(ref[k][b], a[k][b]) for a in alts for k in (1, 2) for b in range(len(ref[0])))
    for b in range(len(ref[0])):
        _close(got[1][b], ref[1][b], spread, "mean of %s block %d" % (what, b))
        _close(got[2][b], ref[2][b], spread, "cov of %s block %d" % (what, b))


def _ref(g, Y=None, test_cov=None, how="lu", kernel_ulps=0):
    from predict_ref import PredictorRef
    from oracle.vector_tree import GPCov as OC
    c = g.cov
    tc = None if test_cov is None else OC(test_cov.wfn_params, test_cov.dfn_params, test_cov.dfn_str, test_cov.wfn_str)
    return PredictorRef(g.X, g.Y if Y is None else Y, g.block_idxs, g.neighbor_dict, g.block_fn,
                        OC(c.wfn_params, c.dfn_params, c.dfn_str, c.wfn_str), g.noise_var, test_cov=tc, inv=how,
                        kernel_ulps=kernel_ulps)


def test_one_block_exact_gp():
    """n = 2000 in ONE block (the blocked path's W) and 500 test points in one group: the exact GP posterior"""
    from gprf_amd import GPCov
    from gprf_amd.gprf import GPRF
    from predict_ref import exact_posterior, PredictorRef
    from oracle.vector_tree import GPCov as OC
    rng = np.random.RandomState(0)
    X, Xs = rng.rand(2000, 2), rng.rand(500, 2)
    Y = rng.randn(2000, 3)
    cov = GPCov([1.0], [0.1, 0.1], "euclidean", "se")
    one = lambda Z: [np.arange(len(Z))]
    g = GPRF(X, Y, one, cov, NV, neighbors=[])
    p = g.train_predictor()
    mean, pc = p(Xs, test_noise_var=NV)
    p.close()
    g.close()
    em, ec = exact_posterior(X, Y, Xs, OC([1.0], [0.1, 0.1], "euclidean", "se"), NV)
    ch = PredictorRef(X, Y, [np.arange(2000)], {}, one, OC([1.0], [0.1, 0.1], "euclidean", "se"), NV, inv="chol")
    cm, cc = ch(Xs, test_noise_var=NV)
    _close(mean, em, [cm], "mean")
    _close(pc, ec, [cc], "cov")


@pytest.fixture(scope="module")
def sdata():
    from gprf_amd.synthetic import SampledData
    from gprf_amd import grid_centers
    sd = SampledData(n=10500, ntrain=10000, lscale=0.06, obs_std=0.02, yd=50, seed=0, use_gpu=True)
    sd.set_centers(grid_centers(100))
    return sd


@pytest.mark.parametrize("local_dist", [1.0, 0.1])
def test_northstar_blocks(sdata, local_dist):
    from gprf_amd.predict import prediction_error
    g = sdata.build_gprf(local_dist=local_dist)
    assert len(g.neighbors) == (0 if local_dist == 1.0 else 342)
    p = g.train_predictor()
    blocks, means, covs = p.predict_blocks(sdata.Xtest, test_noise_var=NV)
    p.close()
    assert sum(len(b) for b in blocks) == 500 and len(blocks) > 50
    ref = _ref(g).predict_blocks(sdata.Xtest, test_noise_var=NV)
    rb, rm, rc = ref
    assert all(np.array_equal(a, b) for a, b in zip(blocks, rb))
    _close_blocks((blocks, means, covs), ref, [_ref(g, how="chol").predict_blocks(sdata.Xtest, test_noise_var=NV)], "north-star")
    got = np.array(prediction_error(g, sdata.Xtest, sdata.Ytest, sdata.SY, NV))
    g.close()
    # the same three numbers from the restatement's blocks (gprfopt.py:121-170), the Gaussian log-likelihood restated here
    from scipy.stats import multivariate_normal

    def _gaussian_ll(Yt, M, C):
        return sum(multivariate_normal(mean=M[:, d], cov=C).logpdf(Yt[:, d]) for d in range(Yt.shape[1]))
    ll_b = sum(_gaussian_ll(sdata.Ytest[b], m, c) for b, m, c in zip(rb, rm, rc))
    ll_d = sum(_gaussian_ll(sdata.Ytest[b], m, np.diag(np.diag(c))) for b, m, c in zip(rb, rm, rc))
    se = sum(np.sum((sdata.Ytest[b] - m) ** 2) for b, m in zip(rb, rm))
    Ym, Ys = sdata.SY.mean(0), sdata.SY.std(0)
    nt = sdata.Ytest.size
    base = np.sum(-0.5 * np.log(2 * np.pi * Ys ** 2) - (sdata.Ytest - Ym) ** 2 / (2 * Ys ** 2)) / nt
    want = np.array([se / np.sum((sdata.Ytest - Ym) ** 2), ll_b / nt - base, ll_d / nt - base])
    assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (got, want)
    assert 0.0 < got[0] < 1.0


def test_lld_matern32():
    from gprf_amd import GPCov, seismic
    from gprf_amd.gprf import GPRF
    n = 480
    X = seismic.synthetic_events(n + 60, seed=2)
    cov = GPCov([1.0], [150.0, 150.0], "lld", "matern32")
    Y = seismic.sample_y(X, cov, 0.1, 3, seed=2)
    Xtr, Xte = X[:n], X[n:]
    blocks, reblock = seismic.pdtree_cluster(Xtr, blocksize=60)
    g = GPRF(Xtr, Y[:n], reblock, cov, 0.1, neighbor_threshold=0.6)
    assert len(g.neighbors) > 0
    p = g.train_predictor()
    blocks, means, covs = p.predict_blocks(Xte, test_noise_var=0.1)
    p.close()
    ref = _ref(g).predict_blocks(Xte, test_noise_var=0.1)
    # (the device evaluates the great-circle Matern with its own exp / haversine forms: the floor includes kernel values a
    # few ulps apart)
    alts = [_ref(g, how="chol").predict_blocks(Xte, test_noise_var=0.1),
            _ref(g, how="chol", kernel_ulps=4).predict_blocks(Xte, test_noise_var=0.1)]
    g.close()
    assert len(blocks) == len(ref[0]) > 1 and all(np.array_equal(a, b) for a, b in zip(blocks, ref[0]))
    _close_blocks((blocks, means, covs), ref, alts, "lld")


def _small():
    from gprf_amd import GPCov, grid_centers
    from gprf_amd.blocking import Blocker
    from gprf_amd.gprf import GPRF
    rng = np.random.RandomState(4)
    X = rng.rand(900, 2)
    Y = rng.randn(900, 5)
    b = Blocker(grid_centers(9))
    g = GPRF(X, Y, b.block_clusters, GPCov([1.0], [0.15, 0.15], "euclidean", "se"), NV,
             neighbors=b.neighbors(diag_connections=True))
    return g, rng


def test_y_and_test_cov_arguments():
    """Y= replaces the targets of the alphas; test_cov= the prior; test_noise_var = 0 on well-separated test points
    (a 6 x 6 lattice, spacing 0.18 > the lengthscale: Kss is well conditioned without noise)"""
    from gprf_amd import GPCov
    g, rng = _small()
    Y2 = rng.randn(900, 5)
    tc = GPCov([2.0], [0.2, 0.25], "euclidean", "se")
    u = (np.arange(6) + 0.5) / 6.0
    Xs = np.stack(np.meshgrid(u, u), -1).reshape(-1, 2)
    p = g.train_predictor(test_cov=tc, Y=Y2)
    mean, cov = p(Xs, test_noise_var=0.0)
    blocks, bm, bc = p.predict_blocks(Xs, test_noise_var=0.0)
    p.close()
    m_lu, c_lu = _ref(g, Y=Y2, test_cov=tc)(Xs, test_noise_var=0.0)
    m_ch, c_ch = _ref(g, Y=Y2, test_cov=tc, how="chol")(Xs, test_noise_var=0.0)
    _close(mean, m_lu, [m_ch], "mean")
    _close(cov, c_lu, [c_ch], "cov")
    ref = _ref(g, Y=Y2, test_cov=tc).predict_blocks(Xs, test_noise_var=0.0)
    _close_blocks((blocks, bm, bc), ref, [_ref(g, Y=Y2, test_cov=tc, how="chol").predict_blocks(Xs, test_noise_var=0.0)],
                  "Y=/test_cov=")
    # the context's own targets are untouched: a predictor without Y= sees them
    p0 = g.train_predictor()
    m0, _ = p0(Xs, test_noise_var=0.0)
    p0.close()
    _close(m0, _ref(g)(Xs)[0], [_ref(g, how="chol")(Xs)[0]], "mean with the model's Y")
    g.close()


def test_snapshot_and_refusals():
    from gprf_amd import GPCov
    from gprf_amd.gprf import GPRF
    g, rng = _small()
    Xs = rng.rand(40, 2)
    p = g.train_predictor()
    a = p.predict_blocks(Xs, test_noise_var=NV)
    a1 = p(Xs[:10], test_noise_var=NV)
    g.update_X(g.X + rng.randn(*g.X.shape) * 0.02)
    g.llgrad(grad_X=True, grad_cov=True)
    b = p.predict_blocks(Xs, test_noise_var=NV)
    b1 = p(Xs[:10], test_noise_var=NV)
    assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0]))
    assert all(np.array_equal(x, y) for k in (1, 2) for x, y in zip(a[k], b[k]))
    assert all(np.array_equal(x, y) for x, y in zip(a1, b1))
    with pytest.raises(ValueError):
        p(rng.rand(513, 2))
    p.close()
    g.close()
    X, Y = rng.rand(200, 2), rng.randn(200, 2)
    cov = GPCov([1.0], [0.2, 0.2], "euclidean", "se")
    blocks = [np.arange(100), np.arange(100, 200)]
    for kw in ({"shard": (0, 2), "reduce": False}, {"devices": [0, 0]}):
        h = GPRF(X, Y, None, cov, NV, block_idxs=blocks, neighbors=[], **kw)
        with pytest.raises(NotImplementedError):
            h.train_predictor()
        h.close()


def test_empty_sources_give_the_prior():
    """test points whose block is empty in training and has no neighbours: no source at all, the result is the prior
    (mean 0, cov = k_test(X*, X*) + test_noise_var I) — also right after a prediction with sources used the same workspace"""
    from gprf_amd import GPCov
    from gprf_amd.gprf import GPRF
    from predict_ref import PredictorRef
    from oracle.vector_tree import GPCov as OC
    rng = np.random.RandomState(7)
    X, Y, Xs = rng.rand(200, 2), rng.randn(200, 3), rng.rand(30, 2)
    blocks = [np.arange(100), np.arange(100, 200), np.zeros(0, np.int64)]
    fn = lambda Z: [np.zeros(0, np.int64), np.zeros(0, np.int64), np.arange(len(Z))]
    g = GPRF(X, Y, fn, GPCov([1.0], [0.2, 0.2], "euclidean", "se"), NV, block_idxs=blocks, neighbors=[(1, 0)])
    p = g.train_predictor()
    oc = OC([1.0], [0.2, 0.2], "euclidean", "se")
    lu = PredictorRef(X, Y, blocks, g.neighbor_dict, fn, oc, NV)
    ch = PredictorRef(X, Y, blocks, g.neighbor_dict, fn, oc, NV, inv="chol")
    for tnv in (NV, 0.5 * NV):
        m1, c1 = p._impl.predict(Xs, [np.arange(30)], [[0, 1]], p._prior_theta, tnv)      # (fills the workspace)
        _close(m1[0], lu.predict_from(Xs, [0, 1], tnv)[0], [ch.predict_from(Xs, [0, 1], tnv)[0]], "mean with sources")
        mean, cov = p(Xs, test_noise_var=tnv)
        assert np.array_equal(mean, np.zeros((30, 3)))
        want, alt = lu(Xs, test_noise_var=tnv), ch(Xs, test_noise_var=tnv)
        prior = lu.test_tree.kernel_matrix(Xs, Xs, False) + tnv * np.eye(30)
        _close(want[1], prior, [alt[1]], "restatement = prior")
        _close(cov, want[1], [alt[1]], "cov")
        _close(cov, prior, [alt[1]], "cov = prior")
        # an explicitly empty source list and an empty block listed as a source: the same
        m2, c2 = p._impl.predict(Xs, [np.arange(30), np.arange(30)], [[], [2]], p._prior_theta, tnv)
        assert np.array_equal(c2[0], cov) and np.array_equal(c2[1], cov)
        assert not np.any(m2[0]) and not np.any(m2[1])
    p.close()
    g.close()
