"""Kernelized observations on the device (GPRF(X, YY, ..., kernelized=True, dy=D); gaussian_llgrad_kernel, gprf.py:674-736)
against the numpy restatement tests/kernelized_ref.py and, with YY = Y Y^T, against the plain (dense) GPRF on the same object
state.

Tolerance.  The device takes P = K^-1 through the Cholesky factor (P = W^T W, W = U^-T); the restatement, like the reference,
through np.linalg.inv / slogdet.  Every check evaluates the restatement on both routes on its own inputs and bounds the device
by ten times their spread (`_bound`: max abs difference, never tighter than 1e-15 of the largest magnitude).  Spreads measured
on CPU on these inputs (max abs difference / max abs value; ll | gradX | gradC):
  north star, 100 blocks + 342 pairs, dy = 50, YY = Y Y^T:        4.5e-15 | 6.4e-12 | 1.1e-14
  dy = 300, YY = Y Y^T / SE kernel over the rows of Y:            1.1e-15 | 2.5e-12 | 2.1e-13  /  3.0e-16 | 3.4e-12 | 2.9e-15
  size classes (units of 300 ... 1950 points):                    1.0e-15 | 2.3e-12 | 6.5e-16
  n = 500, 4 blocks + 6 pairs (tests 4, 7, 8, 9), dy = 10:        1.5e-15 | 1.1e-12 | 6.8e-15
  lld / matern32, seismic stand-in (7 pairs):                     0       | 6.0e-15 | 2.7e-15
(the bounds are computed from the spreads in the test itself, not from this table).  The objective comparison of the L-BFGS-B
run bounds |f_kernelized - f_plain| by ten times the ll spread at the starting point, floored at 1e-14 of |f|.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NV = 0.01


def _bound(spread, scale):
    return 10.0 * max(spread, 1e-15 * scale)


def _check(got, ref, alt, what, other=None):
    """|got - ref| <= 10 |ref - alt| (abs, max over entries); other: a second result held to the same bound"""
    got, ref, alt = (np.atleast_1d(np.asarray(v, dtype=np.float64)).ravel() for v in (got, ref, alt))
    scale = max(np.max(np.abs(ref)), 1e-300)
    b = _bound(np.max(np.abs(ref - alt)), scale)
    err = np.max(np.abs(got - ref))
    assert err <= b, "%s: err %.3e  bound %.3e  (spread %.3e, scale %.3e)" % (what, err, b, np.max(np.abs(ref - alt)), scale)
    if other is not None:
        err2 = np.max(np.abs(np.atleast_1d(np.asarray(other, dtype=np.float64)).ravel() - got))
        assert err2 <= b, "%s (kernelized vs plain): err %.3e  bound %.3e" % (what, err2, b)


def _oc(cov):
    from oracle.vector_tree import GPCov as OC
    return OC(list(cov.wfn_params), list(cov.dfn_params), cov.dfn_str, cov.wfn_str)


def _refs(g, YY, dy, **kw):
    from kernelized_ref import KernelizedRef
    blocks = [np.asarray(b, dtype=np.int64) for b in g.block_idxs]
    return [KernelizedRef(np.array(g.X, dtype=np.float64), YY, dy, None, _oc(g.cov), kw.get("nv", g.noise_var), inv=how,
                          block_idxs=blocks, neighbors=list(g.neighbors)) for how in ("inv", "chol")]


def _compare(g, YY, dy, what, plain=None, local=True, nv=None):
    kw = {} if nv is None else {"nv": nv}
    got = g.llgrad(local=local, grad_X=True, grad_cov=True)      # (first: a pending re-blocking runs inside the evaluation)
    ri, rc = _refs(g, YY, dy, **kw)
    a = ri.llgrad(local=local, grad_X=True, grad_cov=True)
    b = rc.llgrad(local=local, grad_X=True, grad_cov=True)
    p = plain.llgrad(local=local, grad_X=True, grad_cov=True) if plain is not None else (None, None, None)
    _check(got[0], a[0], b[0], what + " ll", p[0])
    _check(got[1], a[1], b[1], what + " gradX", p[1])
    _check(got[2], a[2], b[2], what + " gradC", p[2])
    return got


def _gram(Y):
    A = np.dot(Y, Y.T)
    return 0.5 * (A + A.T)      # (exactly symmetric: IEEE addition commutes)


def _kz(g, YY, dy, block_fn=None, **kw):
    from gprf_amd.gprf import GPRF
    return GPRF(np.array(g.X, dtype=np.float64), YY, block_fn, g.cov, g.noise_var, kernelized=True, dy=dy,
                block_idxs=[np.asarray(b) for b in g.block_idxs], neighbors=list(g.neighbors), **kw)


def test_north_star_against_plain_and_restatement():
    """1. 100 blocks + 342 pairs, dy = 50, YY = Y Y^T: the kernelized GPRF against the plain one and the restatement"""
    from gprf_amd.synthetic import SampledData
    from gprf_amd import grid_centers
    sd = SampledData(n=10500, ntrain=10000, lscale=0.06, obs_std=0.02, yd=50, seed=0, use_gpu=True)
    sd.set_centers(grid_centers(100))
    g = sd.build_gprf(local_dist=0.1)
    assert len(g.neighbors) == 342
    k = _kz(g, _gram(sd.SY), 50, block_fn=sd.reblock)
    assert k.kernelized and k.dy == 50 and not hasattr(k, "Y") and k.YY.shape == (10000, 10000)
    _compare(k, k.YY, 50, "north star", plain=g)
    k.close()
    g.close()


def test_dy_beyond_the_plain_limit():
    """2. Y with 300 columns: the plain GPRF is refused at creation; YY = Y Y^T and an SE kernel over the rows of Y"""
    from gprf_amd import GPCov, _capi
    from gprf_amd.gprf import GPRF
    rng = np.random.RandomState(11)
    n = 1200
    X = rng.rand(n, 2)
    Y = np.sin(6.0 * np.dot(X, rng.randn(2, 300))) + 0.1 * rng.randn(n, 300)
    blocks = [np.flatnonzero((X[:, 0] >= 0.5 * (b // 2)) & (X[:, 0] < 0.5 * (b // 2) + 0.5) &
                             (X[:, 1] >= 0.5 * (b % 2)) & (X[:, 1] < 0.5 * (b % 2) + 0.5)) for b in range(4)]
    nbrs = [(1, 0), (2, 0), (3, 1)]
    cov = GPCov([1.0], [0.15, 0.15], "euclidean", "se")
    with pytest.raises(_capi.GprfHipError):
        GPRF(X, Y, None, cov, NV, block_idxs=blocks, neighbors=nbrs)
    sq = np.sum(Y * Y, axis=1)
    D = sq[:, None] + sq[None, :] - 2.0 * np.dot(Y, Y.T)
    D = 0.5 * (D + D.T)
    for YY, what in ((_gram(Y), "Y Y^T"), (np.exp(-0.5 * np.maximum(D, 0.0) / 300.0), "SE over Y")):
        assert np.array_equal(YY, YY.T)
        k = GPRF(X, YY, None, cov, NV, kernelized=True, dy=300, block_idxs=blocks, neighbors=nbrs)
        _compare(k, YY, 300, "dy=300 " + what)
        k.close()


def test_every_size_class():
    """3. units of <= 512, 513-1024 and > 1024 points (the one-workgroup kernels, the blocked Cholesky with k_mgrad's own
    walk, and the big-unit path)"""
    from gprf_amd import GPCov
    from gprf_amd.gprf import GPRF
    rng = np.random.RandomState(12)
    sizes = [300, 450, 1500]
    n = sum(sizes)
    X = rng.rand(n, 2)
    Y = rng.randn(n, 20)
    perm = rng.permutation(n)
    blocks = np.split(perm, np.cumsum(sizes)[:-1])
    nbrs = [(1, 0), (2, 1)]      # pairs of 750 and 1950 points
    cov = GPCov([1.0], [0.1, 0.1], "euclidean", "se")
    YY = _gram(Y)
    k = GPRF(X, YY, None, cov, NV, kernelized=True, dy=20, block_idxs=blocks, neighbors=nbrs)
    p = GPRF(X, Y, None, cov, NV, block_idxs=blocks, neighbors=nbrs)
    _compare(k, YY, 20, "size classes", plain=p)
    k.close()
    p.close()


def _c1_like():
    from gprf_amd.synthetic import SampledData
    from gprf_amd import grid_centers
    sd = SampledData(n=1000, ntrain=500, lscale=0.4, obs_std=0.04, yd=10, seed=0)
    sd.set_centers(grid_centers(4))
    return sd


def test_reblocking_subset_and_all_pairs():
    """4. update_X with points that change block (re-blocking on the device), llgrad; subset_llgrad; local=False"""
    sd = _c1_like()
    g = sd.build_gprf(local_dist=0.5)
    YY = _gram(sd.SY)
    k = _kz(g, YY, 10, block_fn=sd.reblock)
    before = [np.sort(b) for b in k.block_idxs]
    rng = np.random.RandomState(13)
    Xn = sd.X_obs + 0.08 * rng.randn(*sd.X_obs.shape)
    k.update_X(Xn)
    g.update_X(Xn)
    got = _compare(k, YY, 10, "after update_X", plain=g)
    after = [np.sort(b) for b in k.block_idxs]
    assert any(len(a) != len(b) or not np.array_equal(a, b) for a, b in zip(before, after))
    ri, rc = _refs(k, YY, 10)
    _check(k.subset_llgrad([0, 1]), ri.subset_llgrad([0, 1]), rc.subset_llgrad([0, 1]), "subset_llgrad",
           g.subset_llgrad([0, 1]))
    _compare(k, YY, 10, "local=False", plain=g, local=False)
    assert k.llgrad(grad_X=True)[0] == got[0]          # (and back to the object's own state)
    k.close()
    g.close()


def test_lld_matern32_seismic_stand_in():
    """5. ("lld", "matern32") on the seismic stand-in catalogue (principal-direction-tree blocks)"""
    from gprf_amd import GPCov, seismic
    from gprf_amd.gprf import GPRF
    n, yd = 420, 4
    Xtrue = seismic.synthetic_events(n, seed=0)
    theta = (0.1, 1.0, 150.0, 150.0)
    cov = GPCov([theta[1]], list(theta[2:]), "lld", "matern32")
    Y = seismic.sample_y(Xtrue, cov, theta[0], yd, seed=0)
    rng = np.random.RandomState(1)
    Xobs = Xtrue + rng.randn(n, 3) * 2.0 * np.array([.01, .01, 1.0])
    Xobs[:, 2] = np.abs(Xobs[:, 2])
    blocks, reblock = seismic.pdtree_cluster(Xobs, blocksize=60)
    g = GPRF(Xobs, Y, reblock, cov, theta[0], neighbor_threshold=0.6)
    assert len(g.neighbors) > 0
    YY = _gram(Y)
    k = _kz(g, YY, yd, block_fn=reblock)
    _compare(k, YY, yd, "lld/matern32")
    k.close()
    g.close()


def test_jitter_path_as_plain():
    """6. duplicate points, zero noise: the same jitchol schedule and the same result as the plain path with Y Y^T"""
    from conftest import load_golden
    from gprf_amd import GPCov
    from gprf_amd.gprf import GPRF
    z = load_golden("degenerate.npz")
    X, Y, th = z["dup_X"], z["dup_Y"], z["dup_theta"]
    cov = GPCov([th[1]], th[2:], "euclidean", "se")
    p = GPRF(X, Y, None, cov, th[0], block_idxs=[np.arange(24)], neighbors=[])
    YY = _gram(Y)
    k = GPRF(X, YY, None, cov, th[0], kernelized=True, dy=Y.shape[1], block_idxs=[np.arange(24)], neighbors=[])
    pr = p.llgrad(grad_X=True, grad_cov=True)
    kr = k.llgrad(grad_X=True, grad_cov=True)
    assert k._jitter is not None and np.array_equal(k._jitter, p._jitter)
    # the restatement on the jittered matrix: K + j I = the kernel with noise variance nv + j
    ri, rc = _refs(k, YY, Y.shape[1], nv=th[0] + k._jitter[0])
    a = ri.llgrad(grad_X=True, grad_cov=True)
    b = rc.llgrad(grad_X=True, grad_cov=True)
    for t, what in enumerate(("ll", "gradX", "gradC")):
        _check(kr[t], a[t], b[t], "jitter " + what, pr[t])
    k.close()
    p.close()


def test_lbfgs_xcov_kernelized_against_plain():
    """7. ten L-BFGS-B iterations through Objective, task xcov (locations and the tied lengthscale, HYPER_TIED): the objective
    values of the kernelized model along its own iterates equal the plain model's at the same points"""
    import scipy.optimize
    from gprf_amd.objective import Objective
    from gprf_amd import _capi
    sd = _c1_like()
    g = sd.build_gprf(local_dist=0.5)
    YY = _gram(sd.SY)
    k = _kz(g, YY, 10, block_fn=sd.reblock)
    C0 = np.array([[0.35]])
    ok = Objective(k, sd.X_obs, C0, sd)
    op = Objective(g, sd.X_obs, C0, sd)
    assert ok.layout.mode == _capi.HYPER_TIED and ok._native
    # the rounding floor at the starting point: the restatement's two routes on the starting state
    ri, rc = _refs(k, YY, 10)
    spread = abs(ri.llgrad()[0] - rc.llgrad()[0])
    zs, fs = [], []

    def f(z):
        v = ok(z)
        zs.append(z.copy())
        fs.append(v[0])
        return v
    scipy.optimize.minimize(f, ok.full0, jac=True, method="l-bfgs-b", options={"ftol": 1e-6, "maxiter": 10})
    assert len(zs) >= 10
    for z, fk in zip(zs, fs):
        fp = op(z)[0]
        assert abs(fk - fp) <= 10.0 * max(spread, 1e-14 * abs(fp)), (fk, fp, spread)
    assert fs[-1] < fs[0]
    ok.close()
    op.close()
    k.close()
    g.close()


def test_refusals_and_predictor():
    """8. dy=None, a non-symmetric YY, shard= / devices=, gprf_set_Y on a kernelized context (and gprf_set_YY on a plain one),
    train_predictor without Y=; with Y= the predictor equals the plain model's"""
    from gprf_amd import _capi
    from gprf_amd.gprf import GPRF
    sd = _c1_like()
    g = sd.build_gprf(local_dist=0.5)
    YY = _gram(sd.SY)
    with pytest.raises(ValueError, match="dy"):
        _kz(g, YY, None)
    bad = YY.copy()
    bad[2, 5] = np.nextafter(bad[2, 5], np.inf)
    with pytest.raises(ValueError, match=r"0.5\*\(YY\+YY.T\)"):
        _kz(g, bad, 10)
    with pytest.raises(NotImplementedError):
        _kz(g, YY, 10, shard=(0, 1))
    with pytest.raises(NotImplementedError):
        _kz(g, YY, 10, devices=[0])
    k = _kz(g, YY, 10, block_fn=sd.reblock)
    with pytest.raises(_capi.GprfHipError, match=r"\(-3\)"):
        k._ctx.set_Y(sd.SY)
    with pytest.raises(_capi.GprfHipError, match=r"\(-3\)"):
        g._ctx.set_YY(YY, 10)
    with pytest.raises(ValueError, match="Y="):
        k.train_predictor()
    pk = k.train_predictor(Y=sd.SY)
    pp = g.train_predictor()
    Xs = np.random.RandomState(14).rand(40, 2)
    mk, ck = pk(Xs, test_noise_var=NV)
    mp_, cp = pp(Xs, test_noise_var=NV)
    assert np.array_equal(mk, mp_) and np.array_equal(ck, cp)
    pk.close()
    pp.close()
    # the kernelized model still evaluates after the predictor was built from it
    assert np.isfinite(k.llgrad()[0])
    k.close()
    g.close()


def test_plain_path_unchanged_by_a_kernelized_context():
    """9. in one process: a plain GPRF gives the same bits before and after a kernelized one was built and evaluated"""
    sd = _c1_like()
    g = sd.build_gprf(local_dist=0.5)
    first = g.llgrad(grad_X=True, grad_cov=True)
    k = _kz(g, _gram(sd.SY), 10, block_fn=sd.reblock)
    k.llgrad(grad_X=True, grad_cov=True)
    k.close()
    g2 = sd.build_gprf(local_dist=0.5)
    for h in (g, g2):
        again = h.llgrad(grad_X=True, grad_cov=True)
        assert again[0] == first[0]
        assert np.array_equal(again[1], first[1]) and np.array_equal(again[2], first[2])
    g.close()
    g2.close()
