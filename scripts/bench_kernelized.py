"""Time kernelized observations (GPRF(kernelized=True), gprf.py:674-736) on the north-star data (n = 10000, 100 blocks,
342 pairs, dy = 50, YY = Y Y^T): kernelized against plain evaluations per second (llgrad with the location gradient, the
optimiser's task x), and a dy = 1000 case — beyond the plain path's dy <= 64 — against its numpy restatement
(tests/kernelized_ref.py) on the host.  Prints one JSON line (medians)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(fn, reps, inner=1):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        ts.append((time.perf_counter() - t0) * 1e3 / inner)
    return float(np.median(ts))


def main():
    from gprf_amd import grid_centers
    from gprf_amd.gprf import GPRF
    from gprf_amd.synthetic import SampledData
    from oracle.vector_tree import GPCov as OC
    from kernelized_ref import KernelizedRef
    sd = SampledData(n=10500, ntrain=10000, lscale=0.06, obs_std=0.02, yd=50, seed=0, use_gpu=True)
    sd.set_centers(grid_centers(100))
    g = sd.build_gprf(local_dist=0.1)
    A = np.dot(sd.SY, sd.SY.T)
    YY = 0.5 * (A + A.T)
    del A
    k = GPRF(sd.X_obs, YY, sd.reblock, g.cov, g.noise_var, kernelized=True, dy=50, block_idxs=g.block_idxs,
             neighbors=list(g.neighbors))
    for h in (g, k):
        h.llgrad(grad_X=True)                                      # (warm-up)
    t_plain = _median_ms(lambda: g.llgrad(grad_X=True), 7, 20)
    t_kz = _median_ms(lambda: k.llgrad(grad_X=True), 7, 20)
    k.close()
    del YY

    # dy = 1000: an SE kernel over 1000-column outputs (no plain counterpart exists)
    rng = np.random.RandomState(0)
    Yw = np.tanh(np.dot(sd.SY, rng.randn(50, 1000)) / np.sqrt(50.0))
    sq = np.sum(Yw * Yw, axis=1)
    D = sq[:, None] + sq[None, :] - 2.0 * np.dot(Yw, Yw.T)
    D = 0.5 * (D + D.T)
    YYw = np.exp(-0.5 * np.maximum(D, 0.0) / 1000.0)
    del D
    kw = GPRF(sd.X_obs, YYw, sd.reblock, g.cov, g.noise_var, kernelized=True, dy=1000, block_idxs=g.block_idxs,
              neighbors=list(g.neighbors))
    kw.llgrad(grad_X=True)
    t_wide = _median_ms(lambda: kw.llgrad(grad_X=True), 7, 20)
    ll_dev = kw.llgrad(grad_X=True)
    ref = KernelizedRef(sd.X_obs, YYw, 1000, None, OC([1.0], [0.06, 0.06], "euclidean", "se"), g.noise_var,
                        block_idxs=[np.asarray(b) for b in g.block_idxs], neighbors=list(g.neighbors))
    t0 = time.perf_counter()
    ll_ref = ref.llgrad(grad_X=True)
    t_cpu = (time.perf_counter() - t0) * 1e3
    kw.close()
    print(json.dumps({"metric": "kernelized_northstar", "n": 10000, "blocks": g.n_blocks, "pairs": len(g.neighbors),
                      "plain_dy50_ms": round(t_plain, 4), "kernelized_dy50_ms": round(t_kz, 4),
                      "plain_dy50_evals_per_s": round(1e3 / t_plain, 1), "kernelized_dy50_evals_per_s": round(1e3 / t_kz, 1),
                      "kernelized_dy1000_ms": round(t_wide, 4), "cpu_restatement_dy1000_ms": round(t_cpu, 1),
                      "dy1000_ll_rel_diff": float(abs(ll_dev[0] - ll_ref[0]) / abs(ll_ref[0])),
                      "dy1000_gradX_rel_diff": float(np.max(np.abs(ll_dev[1] - ll_ref[1])) / np.max(np.abs(ll_ref[1])))}))
    g.close()


if __name__ == "__main__":
    main()
