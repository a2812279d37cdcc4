"""Time GPRF prediction on the north-star data (n = 10000, 100 blocks, 342 pairs, 500 test points): train_predictor and
one predict_blocks call over every test block (the loop of the reference's prediction_error, gprfopt.py:121-170), next to
the numpy restatement (tests/predict_ref.py) of the same predict_blocks on the host.  Prints one JSON line (ms, medians)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _median_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def main():
    from gprf_amd import grid_centers
    from gprf_amd.synthetic import SampledData
    from oracle.vector_tree import GPCov as OC
    from predict_ref import PredictorRef
    sd = SampledData(n=10500, ntrain=10000, lscale=0.06, obs_std=0.02, yd=50, seed=0, use_gpu=True)
    sd.set_centers(grid_centers(100))
    g = sd.build_gprf(local_dist=0.1)
    nv = sd.noise_var
    g.train_predictor().close()                                    # (warm-up: module load, first launches)

    def train():
        train.p = g.train_predictor()
    t_train = _median_ms(lambda: (train(), train.p.close()), 7)
    p = g.train_predictor()
    p.predict_blocks(sd.Xtest, test_noise_var=nv)
    t_pred = _median_ms(lambda: p.predict_blocks(sd.Xtest, test_noise_var=nv), 7)
    blocks = p.predict_blocks(sd.Xtest, test_noise_var=nv)[0]
    p.close()
    ref = PredictorRef(g.X, g.Y, g.block_idxs, g.neighbor_dict, g.block_fn, OC([1.0], [0.06, 0.06], "euclidean", "se"), nv)
    t_cpu = _median_ms(lambda: ref.predict_blocks(sd.Xtest, test_noise_var=nv), 3)
    print(json.dumps({"metric": "predict_northstar_ms", "n": 10000, "blocks": g.n_blocks, "pairs": len(g.neighbors),
                      "test_points": int(sd.Xtest.shape[0]), "test_blocks": len(blocks),
                      "train_predictor_ms": round(t_train, 3), "predict_blocks_ms": round(t_pred, 3),
                      "cpu_restatement_predict_blocks_ms": round(t_cpu, 3)}))
    g.close()


if __name__ == "__main__":
    main()
