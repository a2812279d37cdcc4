"""Launch structure of prediction: run under `rocprofv3 --kernel-trace --output-format csv -d <dir> -- python
scripts/gpu_predict_launches.py`, then `python scripts/gpu_predict_launches.py --trace <dir>` lists the kernels launched
after the predictor build: one predict_blocks call over 100 test groups, then one predict call (one group).  Both must
be the same five prediction kernels of the library, nothing else."""
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    from gprf_amd import GPCov, grid_centers
    from gprf_amd.blocking import Blocker
    from gprf_amd.gprf import GPRF
    rng = np.random.RandomState(0)
    X, Y, Xt = rng.rand(10000, 2), rng.randn(10000, 50), rng.rand(500, 2)
    b = Blocker(grid_centers(100))
    g = GPRF(X, Y, b.block_clusters, GPCov([1.0], [0.06, 0.06], "euclidean", "se"), 0.01,
             neighbors=b.neighbors(diag_connections=True))
    p = g.train_predictor()
    blocks, _, _ = p.predict_blocks(Xt, test_noise_var=0.01)
    p(Xt[:50], test_noise_var=0.01)
    p.close()
    g.close()
    print("groups in predict_blocks: %d" % len(blocks))


def summarize(d):
    import csv
    import re
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[-1]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    last = max(i for i, n in enumerate(names) if "k_pred_gather" in n)
    after = [(re.search(r"\b(k_\w+)", n) or re.search(r"(\S+)", n)).group(1) for n in names[last + 1:]]
    print("kernels after the predictor build: %s" % " ".join(after))
    return after


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--trace":
        summarize(sys.argv[2])
    else:
        run()
