"""Planar and spatial arm back to back on one device: 1024 problems of 7 joints x 20 timesteps, 5 link points, 2 obstacles.

Per workload: SCO iterations per second (sum of the problems' SQP iterations over the wall time of solve + fetch, as
bench.py counts them) and the five stages of sco_sqp_last_timing, each the median of the timed steps.  Recorded in
profiles/spatial_arm.md; nothing is gated on it.

    python scripts/gpu_spatial_speed.py [--batch 1024] [--steps 5] [--warmup 2]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sco_py_amd import batch as sb            # noqa: E402
from sco_py_amd import workloads as wl        # noqa: E402

STAGES = ("convexify_ms", "qp_setup_ms", "admm_ms", "decide_ms", "total_ms")


def run(name, B, steps, warmup, **kw):
    a, _ = wl.make_batch(B, d=7, T=20, K=5, O=2, **kw)
    geo = {k: a.get(k) for k in wl.SPATIAL_KEYS}
    rows = []
    with sb.TrajOptBatch(B, 7, 20, 5, 2, spatial=bool(a.get("spatial"))) as tb:
        tb.load(a["x0"], a["start"], a["goal"], a["link_len"], a["point_link"], a["point_frac"], a["obstacles"], **geo)
        for step in range(warmup + steps):
            t0 = time.perf_counter()
            tb.solve()
            res = tb.fetch()
            dt = time.perf_counter() - t0
            if step >= warmup:
                tm = tb.last_timing()
                rows.append([int(res.sqp_iters.sum()) / dt, dt * 1e3] + [tm[k] for k in STAGES] +
                            [tm["rounds"], tm["wv_launches"], int(res.admm_iters.sum()), int(res.qp_solves.sum()), int(res.success.sum())])
    med = np.median(np.array(rows, dtype=np.float64), axis=0)
    print("%-8s %9.0f SCO it/s  step %7.2f ms | convexify %7.2f  qp_setup %6.2f  admm %7.2f  decide %6.2f  total %7.2f ms | "
          "rounds %d  wavefront launches %d  ADMM iterations %d  QPs %d  solved %d / %d"
          % ((name,) + tuple(med[:7]) + tuple(int(v) for v in med[7:]) + (B,)), flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    p = run("planar", args.batch, args.steps, args.warmup)
    s = run("spatial", args.batch, args.steps, args.warmup, spatial=True)
    print("spatial / planar: step %.2f x, convexify %.2f x (%.2f ms more of %.2f ms more per step); "
          "convexify per round: planar %.3f ms, spatial %.3f ms"
          % (s[1] / p[1], s[2] / p[2], s[2] - p[2], s[6] - p[6], p[2] / p[7], s[2] / s[7]))


if __name__ == "__main__":
    main()
