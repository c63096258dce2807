"""A THIRD fp32 implementation's IPO end-state ensembles (CPU only, numpy oracle): tests/golden/<capture>_ipoens_oracle.npz.

tests/test_ensemble_gpu.py holds the HIP kernels' IPO end state (500 Adam iterations, reference run/opt_main.py:180-195) against
the reference's as DISTRIBUTIONS - 201-point quantile functions of rotation angle, depth scale and end-state loss over the 50 750
fits of BASELINE configs[2], ensemble mean against ensemble mean - and finds them 3-7 single-member standard deviations apart at
the worst quantile, signs changing from draw to draw.  DESIGN.md attributes that to the order of the sum over joints.  This script
puts the claim to the test with an implementation that shares NO code with either side: oracle/zedo_oracle.py::ipo_fit (numpy,
float32, numpy's own pairwise sums), run on ulp-perturbed copies of the three captures' detections (streams 2001, 2002, ...:
disjoint from the reference's 1.. and the kernels' 101..) and summarised by the same tests/_ipo_summary.py.  The oracle is test
infrastructure; this script does not import the reference (the reference-side members are tools/gen_golden.py::gen_driver_pw3d_ipoens).

    python tools/gen_oracle_ipoens.py [--members 12] [--workers 6] [--draws a,b,c]      # ~2 CPU-minutes per member
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "zedo-release_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden")
SEED0 = 2000
DRAWS = {"a": "driver_pw3d_full", "b": "driver_pw3d_full_b", "c": "driver_pw3d_full_c"}       # seeds and settings: the fixtures' own


def member(task):
    draw, run = task
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import _ipo_summary as ips
    import zedo_oracle as O
    from _shared import Capture
    tag = DRAWS[draw]
    cap = Capture(tag)
    N, H, K = cap.N, cap.H, cap.K
    KEYLIST, IPO_T, MIN_T = [int(k) for k in cap.g["keylist"]], float(cap.g["ipo_T"]), float(cap.g["minT"])
    uv = np.ascontiguousarray(cap.detections(SEED0 + run)[:, :, :2])
    x0c = (cap.cl - cap.cl[:, 0:1, :]).astype(np.float32)
    t0 = time.time()
    T0 = O.ipo_init_T(uv, K, IPO_T)
    cs, Ts = [], []
    for sid in range(H):         # one hypothesis = one batch of N fits, like the reference's loop (the mean's divisor is N * k * 2)
        x0k = np.broadcast_to(x0c[sid][None, KEYLIST, :], (N, len(KEYLIST), 3))
        R, T, _, _, _ = O.ipo_fit(x0k, T0, K, uv[:, KEYLIST, :], "z", MIN_T, 2.0, 500)
        cs.append(np.stack([R[:, 0, 0], R[:, 1, 0]], -1))
        Ts.append(T[:, 0, :])
    s = ips.summary(np.stack(cs), np.stack(Ts), x0c[:, None], uv, K, KEYLIST, IPO_T)
    print(f"  {tag} oracle ipo ensemble: member {run} in {time.time() - t0:.0f} s", flush=True)
    return draw, run, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=12)
    ap.add_argument("--workers", type=int, default=6)
    ap.add_argument("--draws", default="a,b,c")
    a = ap.parse_args()
    from multiprocessing import Pool
    from _shared import Capture
    draws = a.draws.split(",")
    tasks = [(dr, r) for dr in draws for r in range(1, a.members + 1)]
    with Pool(a.workers) as pool:
        res = pool.map(member, tasks, chunksize=1)
    for dr in draws:
        tag = DRAWS[dr]
        sha = str(Capture(tag).g["inputs_sha"])             # Capture regenerates the inputs and checks them against it
        rows = [s for (q, r, s) in sorted((x for x in res if x[0] == dr), key=lambda x: x[1])]
        np.savez_compressed(os.path.join(OUT, tag + "_ipoens_oracle.npz"), members=np.arange(1, len(rows) + 1) + SEED0,
                            inputs_sha=np.array(sha), implementation=np.array("oracle/zedo_oracle.py::ipo_fit (numpy float32)"),
                            **{k: np.stack([np.asarray(r[k]) for r in rows]) for k in rows[0]})
        print("wrote", tag + "_ipoens_oracle.npz", len(rows), "members")


if __name__ == "__main__":
    main()
