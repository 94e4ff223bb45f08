"""Time pmx_covariance_sampling (CovarianceSamplingDataPointsFilter on the GPU)
on the benchmark's 1M-point float cloud with its analytic normals, nbSample
5000: wall time of the whole synchronous call (upload, centre, L, covariance,
host Jacobi, keys, six sorts, host picks, gather, download) after one warm-up
call, the median of --repeat calls per torque norm; and beside it, once, the
literal host program of tests/covariance_sampling_main.cpp built -O2 here, on
the first --literal-n points of the same cloud with the centre, L and basis the
library reports for them (torqueNorm 1).  Prints one JSON line.

    python tools/time_covariance_sampling.py [--n 1000000] [--nb-sample 5000] [--repeat 5] [--literal-n N]
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import covariance_sampling_cases as cc  # noqa: E402
from libpointmatcher_amd import _capi  # noqa: E402
from libpointmatcher_amd.synth import reference_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nb-sample", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--literal-n", type=int, default=0, help="points given to the literal program (0: all)")
    a = ap.parse_args()
    pts, nrm = reference_cloud(a.n, np.float32)
    _capi.covariance_sampling(pts[:1000], nrm[:1000], 0, 10, 1)  # warm-up: module load
    out = {"n": a.n, "nb_sample": a.nb_sample}
    for tn in cc.TORQUE_NORMS:
        ms, rep = [], None
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            f, _, rep = _capi.covariance_sampling(pts, nrm, 0, a.nb_sample, tn)
            ms.append((time.perf_counter() - t0) * 1e3)
            assert len(f) == a.nb_sample
        out[f"torque_norm_{tn}"] = {"call_ms_median": float(np.median(ms)), "call_ms_min": float(min(ms)),
                                    "call_ms_all": ms, "depth": rep["depth"]}
    ln = a.literal_n or a.n
    lp, lnrm = np.ascontiguousarray(pts[:ln]), np.ascontiguousarray(nrm[:ln])
    rep = _capi.covariance_sampling(lp, lnrm, 0, a.nb_sample, 1)[2]
    with tempfile.TemporaryDirectory() as tmp:
        prog = cc.Programs(tmp, sanitize=False)
        path = prog.write(lp, lnrm, rep["center"], rep["lnorm"], rep["eigvec"])
        text = subprocess.run([prog.exe["literal"], "time", "f", path, str(ln), str(a.nb_sample)],
                              capture_output=True, text=True, check=True).stdout.split()
    out["literal_n"] = ln
    out["literal"] = {text[i]: float(text[i + 1]) for i in range(0, len(text), 2)}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
