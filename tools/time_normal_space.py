"""Time pmx_normal_space (NormalSpaceDataPointsFilter on the GPU) on the
benchmark's 1M-point float cloud with SurfaceNormalDataPointsFilter's normals,
nbSample 5000, epsilon pi / 32: wall time of the whole synchronous call
(upload, keys, host shuffle, sort, host picks, gather, download) after one
warm-up call, and beside it the host phases alone and the literal host program
of tests/normal_space_main.cpp on the same normals, both built -O2 here.
Prints one JSON line.

    python tools/time_normal_space.py [--n 1000000] [--nb-sample 5000] [--repeat 5]
"""
import argparse
import json
import math
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import normal_space_cases as nc  # noqa: E402
from libpointmatcher_amd import _capi  # noqa: E402
from libpointmatcher_amd.synth import reference_cloud  # noqa: E402


def phases(text):
    w = text.split()
    return {w[i]: float(w[i + 1]) for i in range(0, len(w), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nb-sample", type=int, default=5000)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    eps = math.pi / 32
    pts, _ = reference_cloud(a.n, np.float32)
    nrm = np.ascontiguousarray(_capi.surface_normals(pts, knn=8)["normals"])
    _capi.normal_space(pts[:1000], nrm[:1000], 0, 10, 1, eps)  # warm-up: module load
    ms, rechecked = [], 0
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        f, _, rechecked = _capi.normal_space(pts, nrm, 0, a.nb_sample, 1, eps)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert len(f) == a.nb_sample
    with tempfile.TemporaryDirectory() as tmp:
        prog = nc.Programs(tmp, sanitize=False)
        args = (a.nb_sample, 1, 1, nc.eps_bits(eps))
        shared = [phases(prog.run("shared", "time", nrm, *args)) for _ in range(a.repeat)]
        literal = [phases(prog.run("literal", "time", nrm, *args)) for _ in range(a.repeat)]
    med = lambda rows, k: float(np.median([r[k] for r in rows]))  # noqa: E731
    print(json.dumps({"n": a.n, "nb_sample": a.nb_sample, "epsilon": eps, "rechecked": rechecked,
                      "call_ms_median": float(np.median(ms)), "call_ms_min": float(min(ms)), "call_ms_all": ms,
                      "host_shuffle_ms": med(shared, "shuffle_ms"), "host_pick_ms": med(shared, "pick_ms"),
                      "host_replay_ms": med(shared, "replay_ms"),
                      "literal_total_ms": med(literal, "total_ms"), "literal_shuffle_ms": med(literal, "shuffle_ms"),
                      "literal_fill_ms": med(literal, "fill_ms"), "literal_pick_ms": med(literal, "pick_ms"),
                      "literal_swap_ms": med(literal, "swap_ms")}), flush=True)


if __name__ == "__main__":
    main()
