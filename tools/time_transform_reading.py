"""Time Context.transform_reading (pmx_transform_reading: one kernel over the
resident reading, one download, no upload) at 1M float 3-D points, beside
_capi.transform_cloud on the same array (upload, kernel, download: DESIGN.md
section 5s's call).  A host clock around each call, which ends in a stream
synchronise, after one warm-up call of each; the two calls alternate.  Prints
one JSON line.

    python tools/time_transform_reading.py [--n 1000000] [--repeat 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libpointmatcher_amd import _capi  # noqa: E402
from libpointmatcher_amd.synth import reading_cloud, reference_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--repeat", type=int, default=20)
    a = ap.parse_args()
    ref, nrm = reference_cloud(100000, np.float32)
    rd = reading_cloud(a.n, np.float32)
    T = np.eye(4, dtype=np.float32)
    c, s = np.cos(0.3), np.sin(0.3)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = [0.1, -0.2, 0.3]
    ctx = _capi.Context(0, np.float32)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    got = ctx.transform_reading(T)  # warm-up (and the staging buffer's allocation)
    want = _capi.transform_cloud(rd, T)[0]
    assert np.array_equal(got, want)
    resident, cloud = [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        ctx.transform_reading(T)
        t1 = time.perf_counter()
        _capi.transform_cloud(rd, T)
        t2 = time.perf_counter()
        resident.append((t1 - t0) * 1e3)
        cloud.append((t2 - t1) * 1e3)
    ctx.close()
    print(json.dumps({"n": a.n, "dtype": "float32", "repeat": a.repeat,
                      "transform_reading_ms_median": float(np.median(resident)),
                      "transform_reading_ms_min": float(min(resident)),
                      "transform_reading_ms_max": float(max(resident)),
                      "transform_cloud_ms_median": float(np.median(cloud)),
                      "transform_cloud_ms_min": float(min(cloud))}), flush=True)


if __name__ == "__main__":
    main()
