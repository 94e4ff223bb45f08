"""Time pmx_octree_grid (OctreeGridDataPointsFilter on the GPU) on the
benchmark's 1M-point float cloud, maxPointByNode 8, once per sampling method
after one warm-up call: device events around the whole call (upload, tree
walk, sampler, download) and the kept count.  Prints one JSON line per method.

    python tools/time_octree.py [--n 1000000] [--max-points 8] [--repeat 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from libpointmatcher_amd import _capi  # noqa: E402
from libpointmatcher_amd.synth import reference_cloud  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--max-points", type=int, default=8)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    pts, nrm = reference_cloud(a.n, np.float32)
    torch.cuda.init()
    _capi.octree_grid(pts[:1000], nrm[:1000], a.max_points, 0.0, 0)  # warm-up: module load
    for method in range(4):
        ms = []
        kept = 0
        for _ in range(a.repeat):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f, _ = _capi.octree_grid(pts, nrm, a.max_points, 0.0, method)
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
            kept = len(f)
        print(json.dumps({"method": method, "n": a.n, "max_point_by_node": a.max_points, "kept": kept,
                          "ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_all": ms}), flush=True)


if __name__ == "__main__":
    main()
