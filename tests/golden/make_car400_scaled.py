"""Generate the fixtures of the similarity ICP's known answer from the
reference's own test data (utest/utest.cpp:222-243).

Run once, with the reference's examples/data directory:
    python tests/golden/make_car400_scaled.py <reference>/examples/data
Outputs (data only) go to tests/golden/:
  - car400_scaled.npz: xyz of examples/data/car_cloud400_scaled.csv as a
      float32 (n, 3) array under the key "car400_scaled" (car_cloud400 itself
      is "car400" of clouds.npz);
  - data/defaultSimilarityPointToPointMinDistDataPointsFilter.yaml: the chain
      configuration the reference's test loads, as it is.
"""
import os
import shutil
import sys

import numpy as np

REF = sys.argv[1] if len(sys.argv) > 1 else "examples/data"
OUT = os.path.dirname(os.path.abspath(__file__))
YAML = "defaultSimilarityPointToPointMinDistDataPointsFilter.yaml"


def main():
    with open(os.path.join(REF, "car_cloud400_scaled.csv")) as f:
        header = [h.strip() for h in f.readline().split(",")]
        assert header[:3] == ["x", "y", "z"], header
        a = np.array([[float(x) for x in line.split(",")[:3]] for line in f if line.strip()], dtype=np.float64)
    np.savez_compressed(os.path.join(OUT, "car400_scaled.npz"), car400_scaled=a.astype(np.float32))
    shutil.copyfile(os.path.join(REF, "icp_data", YAML), os.path.join(OUT, "data", YAML))
    print(f"car400_scaled: {a.shape}")


if __name__ == "__main__":
    main()
