"""PointToPointSimilarityErrorMinimizer in the host chain, without a GPU: the
registry creates it from the reference's own similarity chain
(examples/data/icp_data/defaultSimilarityPointToPointMinDistDataPointsFilter.yaml,
copied under tests/golden/data) and from the shape of examples/data/icp_scale.yaml,
it takes no parameter (ADD_TO_REGISTRAR_NO_PARAM: a given one is rejected as
the registry rejects unused parameters), PointToPointErrorMinimizer chains load
and behave as before, and the libraries carry the new entry point.
"""
import os

import numpy as np
import pytest

from helpers import chain_yaml

SIM = "PointToPointSimilarityErrorMinimizer"
P2P = "PointToPointErrorMinimizer"
HERE = os.path.dirname(os.path.abspath(__file__))
YAML = os.path.join(HERE, "golden", "data", "defaultSimilarityPointToPointMinDistDataPointsFilter.yaml")

# the modules of examples/data/icp_scale.yaml (inspector and logger stand-ins included)
ICP_SCALE = """
readingDataPointsFilters:
  - RandomSamplingDataPointsFilter:
      prob: 0.5
referenceDataPointsFilters:
  - SamplingSurfaceNormalDataPointsFilter:
      knn: 10
matcher:
  KDTreeMatcher:
    knn: 3
    epsilon: 0
outlierFilters:
  - TrimmedDistOutlierFilter:
      ratio: 0.95
errorMinimizer:
  PointToPointSimilarityErrorMinimizer
transformationCheckers:
  - CounterTransformationChecker:
      maxIterationCount: 80
  - DifferentialTransformationChecker:
      minDiffRotErr: 0.08
      minDiffTransErr: 0.01
      smoothLength: 4
inspector:
 VTKFileInspector:
     baseFileName: pointmatcher-run1
     dumpIterationInfo: 1
logger:
  FileLogger
"""


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_reference_similarity_yaml_loads(dtype):
    from libpointmatcher_amd.icp import ICP
    icp = ICP(dtype)
    with open(YAML) as f:
        text = f.read()
    assert SIM in text and "epsilon: 3.16" in text
    icp.load_yaml(text)
    icp.load_yaml(ICP_SCALE)
    icp.load_yaml(chain_yaml(minimizer=SIM))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_minimizer_given_a_parameter_is_rejected(dtype):
    from libpointmatcher_amd import icp as I
    icp = I.ICP(dtype)
    # the same rejection as PointToPointErrorMinimizer's, registered the same way
    errs = []
    for name in (P2P, SIM):
        with pytest.raises(I.InvalidParameter) as e:
            icp.load_yaml(chain_yaml(minimizer=name + ":\n    sensorStdDev: 0.01\n"))
        errs.append(str(e.value))
        assert "sensorStdDev" in errs[-1]
    assert errs[1] == errs[0].replace(P2P, SIM)
    with pytest.raises(I.InvalidParameter, match="force2D"):
        icp.load_yaml(chain_yaml(minimizer=SIM + ":\n    force2D: 0\n"))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_point_to_point_chains_unaffected(dtype):
    from libpointmatcher_amd import icp as I
    icp = I.ICP(dtype)
    icp.load_yaml(chain_yaml(minimizer=P2P))
    with pytest.raises(I.InvalidParameter, match="force2D"):
        icp.load_yaml(chain_yaml(minimizer=P2P + ":\n    force2D: 0\n"))
    # the other unbuilt registry entries stay unknown
    for name in ("PointToPointWithCovErrorMinimizer", "IdentityErrorMinimizer"):
        with pytest.raises(I.InvalidElement, match=name):
            icp.load_yaml(chain_yaml(minimizer=name))


def test_libraries_and_bindings_carry_the_entry_point():
    from libpointmatcher_amd import _capi
    assert hasattr(_capi.lib(), "pmx_p2point_similarity_system")
    assert "pmx_p2point_similarity_system" in _capi.EXPORTS
    assert callable(_capi.Context.p2point_similarity_system)
    # pmx_p2point_system keeps its signature
    assert len(_capi.lib().pmx_p2point_system.argtypes) == 5
