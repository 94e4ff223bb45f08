"""SurfaceNormalOutlierFilter in the host chain, without a GPU: the registry
creates it from a YAML chain, its parameter keeps the reference's bounds
(OutlierFiltersImpl.h:182-187: maxAngle, default 1.57, range 0.0 to 3.1416)
and the C ABI and its Python binding carry the new entry points.  (That the
default is 1.57 is checked where the filter runs, test_gpu_surface_normal_filter.py.)
"""
import numpy as np
import pytest

from helpers import chain_yaml

SN = "SurfaceNormalOutlierFilter"


def test_yaml_chain_with_the_filter_loads():
    from libpointmatcher_amd.icp import ICP
    icp = ICP(np.float32)
    icp.load_yaml(chain_yaml(filters=[("TrimmedDistOutlierFilter", {"ratio": 0.85}), (SN, {"maxAngle": 0.6})]))
    # without parameters (the default), alone, twice, and in double
    icp.load_yaml(chain_yaml(filters=[(SN, {})]))
    icp.load_yaml(chain_yaml(filters=[(SN, {"maxAngle": 0.0}), (SN, {"maxAngle": 3.1416})],
                             minimizer="PointToPointErrorMinimizer"))
    ICP(np.float64).load_yaml(chain_yaml(filters=[(SN, {"maxAngle": 1.57})]))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_max_angle_bounds(dtype):
    from libpointmatcher_amd import icp as I
    icp = I.ICP(dtype)
    with pytest.raises(I.InvalidParameter, match="maxAngle.*larger than maximum"):
        icp.load_yaml(chain_yaml(filters=[(SN, {"maxAngle": 4})]))
    with pytest.raises(I.InvalidParameter, match="maxAngle.*smaller than minimum"):
        icp.load_yaml(chain_yaml(filters=[(SN, {"maxAngle": -0.1})]))
    with pytest.raises(I.InvalidParameter, match="maxAngel"):
        icp.load_yaml(chain_yaml(filters=[(SN, {"maxAngel": 1.0})]))


def test_binding_carries_the_entry_points():
    from libpointmatcher_amd import _capi
    l = _capi.lib()
    assert hasattr(l, "pmx_set_reading_normals") and hasattr(l, "pmx_outlier_surface_normal")
    assert _capi.FILTER_KIND[SN] == 8
    assert callable(_capi.Context.set_reading_normals) and callable(_capi.Context.outlier_surface_normal)
