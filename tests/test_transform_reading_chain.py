"""The resident-reading transformation's entry points, as far as they go
without a GPU: the C ABI symbols in the built libraries, the Python bindings,
and the state error of ICP.reading_transformed before any compute (an ICP
object is built and loaded without touching a device).
"""
import ctypes
import os

import numpy as np
import pytest

from helpers import chain_yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [np.float32, np.float64]


def test_libraries_and_bindings_carry_the_entry_points():
    from libpointmatcher_amd import _capi
    _capi.lib()
    lib = os.path.join(ROOT, "libpointmatcher_amd", "lib")
    pmx = ctypes.CDLL(os.path.join(lib, "libpmx.so"))
    assert hasattr(pmx, "pmx_transform_reading") and hasattr(pmx, "pmx_transform_reading_offset")
    assert hasattr(ctypes.CDLL(os.path.join(lib, "libpmx_icp.so")), "pmx_icp_reading_transformed")
    assert "pmx_transform_reading" in _capi.EXPORTS and "pmx_transform_reading_offset" in _capi.EXPORTS
    assert callable(_capi.Context.transform_reading)


@pytest.mark.parametrize("dtype", DTYPES)
def test_reading_transformed_before_any_compute_is_a_state_error(dtype):
    from libpointmatcher_amd.icp import ICP, ICPSequence
    for cls in (ICP, ICPSequence):
        icp = cls(dtype)
        icp.load_yaml(chain_yaml())
        with pytest.raises(RuntimeError, match="no compute has run"):
            icp.reading_transformed()
        icp.close()


def test_null_handles_are_refused():
    from libpointmatcher_amd import _capi
    from libpointmatcher_amd import icp as I
    out = np.zeros((1, 4), np.float32)
    T = np.eye(4, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert _capi.lib().pmx_transform_reading(None, p(T), p(out), None) == _capi.PMX_E_BAD_PARAM
    n, rows = ctypes.c_int64(0), ctypes.c_int(0)
    assert I.lib().pmx_icp_reading_transformed(None, p(out), out.size, ctypes.byref(n), ctypes.byref(rows)) == -3
