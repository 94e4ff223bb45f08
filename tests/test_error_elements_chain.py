"""getErrorElements at the whole-chain boundary (pmx_icp_error_elements*), the
part that needs no GPU: the chain library loads without one, a fresh ICP has
zero columns and no error (the reference's default-constructed
lastErrorElements), and bad arguments return PMX_ICP_INVALID_PARAMETER.
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
from helpers import chain_yaml  # noqa: E402
from libpointmatcher_amd.icp import ICP, ICPSequence, IcpElementsInfo  # noqa: E402

INVALID_PARAMETER = -3  # PMX_ICP_INVALID_PARAMETER (include/pmx_icp.h)


def test_fresh_icp_has_no_columns_and_no_error():
    for cls in (ICP, ICPSequence):
        for dtype in (np.float32, np.float64):
            icp = cls(dtype)
            icp.load_yaml(chain_yaml())
            info = IcpElementsInfo()
            assert icp._l.pmx_icp_error_elements_info(icp.h, C.byref(info)) == 0
            assert (info.columns, info.rejected_matches, info.rejected_points) == (0, 0, 0)
            assert (info.reading_desc_dim, info.reference_desc_dim) == (0, 0)
            e = icp.error_elements()
            assert e.columns == 0 and e.reading.shape[0] == 0 and e.ids.dtype == np.int32
            assert e.descriptor("reading", "normals") is None and e.descriptor("reference", "normals") is None
            icp.close()


def test_bad_arguments():
    icp = ICP(np.float32)
    icp.load_yaml(chain_yaml())
    l, h = icp._l, icp.h
    info = IcpElementsInfo()
    span = C.c_int(7)
    buf = np.zeros(4, np.float32)
    p = buf.ctypes.data_as(C.c_void_p)
    assert l.pmx_icp_error_elements_info(None, C.byref(info)) == INVALID_PARAMETER
    assert l.pmx_icp_error_elements_info(h, None) == INVALID_PARAMETER
    assert l.pmx_icp_error_elements(None, 0, None, None, None, None, None, None) == INVALID_PARAMETER
    assert l.pmx_icp_error_elements(h, -1, None, None, p, None, None, None) == INVALID_PARAMETER  # short capacity
    assert b"capacity" in l.pmx_icp_last_error(h)
    assert l.pmx_icp_error_elements(h, 0, None, None, None, None, None, None) == 0  # every pointer may be NULL
    assert l.pmx_icp_error_elements_descriptor(None, 0, b"normals", None, 0, C.byref(span)) == INVALID_PARAMETER
    assert l.pmx_icp_error_elements_descriptor(h, 0, None, None, 0, C.byref(span)) == INVALID_PARAMETER
    assert l.pmx_icp_error_elements_descriptor(h, 0, b"normals", None, 0, None) == INVALID_PARAMETER
    assert l.pmx_icp_error_elements_descriptor(h, 2, b"normals", None, 0, C.byref(span)) == INVALID_PARAMETER
    assert l.pmx_icp_error_elements_descriptor(h, 1, b"normals", p, 4, C.byref(span)) == 0 and span.value == 0
    icp.close()
