"""pmx_loop_error_elements_prepare: the columns of a stopped device loop's last
match equal the module path's at the same match, and the restatement
(error_elements_cases.restate) on that match's mirrors.  Exact comparisons.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import error_elements_cases as E  # noqa: E402
import quality_cases as Q  # noqa: E402

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", [Q.PLANE, Q.POINT])
def test_device_loop_equals_module_path(dtype, kind):
    from libpointmatcher_amd import _capi
    rd, ref, nrm = Q.clouds(1000, dtype)
    ctx = _capi.Context(0, dtype)
    ctx.set_reference(ref, nrm)
    ctx.set_reading(rd)
    info = _capi.ElementsInfo()
    assert ctx._l.pmx_loop_error_elements_prepare(ctx.h, C.byref(info)) == _capi.PMX_E_STATE  # no loop yet
    ctx.loop_begin(filters=[("TrimmedDistOutlierFilter", 0.85)], minimizer=kind,
                   checkers=[("CounterTransformationChecker", 4)], keep_trace=True)
    st = ctx.loop_run(10)
    assert st.done and st.iterations == 4
    loop = ctx.loop_error_elements()
    assert loop.columns == st.last.kept
    assert (loop.rejected_matches, loop.rejected_points) == (st.last.rejected_matches, st.last.rejected_points)
    tr = ctx.loop_trace(0, 4)
    # the module path: the fourth iteration's match ran at the third's transform
    ctx.set_reading(rd)
    ctx.match(tr[2], knn=1)
    ctx.outlier("TrimmedDistOutlierFilter", 0, ratio=0.85)
    mod = ctx.error_elements()
    d, ids = ctx.get_matches()
    want = E.restate(d, ids, ctx.get_weights(), E.step_reading(tr[2], rd), ref, nrm)
    ctx.close()
    assert 0 < len(want["dists"]) < d.size
    E.assert_equal(mod, want, "module")
    E.assert_equal(loop, want, "loop")
