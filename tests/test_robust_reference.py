"""The oracle's RobustOutlierFilter (oracle/pmo_impl.inc pmo_robust_weights) held
to the cases, the independent reference and the bars of tests/robust_cases.py,
without a GPU: thresholds met exactly, d == 0, float and double underflow and
the 1e-50 clamp, degenerate scales, median ties and the point-to-plane distance
at invalid entries.  tests/test_gpu_robust_edges.py holds the device to the
same cases and bars; the cases must be ones the oracle passes.
"""
import numpy as np
import pytest

import robust_cases as rc

CASES = rc.case_ids()


@pytest.mark.parametrize("group,name,dtype", CASES, ids=[f"{n}-{np.dtype(t).name}" for _, n, t in CASES])
def test_oracle_on_edge_case(oracle, group, name, dtype):
    case = rc.get_case(group, name, dtype)
    for k in case.ks:
        sc = rc.scene(case, dtype, k)
        exp = rc.expected(case, dtype, k)
        r = oracle.make_robust(case.params())
        if case.raises:
            assert exp is None and not np.isfinite(sc.d).any()
            code, _ = oracle.robust_weights(r, sc.d, sc.ids, step=sc.rd, ref=sc.ref, normals=sc.nrm)
            assert code == oracle.E_EMPTY_QUANTILE
            continue
        assert exp is not None
        print(f"{name} {np.dtype(dtype).name} k={k}: bands {rc.check_bands(case, exp)}")
        for call, x in enumerate(exp):
            code, w = oracle.robust_weights(r, sc.d, sc.ids, step=sc.rd, ref=sc.ref, normals=sc.nrm)
            assert code == 0
            print(f"  call {call + 1}: scale {x.scale!r}, {rc.band_counts(x)}")
            rc.check_call(case, x, r.scale, w, "oracle")
            assert r.iteration == call + 2


def test_scene_is_exact():
    """the scene's own claims: 10-bit offsets, their neighbours, a centred lattice"""
    assert rc.neighbours(0.5) == (1023 / 2048, 513 / 1024)
    assert rc.neighbours(0.75) == (767 / 1024, 769 / 1024)
    assert rc.ten_bits(1023 / 2048) and not rc.ten_bits(1025 / 2048) and not rc.ten_bits(2.0 ** -19)
    for dtype in (np.float32, np.float64):
        ref = rc.lattice(dtype)
        assert ref.shape == (rc.M, 4) and np.all(ref[:, :3].mean(0) == 0)
        assert np.abs(ref[:, :3]).max() == 60 and np.abs(ref[:, :3]).min() == 4
