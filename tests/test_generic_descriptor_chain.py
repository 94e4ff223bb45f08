"""GenericDescriptorOutlierFilter in the host chain (csrc/host/pm_icp.cpp
GenericDescriptorOF; the reference: OutlierFiltersImpl.h:196-221,
OutlierFiltersImpl.cpp:290-374).

Without a GPU: a YAML chain naming the filter loads, its parameters are
bounded as the reference's, and the three exceptions of the reference arise
(a bad `source`, a missing descriptor, a descriptor with more than one row),
before the device is touched.  Before the filter existed every one of these
failed with InvalidElement at load_yaml.
With a GPU: `source: reading` reads the filtered reference as `source:
reference` does (the reference's own behaviour, :322-325); the device loop
and the per-module path agree for hard and soft chains under the criterion of
tests/test_gpu_loop.py; ICPSequence reads the descriptor staged for its map.
"""
import numpy as np
import pytest

from helpers import chain_yaml
from libpointmatcher_amd import _capi
from libpointmatcher_amd.icp import (ICP, ConfigurationError, ICPSequence, InvalidElement, InvalidField,
                                     InvalidParameter, outlier_filter_doc)
from libpointmatcher_amd.synth import reading_cloud, reference_cloud

NAME = "GenericDescriptorOutlierFilter"
N, M = 3000, 4000
TOL = {np.float32: 1e-5, np.float64: 1e-12}  # (README, Parity: the transform tolerances)
ITERS = 8


def gd(**p):
    return (NAME, dict({"descName": "quality"}, **p))


def yaml_of(*filters, minimizer="PointToPlaneErrorMinimizer", maxit=ITERS):
    return chain_yaml(filters=filters, minimizer=minimizer, maxit=maxit)


def quality(dtype, m=M):
    rng = np.random.default_rng(11)
    v = rng.uniform(0.05, 1.0, m).astype(dtype)
    v[rng.choice(m, 50, replace=False)] = dtype(0.5)
    return v


def have_gpu():
    try:
        return _capi.lib().pmx_device_count() > 0
    except Exception:
        return False


# ------------------------------------------------------------ without a GPU --
def test_yaml_chain_with_the_filter_loads():
    icp = ICP(np.float32)
    icp.load_yaml(yaml_of(gd()))
    icp.load_yaml(yaml_of(("TrimmedDistOutlierFilter", {"ratio": 0.8}),
                          gd(source="reading", useSoftThreshold=1, useLargerThan=0, threshold=0.25)))
    icp.close()


# what the reference prints for the filter's parameters (Parametrizable.cpp:51-74 over
# OutlierFiltersImpl.h:202-211): names, defaults, doc strings and bounds
REFERENCE_DOC = (
    "- source (default: reference) - Point cloud from which the descriptor will be used: reference or reading\n"
    "- descName (default: none) - Descriptor name used to weight paired points\n"
    "- useSoftThreshold (default: 0) - If set to 1 (true), uses the value of the descriptor as a weight. If set to 0 "
    "(false), uses the parameter 'threshold' to set binary weights. - min: 0 - max: 1\n"
    "- useLargerThan (default: 1) - If set to 1 (true), values over the 'threshold' will have a weight of one.  If "
    "set to 0 (false), values under the 'threshold' will have a weight of one. All other values will have a weight "
    "of zero. - min: 0 - max: 1\n"
    "- threshold (default: 0.1) - Value used to determine the binary weights - min: 0.0000001 - max: inf\n")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_parameters_print_as_the_references(dtype):
    assert outlier_filter_doc(NAME, dtype) == REFERENCE_DOC
    with pytest.raises(InvalidElement):
        outlier_filter_doc("NoSuchOutlierFilter", dtype)


def test_source_must_be_reference_or_reading():
    icp = ICP(np.float32)
    with pytest.raises(InvalidParameter) as e:
        icp.load_yaml(yaml_of(gd(source="map")))
    assert str(e.value) == ("GenericDescriptorOutlierFilter: Error, the parameter named 'source' can only be set to "
                            "'reference' or 'reading' but was set to map")
    icp.close()


@pytest.mark.parametrize("bad", [{"threshold": 0}, {"useSoftThreshold": 2}, {"useLargerThan": -1}])
def test_parameter_bounds_are_the_references(bad):
    icp = ICP(np.float32)
    with pytest.raises(InvalidParameter):
        icp.load_yaml(yaml_of(gd(**bad)))
    icp.close()


def test_missing_descriptor_is_invalid_field():
    ref, nrm = reference_cloud(M, np.float32)
    icp = ICP(np.float32)
    icp.load_yaml(yaml_of(gd()))
    with pytest.raises(InvalidField, match="quality"):
        icp.compute(reading_cloud(N, np.float32), ref, nrm)
    icp.close()


def test_descriptor_with_two_rows_is_invalid_parameter():
    ref, nrm = reference_cloud(M, np.float32)
    icp = ICP(np.float32)
    icp.load_yaml(yaml_of(gd()))
    icp.add_descriptor("reference", "quality", np.ones((M, 2), np.float32))
    with pytest.raises(InvalidParameter) as e:
        icp.compute(reading_cloud(N, np.float32), ref, nrm)
    assert str(e.value) == ("GenericDescriptorOutlierFilter: Error, the parameter named 'descName' must be a 1D "
                            "descriptor but the field quality is 2D")
    icp.close()


def test_a_second_filter_is_a_configuration_error():
    ref, nrm = reference_cloud(M, np.float32)
    icp = ICP(np.float32)
    icp.load_yaml(yaml_of(gd(), gd(useSoftThreshold=1)))
    icp.add_descriptor("reference", "quality", quality(np.float32))
    with pytest.raises(ConfigurationError, match="at most one GenericDescriptorOutlierFilter"):
        icp.compute(reading_cloud(N, np.float32), ref, nrm)
    icp.close()


def test_the_chain_runs_on_the_gpu_or_fails_loudly():
    """With a valid descriptor the host checks pass and the chain needs the
    device: without one it raises what every chain raises there (the context
    cannot be created), never a CPU result."""
    ref, nrm = reference_cloud(M, np.float32)
    icp = ICP(np.float32)
    icp.load_yaml(yaml_of(gd(threshold=0.5)))
    icp.add_descriptor("reference", "quality", quality(np.float32))
    if have_gpu():
        icp.compute(reading_cloud(N, np.float32), ref, nrm)
        assert 0 < icp.stats().kept < N
    else:
        with pytest.raises(RuntimeError, match=r"pmx_ctx_create failed \(-13\): no usable HIP device"):
            icp.compute(reading_cloud(N, np.float32), ref, nrm)
    icp.close()


# --------------------------------------------------------------- with a GPU --
def run(monkeypatch, mode, text, dtype, desc):
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1" if mode == "loop" else "0")
    ref, nrm = reference_cloud(M, dtype)
    icp = ICP(dtype)
    icp.load_yaml(text)
    icp.keep_trace(True)
    icp.add_descriptor("reference", "quality", desc)
    T = icp.compute(reading_cloud(N, dtype), ref, nrm)
    st, tr = icp.stats(), icp.trace()
    icp.close()
    return T, st, tr


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("minimizer", ["PointToPlaneErrorMinimizer", "PointToPointErrorMinimizer"])
@pytest.mark.parametrize("soft", [0, 1])
def test_device_loop_equals_modules(monkeypatch, dtype, minimizer, soft):
    text = yaml_of(("TrimmedDistOutlierFilter", {"ratio": 0.8}), gd(useSoftThreshold=soft, threshold=0.5),
                   minimizer=minimizer)
    desc = quality(dtype)
    Tl, sl, trl = run(monkeypatch, "loop", text, dtype, desc)
    Tm, sm, trm = run(monkeypatch, "modules", text, dtype, desc)
    print(f"{np.dtype(dtype).name} {minimizer} soft={soft}: |Tl - Tm| {np.linalg.norm(Tl - Tm):.3g} kept {sl.kept}")
    assert sl.iterations == sm.iterations == ITERS
    assert len(trl) == len(trm) == ITERS
    assert np.linalg.norm(Tl - Tm) <= TOL[dtype]
    assert np.abs(trl - trm).max() <= 10 * TOL[dtype]
    assert sl.kept == sm.kept and sl.rejected_matches == sm.rejected_matches
    # the filter acts: the chain without it keeps more pairs
    T0, s0, _ = run(monkeypatch, "modules", yaml_of(("TrimmedDistOutlierFilter", {"ratio": 0.8}),
                                                    minimizer=minimizer), dtype, desc)
    assert (sm.kept < s0.kept) if not soft else (np.linalg.norm(T0 - Tm) > 0)


@pytest.mark.gpu
def test_source_reading_reads_the_reference(monkeypatch):
    dtype = np.float32
    desc = quality(dtype)
    a = run(monkeypatch, "modules", yaml_of(gd(source="reference", threshold=0.5)), dtype, desc)
    b = run(monkeypatch, "modules", yaml_of(gd(source="reading", threshold=0.5)), dtype, desc)
    assert np.array_equal(a[0], b[0]) and a[1].kept == b[1].kept


@pytest.mark.gpu
def test_icp_sequence_reads_the_maps_descriptor(monkeypatch):
    dtype = np.float32
    monkeypatch.setenv("PMX_DEVICE_LOOP", "1")
    ref, nrm = reference_cloud(M, dtype)
    rd = reading_cloud(N, dtype)
    desc = quality(dtype)
    text = yaml_of(gd(threshold=0.5))
    one, st, _ = run(monkeypatch, "loop", text, dtype, desc)
    seq = ICPSequence(dtype)
    seq.load_yaml(text)
    seq.add_descriptor("reference", "quality", desc)
    assert seq.set_map(ref, nrm)
    T1 = seq.compute(rd)
    T2 = seq.compute(rd)  # (the map and its descriptor stay resident)
    s = seq.stats()
    seq.close()
    assert np.array_equal(T1, T2) and s.kept == st.kept
    assert np.linalg.norm(T1 - one) <= 1e-5
