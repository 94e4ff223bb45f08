"""The quantile select's test reference (helpers.quantile_limit, a plain
numpy sort) against the CPU oracle's nth_element chain, bit for bit, on every
adversarial key set tests/test_gpu_select_edges.py feeds the GPU — and the
stated property of each key set, so that a recipe that drifts is caught here,
without a GPU.
"""
import numpy as np
import pytest

from helpers import (MEDIAN, SELECT_KEY_SETS, SELECT_SIZES, TRIMMED, filter_params, key_bits, matched_dists,
                     max_dist_keeping, quantile_limit, quantile_rank, select_filters, select_reading_x)

DTYPES = [np.float32, np.float64]


def check_against_oracle(oracle, d, dtype, filters):
    for kind, p in filters:
        rc, ow = oracle.outlier_chain([(kind, filter_params(kind, p))], d)
        assert rc == 0
        limit, w = quantile_limit(d, kind, p, dtype)
        assert w.dtype == d.dtype and w.shape == d.shape
        assert np.array_equal(w, ow), (kind, p)
        assert np.isfinite(limit)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3000, 20_000])
@pytest.mark.parametrize("tag", SELECT_KEY_SETS)
def test_reference_equals_oracle_on_key_sets(oracle, tag, n, dtype):
    d = matched_dists(select_reading_x(tag, n, dtype))
    check_against_oracle(oracle, d, dtype, select_filters(dtype) + [(TRIMMED, 0.80)])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SELECT_SIZES)
@pytest.mark.parametrize("tag", ["lastdigit", "decades"])
def test_reference_equals_oracle_on_sizes(oracle, tag, n, dtype):
    d = matched_dists(select_reading_x(tag, n, dtype))
    check_against_oracle(oracle, d, dtype, select_filters(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_equals_oracle_k3(oracle, dtype):
    # k = 3 against the reference points x = 0, -1, -2: n = 3 * 1367 = 4101
    x = select_reading_x("decades", 1367, dtype)
    d = np.stack([x * x, (x + 1) * (x + 1), (x + 2) * (x + 2)], 1).astype(dtype)
    assert d.size == 4101 and d.size % 16 != 0
    check_against_oracle(oracle, d, dtype, select_filters(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
def test_reference_chain_position_one(oracle, dtype):
    # MaxDist then Trimmed: the second quantile still runs over every finite distance
    for tag, cut, ratio in (("two_values", 0.125, 0.85), ("decades", 1e-7, 0.3)):
        d = matched_dists(select_reading_x(tag, 3000, dtype))
        rc, ow = oracle.outlier_chain([("MaxDistOutlierFilter", {"maxDist": cut}),
                                       (TRIMMED, {"ratio": ratio})], d)
        assert rc == 0
        T = np.dtype(dtype).type
        w = (d <= T(np.power(float(T(cut)), 2.0))).astype(dtype) * quantile_limit(d, TRIMMED, ratio, dtype)[1]
        assert np.array_equal(w, ow)
        assert 0 < w.sum() < d.size


def test_reference_nothing_finite():
    with pytest.raises(LookupError):
        quantile_limit(np.full((5, 1), np.inf, np.float32), TRIMMED, 0.85, np.float32)


# ---- the stated property of each key set ----
@pytest.mark.parametrize("dtype", DTYPES)
def test_lastdigit_keys_share_all_but_the_last_digits(dtype):
    k = key_bits(matched_dists(select_reading_x("lastdigit", 3000, dtype)))
    assert len(np.unique(k)) == 3000
    if dtype is np.float32:
        assert (int(k.min()), int(k.max())) == (0x3F800000, 0x3F80176F)
        assert len(np.unique(k >> 21)) == 1 and len(np.unique(k >> 10)) == 6
    else:
        assert int(k.min()) == 0x3FF0000000000000
        assert len(np.unique(k >> np.uint64(20))) == 1  # the first four passes carry one prefix
        assert len(np.unique(k >> np.uint64(10))) == 6  # six buckets of the top 54 bits
    # extended to the largest size the keys stay distinct and ordered
    kk = key_bits(matched_dists(select_reading_x("lastdigit", SELECT_SIZES[-1], dtype)))
    assert np.all(np.diff(kk.astype(np.int64)) > 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3000, 20_000])
def test_equal_and_zero_keys(dtype, n):
    d = matched_dists(select_reading_x("equal", n, dtype))
    assert np.all(d == 0.25)
    z = key_bits(matched_dists(select_reading_x("zero", n, dtype)))
    assert np.all(z == 0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3000, 20_000])
def test_two_values_tie_positions(dtype, n):
    d = matched_dists(select_reading_x("two_values", n, dtype))
    s = np.sort(d.ravel())
    low = n * 4 // 5
    assert np.all(s[:low] == 2.0 ** -8) and np.all(s[low:] == 2.0 ** -4)
    # Trimmed 0.80: the rank computed in T is the first key of the upper tie
    r80 = quantile_rank(n, TRIMMED, 0.80, dtype)
    assert r80 == low and s[r80 - 1] < s[r80]
    # Trimmed 0.85: inside the upper tie, thousands of equal keys either side
    r85 = quantile_rank(n, TRIMMED, 0.85, dtype)
    assert low + n // 25 <= r85 < n - n // 25 and s[r85 - 1] == s[r85] == s[r85 + 1]
    assert quantile_limit(d, TRIMMED, 0.80, dtype)[0] == quantile_limit(d, TRIMMED, 0.85, dtype)[0] == 2.0 ** -4
    # Median: inside the lower tie
    assert s[quantile_rank(n, MEDIAN, 3.0, dtype)] == 2.0 ** -8


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3000, 20_000])
def test_decades_keys(dtype, n):
    d = matched_dists(select_reading_x("decades", n, dtype))
    assert np.all(np.isfinite(d)) and np.all(d > 0)
    k = key_bits(d)
    assert len(np.unique(k)) == n
    if dtype is np.float32:
        # 42 decades of d = 140 binades, four values of the top digit each
        top = len(np.unique(k >> 21))
        assert 555 <= top <= 562, top
        assert np.all(d >= np.finfo(np.float32).tiny)  # no subnormal


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [3000, 20_000])
def test_mostly_inf_counts(oracle, dtype, n):
    x = select_reading_x("decades", n, dtype)
    for m in (1, 2, n // 100, n // 100 + 1):
        d = matched_dists(x, max_dist_keeping(x, m))
        fin = d[d != np.inf]
        assert fin.size == m and np.array_equal(np.sort(fin), np.sort((x * x))[:m])
        assert quantile_rank(m, TRIMMED, 1e-6, dtype) == 0
        assert quantile_rank(m, MEDIAN, 3.0, dtype) == m // 2
        check_against_oracle(oracle, d, dtype, select_filters(dtype))
    assert (n // 100) % 2 == 0  # (an even and an odd count beside 1 and 2)
