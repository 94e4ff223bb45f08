"""error_elements_cases.restate, the yardstick of the getErrorElements tests,
on cases whose answer is known without it: the reference's own known-answer
shape (utest/ui/ErrorMinimizers.cpp:49-106: 100 points, weights of one,
ids = i) and a k = 2 match written out by hand.  No GPU.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import error_elements_cases as E  # noqa: E402

INF = np.inf


def test_reference_known_answer_shape():
    n = 100
    rng = np.random.default_rng(0)
    rd = np.c_[rng.normal(0, 1, (n, 3)), np.ones(n)].astype(np.float32)
    ref = np.c_[rng.normal(0, 1, (n, 3)), np.ones(n)].astype(np.float32)
    d = np.ones((n, 1), np.float32)
    w = np.ones((n, 1), np.float32)
    ids = np.arange(n, dtype=np.int32)[:, None]
    e = E.restate(d, ids, w, rd, ref)
    assert e["reading"].shape == (100, 4) and e["reference"].shape == (100, 4)
    np.testing.assert_array_equal(e["reading"], rd)
    np.testing.assert_array_equal(e["reference"], ref)
    np.testing.assert_array_equal(e["ids"], np.arange(n))
    np.testing.assert_array_equal(e["reading_index"], np.arange(n))
    assert (e["link_rank"] == 0).all() and (e["weights"] == 1).all() and (e["dists"] == 1).all()
    assert (e["rejected_matches"], e["rejected_points"]) == (0, 0)


def test_hand_written_two_links():
    """Five reading points, k = 2: an inf entry, a zero weight, a negative
    weight and a point (3) with no kept link."""
    d = np.array([[0.1, 0.2], [0.3, INF], [0.4, 0.5], [INF, 0.6], [0.7, 0.8]], np.float32)
    w = np.array([[1.0, 0.0], [0.5, 1.0], [-0.25, 1.0], [1.0, 0.0], [0.0, 2.0]], np.float32)
    ids = np.array([[4, 3], [2, -1], [1, 0], [-1, 2], [0, 4]], np.int32)
    rd = np.c_[np.arange(5) * 10.0, np.arange(5) * 10.0 + 1, np.arange(5) * 10.0 + 2, np.ones(5)].astype(np.float32)
    ref = np.c_[np.arange(5) * 100.0, np.arange(5) * 100.0 + 1, np.arange(5) * 100.0 + 2, np.ones(5)].astype(np.float32)
    nrm = np.eye(3, dtype=np.float32)[[0, 1, 2, 0, 1]]
    e = E.restate(d, ids, w, rd, ref, nrm)
    # columns: (0,0) (1,0) (2,0) (2,1) (4,1); (1,1) has w != 0 but dist == inf
    np.testing.assert_array_equal(e["reading_index"], [0, 1, 2, 2, 4])
    np.testing.assert_array_equal(e["link_rank"], [0, 0, 0, 1, 1])
    np.testing.assert_array_equal(e["ids"], [4, 2, 1, 0, 4])
    np.testing.assert_array_equal(e["dists"], np.array([0.1, 0.3, 0.4, 0.5, 0.8], np.float32))
    np.testing.assert_array_equal(e["weights"], np.array([1.0, 0.5, -0.25, 1.0, 2.0], np.float32))
    np.testing.assert_array_equal(e["reading"][:, 0], [0, 10, 20, 20, 40])
    np.testing.assert_array_equal(e["reference"][:, 0], [400, 200, 100, 0, 400])
    np.testing.assert_array_equal(e["ref_normals"], nrm[[4, 2, 1, 0, 4]])
    # rejected matches: (0,1), (3,1), (4,0): finite with a zero weight; (3,0) is inf, not counted
    assert e["rejected_matches"] == 3
    assert e["rejected_points"] == 1  # point 3
    assert e["ids"].dtype == np.int32 and e["reading_index"].dtype == np.int32 and e["link_rank"].dtype == np.int32


def test_step_reading_embeds_two_dimensions():
    T = np.array([[0.8, -0.6, 1.5], [0.6, 0.8, -2.0], [0, 0, 1]], np.float32)
    rd = np.array([[1.0, 2.0, 1.0], [-3.0, 0.5, 1.0]], np.float32)
    got = E.step_reading(T, rd)
    want = np.stack([(T[0, 0] * rd[:, 0] + T[0, 1] * rd[:, 1]) + T[0, 2] * rd[:, 2],
                     (T[1, 0] * rd[:, 0] + T[1, 1] * rd[:, 1]) + T[1, 2] * rd[:, 2], rd[:, 2]], 1)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, want)
