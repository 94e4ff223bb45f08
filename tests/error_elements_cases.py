"""The yardstick of ErrorMinimizer::getErrorElements: the constructor of
ErrorElements (ErrorMinimizer.cpp:58-193) restated in numpy.

A column is an entry (i, s) of the k x N match with dist != inf and w != 0, in
the order of the loop at :98-135: the reading point rising, the link rank
rising within it, which is np.nonzero's order on the N x k mirrors (the order
quality_cases.restate uses).  Every value is a copy of a stored one, so the
comparisons against it are exact.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(__file__))
import quality_cases as Q  # noqa: E402

FIELDS = ("reading", "reference", "dists", "ids", "weights", "reading_index", "link_rank")


def step_reading(T, rd):
    """The step reading the columns hold: quality_cases.xform3 of rd (n x rows)
    under T (rows x rows), the homogeneous row the point's own.  A 2-D cloud goes
    through the embedded form (x, y, 0, h), whose z terms add an exact 0."""
    dtype = rd.dtype
    T = np.asarray(T, dtype)
    if rd.shape[1] == 4:
        return np.ascontiguousarray(np.c_[Q.xform3(T, rd), rd[:, 3]], dtype=dtype)
    T4 = np.zeros((4, 4), dtype)
    T4[np.ix_([0, 1, 3], [0, 1, 3])] = T
    T4[2, 2] = 1
    p4 = np.zeros((len(rd), 4), dtype)
    p4[:, [0, 1, 3]] = rd
    return np.ascontiguousarray(np.c_[Q.xform3(T4, p4)[:, :2], rd[:, 2]], dtype=dtype)


def restate(d, ids, w, rd_step, ref, nrm=None):
    """d, ids, w: N x k (the mirrors); rd_step N x rows (step_reading); ref M x
    rows; nrm M x D or None.  Returns the columns and the two rejected counts."""
    d, w, ids = np.asarray(d), np.asarray(w), np.asarray(ids)
    finite = d != np.inf
    kept = finite & (w != 0)
    qi, s = np.nonzero(kept)
    out = dict(reading=rd_step[qi], reference=np.asarray(ref)[ids[qi, s]], dists=d[qi, s],
               ids=ids[qi, s].astype(np.int32), weights=w[qi, s], reading_index=qi.astype(np.int32),
               link_rank=s.astype(np.int32), ref_normals=None if nrm is None else np.asarray(nrm)[ids[qi, s]],
               rejected_matches=int((finite & ~kept).sum()), rejected_points=int((~kept.any(1)).sum()))
    return out


def assert_equal(got, want, tag=""):
    """got: an ErrorElements-like object or dict; want: restate's dict.  Exact."""
    g = got if isinstance(got, dict) else got.__dict__
    for f in FIELDS:
        assert g[f].dtype == want[f].dtype, (tag, f, g[f].dtype, want[f].dtype)
        np.testing.assert_array_equal(g[f], want[f], err_msg=f"{tag} {f}")
    if want["ref_normals"] is not None and g.get("ref_normals") is not None:
        np.testing.assert_array_equal(g["ref_normals"], want["ref_normals"], err_msg=f"{tag} ref_normals")
    assert int(g["rejected_matches"]) == want["rejected_matches"], tag
    assert int(g["rejected_points"]) == want["rejected_points"], tag
