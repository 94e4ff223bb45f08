"""RobustOutlierFilter at its branch and scale edges: the cases, an independent
reference and the bars, shared by tests/test_robust_reference.py (the oracle,
on a CPU) and tests/test_gpu_robust_edges.py (the device).

The reference (NpRobust) restates RobustOutlierFilter's constructor,
robustFiltering and computePointToPlaneDistance (OutlierFiltersImpl.cpp:394-598)
and the Matches scale estimators (Matches.cpp:60-129) step by step in T with
numpy.  It shares no code with oracle/ or the device; every branch is decided
on the T-rounded e^2, as the reference decides it.

Scenes.  The reference cloud is a dyadic lattice: 16 points per axis at spacing
8, at +-4, +-12, ... +-60, so its mean is exactly 0 in T.  Reading point i is
lattice point i mod 4096 moved along x by an offset a_i, |a_i| < 1 or a_i = 2,
with at most 10 significant bits and no bit below 2^-18 (the float grain at
|x| < 64).  Then x + a_i, the difference back and d = a_i^2 are all exact in
float, the nearest lattice point is the owner (d <= 4 against >= 36), and with
k = 2 and a search radius of 1 the second entry is (inf, -1).  Under
scaleEstimator none s = 1 and e^2 = d exactly, so a dyadic tuning puts e^2 on a
threshold exactly, and the neighbouring 10-bit offsets put it on the nearest
representable squares on either side.  N = 4099 (no multiple of 256), M = 4096.

Bars (check_call):
  scale    bit-equal for none, mad, berg; std within 4e-7 / 1e-13 where finite
           (fp64 sums in another order); NaN exactly where the reference is NaN.
  weights  the patterns w == 0, isnan, isinf equal everywhere; bit-equal where
           the reference value is exact by construction (0, the 1e-50 clamp, and
           1 from a branch, a division by 1 or exp / pow of 0); rtol 1e-6 / 1e-12
           elsewhere in the normal range.  Where exp / pow returned a subnormal p
           of T the bar is SUBNORMAL_QUANTA quanta of p, carried through the
           factors that follow it (Student multiplies p by (k + 3) / (k + e^2)):
           a subnormal has lost its relative precision, and two libm's that are
           each within 2 ulp of the true p can differ by that many quanta.
           For that reason the underflow offsets keep p either >= 4 quanta or
           below a third of one, where every such libm agrees on zero / non-zero.
  counts   kept = finite(d) & (w != 0), NaN and inf counted as non-zero.
"""
import math
from dataclasses import dataclass, field

import numpy as np

FCTS = ["cauchy", "welsch", "sc", "gm", "tukey", "huber", "L1", "student"]
BERG = {"cauchy": 4.3040, "tukey": 7.0589, "huber": 2.0138}
TOL = {np.float32: 1e-6, np.float64: 1e-12}
STD_TOL = {np.float32: 4e-7, np.float64: 1e-13}
SUBNORMAL_QUANTA = 4

AXIS, SPACING = 16, 8.0
M, N = AXIS ** 3, AXIS ** 3 + 3
FAR = 2.0   # an offset outside the search radius of 1: its entries are (inf, -1) under that radius


class NpRobust:
    """numpy restatement of the reference object (constructor + robustFiltering)."""

    def __init__(self, dtype, fct="cauchy", tuning=1.0, scale="mad", nb=0, approx=np.inf, p2pl=False):
        T = np.dtype(dtype).type
        self.T, self.fct, self.scale_est, self.nb, self.p2pl = T, fct, scale, nb, p2pl
        self.k = T(tuning)
        self.target = T(0)
        if scale == "berg":
            self.target = T(tuning)
            if fct in BERG:
                self.k = T(BERG[fct])
        self.sqa = T(np.inf) if np.isinf(approx) else T(T(approx) ** 2)
        self.it, self.scale = 1, T(0)

    def p2pl_distance(self, ids, pts, ref, normals):
        """computePointToPlaneDistance (:466-499): 0 for an invalid id; the normal
        normalised in T (Eigen normalized(): v / sqrt(v.v), v itself when v.v is 0)."""
        T = self.T
        with np.errstate(all="ignore"):
            j = np.where(ids >= 0, ids, 0)
            n = normals[j].astype(T)
            sq = ((n[..., 0] * n[..., 0] + n[..., 1] * n[..., 1]) + n[..., 2] * n[..., 2]).astype(T)
            nn = np.where(sq > 0, np.sqrt(sq), T(1)).astype(T)
            n = (n / nn[..., None]).astype(T)
            dl = (pts[:, None, :3] - ref[j][..., :3]).astype(T)
            dot = ((n[..., 0] * dl[..., 0] + n[..., 1] * dl[..., 1]) + n[..., 2] * dl[..., 2]).astype(T)
            return np.where(ids >= 0, dot * dot, T(0)).astype(T)

    def weights(self, d, ids=None, pts=None, ref=None, normals=None):
        T = self.T
        rec = self.it <= self.nb or self.nb == 0
        fin = d[d != np.inf]
        if self.scale_est in ("mad", "berg") and rec and not (self.scale_est == "berg" and self.it > 1) \
                and fin.size == 0:
            raise ValueError("no outlier to filter")
        with np.errstate(all="ignore"):
            if self.scale_est == "mad" and rec:
                med = np.sort(fin)[len(fin) // 2]
                dev = np.abs(fin - med).astype(T)
                self.scale = T(np.sqrt(np.sort(dev)[len(dev) // 2]))
            elif self.scale_est == "std" and rec:
                s = np.sum(d.astype(np.float64))
                mean = T(s / d.size)
                c = (d - mean).astype(T)
                var = T(T(np.sum((c * c).astype(np.float64))) / T(d.size - 1))
                self.scale = T(np.sqrt(T(np.sqrt(var))))
            elif self.scale_est == "berg" and rec:
                if self.it == 1:
                    q = np.partition(fin, int(T(len(fin)) * T(0.5)))[int(T(len(fin)) * T(0.5))]
                    self.scale = T(1.9 * float(T(np.sqrt(q))))
                else:
                    self.scale = T(T(0.85) * (self.scale - self.target) + self.target)
            elif self.scale_est == "none":
                self.scale = T(1)
            self.it += 1
            dist = self.p2pl_distance(ids, pts, ref, normals) if self.p2pl else d
            e2 = (dist / (self.scale * self.scale)).astype(T)
            k, k2 = self.k, T(self.k * self.k)
            one = T(1)
            f = self.fct
            # p: what exp / pow returned (None elsewhere); gain: |dw / dp| after it
            self.p, self.gain = None, None
            if f == "cauchy":
                w = one / (one + e2 / k2)
            elif f == "welsch":
                w = np.exp(-e2 / k2)
                self.p, self.gain = w.astype(T), np.ones(e2.shape)
            elif f == "sc":
                s = (k + e2).astype(T)
                w = np.where(e2 >= k, T(4.0 * float(k2)) * (one / (s * s)), one)
            elif f == "gm":
                s = (k + e2).astype(T)
                w = k2 * (one / (s * s))
            elif f == "tukey":
                a = (one - e2 / k2).astype(T)
                w = np.where(e2 >= k2, T(0), a * a)
            elif f == "huber":
                w = np.where(e2 >= k2, k * (one / np.sqrt(e2)), one)
            elif f == "L1":
                w = one / np.sqrt(e2)
            else:
                dd = T(3)
                p = np.power(one + e2 / k, -(k + dd) / T(2)).astype(T)
                w = p * (k + dd) * (one / (k + e2))
                self.p = p
                self.gain = np.abs(np.float64(k + dd) / (np.float64(k) + e2.astype(np.float64)))
            w = w.astype(T)
            self.raw, self.e2 = w, e2
            w = np.where(w <= T(1e-50), T(1e-50), w).astype(T)
            if not np.isinf(self.sqa):
                w = np.where(e2 >= self.sqa, T(0), w).astype(T)
        return w


# ---------------------------------------------------------------- scenes --
def ten_bits(a):
    """a has at most 10 significant bits and none below 2^-18"""
    if a == 0:
        return True
    m, _ = math.frexp(abs(a))
    return (m * 1024).is_integer() and (abs(a) * 2 ** 18).is_integer()


def neighbours(a):
    """the 10-bit numbers just below and just above a > 0"""
    m, e = math.frexp(a)          # a = m 2^e, m in [0.5, 1)
    m = int(m * 1024)             # [512, 1024)
    lo = (m - 1) * 2.0 ** (e - 10) if m > 512 else 1023 * 2.0 ** (e - 11)
    return lo, (m + 1) * 2.0 ** (e - 10)


def lattice(dtype):
    c = (np.arange(AXIS) - (AXIS - 1) / 2) * SPACING
    x, y, z = np.meshgrid(c, c, c, indexing="ij")
    ref = np.stack([x.ravel(), y.ravel(), z.ravel(), np.ones(M)], axis=1).astype(dtype)
    assert np.all(ref[:, :3].astype(np.float64).sum(0) == 0)
    return ref


UNIT_NORMALS = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.6, 0.8, 0], [0, -0.6, 0.8], [-1, 0, 0]], np.float64)
ODD_NORMALS = np.array([[0, 0, 0], [2, 0, 0], [3, 4, 0], [1, 1, 1], [0, 0, 0], [-0.5, 0, 0]], np.float64)


def lattice_normals(dtype, odd=False):
    n = UNIT_NORMALS[np.arange(M) % len(UNIT_NORMALS)].copy()
    if odd:   # every 7th lattice point: a zero or an unnormalised normal
        j = np.arange(0, M, 7)
        n[j] = ODD_NORMALS[np.arange(j.size) % len(ODD_NORMALS)]
    return n.astype(dtype)


def shares(values, counts, n=N, seed=5):
    """n offsets: values[i] counts[i] times (the last value fills up), in a fixed
    shuffled order with shuffled signs"""
    counts = list(counts)
    counts[-1] = n - sum(counts[:-1])
    assert len(counts) == len(values) and min(counts) >= 0
    a = np.repeat(np.asarray(values, np.float64), counts)
    rng = np.random.default_rng(seed)
    a = a[rng.permutation(n)]
    return a * rng.choice([-1.0, 1.0], n)


def spread(values, n=N, seed=5):
    return shares(values, [n // len(values)] * len(values), n, seed)


@dataclass
class Case:
    name: str
    fct: str
    offsets: np.ndarray                      # one per reading point
    tuning: float = 0.5
    scale: str = "none"
    approx: float = np.inf
    nb: int = 0
    calls: int = 1
    p2pl: bool = False
    odd_normals: bool = False
    radius_k1: float = np.inf                # the search radius of the k = 1 run (k = 2 always runs with 1)
    ks: tuple = (1, 2)
    raises: bool = False                     # no finite entry: mad / berg throw
    bands: dict = field(default_factory=dict)  # band name -> predicate(expected call) that must hold somewhere

    def params(self):
        p = {"robustFct": self.fct, "scaleEstimator": self.scale, "tuning": self.tuning,
             "nbIterationForScale": self.nb, "approximation": self.approx}
        if self.p2pl:
            p["distanceType"] = "point2plane"
        return p


@dataclass
class Scene:
    ref: np.ndarray
    nrm: np.ndarray
    rd: np.ndarray
    k: int
    max_dist: float
    d: np.ndarray       # the intended match, (N, k)
    ids: np.ndarray


def scene(case, dtype, k):
    a = np.asarray(case.offsets, np.float64)
    assert all(ten_bits(float(v)) for v in np.unique(a)) and np.all((np.abs(a) < 1) | (np.abs(a) == FAR))
    n = a.size
    ref = lattice(dtype)
    own = (np.arange(n) % M).astype(np.int32)
    rd = ref[own].copy()
    rd[:, 0] = (rd[:, 0].astype(np.float64) + a).astype(dtype)
    assert np.array_equal(rd[:, 0].astype(np.float64), ref[own, 0].astype(np.float64) + a)   # exact in T
    max_dist = 1.0 if k == 2 else case.radius_k1
    d = np.full((n, k), np.inf, dtype)
    ids = np.full((n, k), -1, np.int32)
    hit = a * a <= max_dist ** 2
    d[hit, 0] = (a[hit] * a[hit]).astype(dtype)
    assert np.array_equal(d[hit, 0].astype(np.float64), a[hit] * a[hit])
    ids[hit, 0] = own[hit]
    return Scene(ref, lattice_normals(dtype, case.odd_normals), rd, k, max_dist, d, ids)


# ----------------------------------------------------------------- cases --
def _f32(dtype):
    return np.dtype(dtype) == np.float32


def _has(pred):
    return lambda x: bool(np.any(pred(x)))


def _tiny(x):
    return np.finfo(x.raw.dtype).tiny


def thresholds_cases(dtype):
    thr = [0.25, 0.5, 0.75]
    vals = [0.125, 0.375, 0.875]
    for t in thr:
        vals += [t, *neighbours(t)]
    off = spread(vals)

    def around(v):
        return {f"e2 == {v}": _has(lambda x: x.e2 == v), f"e2 just below {v}": _has(
            lambda x: x.e2 == x.e2.dtype.type(neighbours(math.sqrt(v))[0]) ** 2),
            f"e2 just above {v}": _has(lambda x: x.e2 == x.e2.dtype.type(neighbours(math.sqrt(v))[1]) ** 2)}

    yield Case("thresholds-sc", "sc", off, tuning=0.25, bands={**around(0.25), **around(0.0625)})   # e2 >= k, not k^2
    yield Case("thresholds-tukey", "tukey", off, tuning=0.5, bands=around(0.25))
    yield Case("thresholds-huber", "huber", off, tuning=0.5, bands=around(0.25))
    yield Case("thresholds-approx", "cauchy", off, tuning=1.0, approx=0.5, bands=around(0.25))
    # the clamp and the cut compose: cut below the Tukey threshold, and above it
    # (Tukey's 0 -> 1e-50 in double between the two, -> 0 again past the cut)
    yield Case("thresholds-tukey-cut-below", "tukey", off, tuning=0.5, approx=0.25, bands=around(0.0625))
    yield Case("thresholds-tukey-cut-above", "tukey", off, tuning=0.5, approx=0.75, bands={
        **around(0.5625), "clamped 0": _has(lambda x: (x.raw == 0) & (x.e2 < 0.5625))})


def zero_distance_cases(dtype):
    vals = [0.0, 0.125, 0.25, 0.5, 0.75]
    off = shares(vals, [N // 4, N // 8, N // 4, N // 4, 0])
    for fct in FCTS:
        yield Case(f"zero-none-{fct}", fct, off, tuning=0.5, bands={"d == 0": _has(lambda x: x.e2 == 0)})
        yield Case(f"zero-mad-{fct}", fct, off, tuning=0.5, scale="mad", bands={
            "d == 0": _has(lambda x: x.e2 == 0), "MAD > 0": lambda x: x.scale > 0})


def underflow_cases(dtype):
    """Welsch: e2 / k^2 = a^2 / k^2 through the normal range of exp's result, the
    subnormal band of T and past it.  Student: k tiny, so (1 + e2 / k)^(-(k + 3) / 2)
    = (d / k)^-1.5 runs through the same bands.  In double everything at or below
    1e-50 ends on the clamp; offsets sit on both sides of it."""
    sub = lambda x: (x.p > 0) & (x.p < _tiny(x))
    if _f32(dtype):
        # a = j / 1024, k = 2^-4: e2 / k^2 = j^2 / 4096
        #   normal  <= 86.7 (j <= 596) | subnormal 87.9 .. 101.9 (600 .. 646, >= 4 quanta) | zero >= 106.3 (j >= 660)
        j = [64, 256, 512, 590, 596, 600, 610, 620, 630, 640, 646, 660, 700, 800, 1000]
        yield Case("underflow-welsch", "welsch", spread([v / 1024 for v in j]), tuning=2.0 ** -4, bands={
            "normal": _has(lambda x: x.p >= _tiny(x)), "subnormal": _has(sub), "exact 0": _has(lambda x: x.p == 0)})
        # k = 2^-104, a = 2^-m: p = 2^(3m - 156); >= 2^-126 normal (m >= 10), 2^-147 (4 quanta, m = 3) .. 2^-129
        # subnormal, 2^-153 (m = 1) and 0.75, 0.875 (0.29, 0.18 of a quantum) zero
        a = [2.0 ** -1, 0.75, 0.875, 2.0 ** -3, 2.0 ** -4, 3 * 2.0 ** -6, 2.0 ** -5, 2.0 ** -6, 2.0 ** -8,
             5 * 2.0 ** -11, 2.0 ** -10, 2.0 ** -12, 2.0 ** -14, 3 * 2.0 ** -17, 2.0 ** -16]
        yield Case("underflow-student", "student", spread(a), tuning=2.0 ** -104, bands={
            "normal": _has(lambda x: x.p >= _tiny(x)), "subnormal": _has(sub), "exact 0": _has(lambda x: x.p == 0)})
    else:
        # a = j / 1024, k = 2^-5: e2 / k^2 = j^2 / 1024
        #   above the clamp < 115.13 (j <= 343: 114.9) | below it, normal (344: 115.6 .. 850: 705.6)
        #   | subnormal 713.9 .. 739.2 (855 .. 870) | exact 0 >= 756.3 (j >= 880)
        j = [64, 256, 340, 343, 344, 350, 400, 700, 850, 855, 860, 870, 880, 1000]
        clamp = {"above the clamp": _has(lambda x: x.raw > 1e-50),
                 "clamped from the normal range": _has(lambda x: (x.p >= _tiny(x)) & (x.raw <= 1e-50))}
        yield Case("underflow-welsch", "welsch", spread([v / 1024 for v in j]), tuning=2.0 ** -5, bands={
            **clamp, "clamped subnormal": _has(sub), "clamped 0": _has(lambda x: x.p == 0)})
        # k = 2^-120: w = 3 d^-2.5 2^-180 against 1e-50 = 2^-166.1: a = 23/128 is 4.7 % above, 3/16 15 % below
        a = [2.0 ** -6, 2.0 ** -4, 2.0 ** -3, 23 / 128, 3 / 16, 2.0 ** -2, 0.5, 0.875]
        yield Case("underflow-student-clamp", "student", spread(a), tuning=2.0 ** -120, bands=clamp)
        # k = 2^-718: p = d^-1.5 2^-1077: 0.875, 0.75 are 0.19, 0.30 of a quantum (zero); 2^-2 is 8 quanta; 2^-17 is
        # 2^-1026 (subnormal); everything ends on the clamp
        a = [0.875, 0.75, 2.0 ** -2, 2.0 ** -3, 2.0 ** -10, 2.0 ** -17]
        yield Case("underflow-student-deep", "student", spread(a), tuning=2.0 ** -718, bands={
            "clamped subnormal": _has(sub), "clamped 0": _has(lambda x: x.p == 0)})


def scale_degenerate_cases(dtype):
    same = shares([0.5], [N])
    twins = shares([0.0, 0.5], [N // 4, 0])
    zero_scale = {"scale == 0": lambda x: x.scale == 0}
    for fct in ("cauchy", "tukey", "L1", "sc"):
        # all finite distances equal: MAD 0, and std 0 where no entry is inf (k = 1)
        yield Case(f"degenerate-equal-mad-{fct}", fct, same, scale="mad", bands={
            **zero_scale, "e2 == inf": _has(lambda x: np.isinf(x.e2))})
        yield Case(f"degenerate-equal-std-{fct}", fct, same, scale="std", ks=(1,), bands=zero_scale)
    for fct in ("cauchy", "sc", "huber", "L1"):
        # ... with twins at d = 0: e2 = 0 / 0 (sc and huber answer 1 to a NaN, the others NaN)
        yield Case(f"degenerate-twins-mad-{fct}", fct, twins, scale="mad", bands={
            **zero_scale, "e2 is NaN": _has(lambda x: np.isnan(x.e2))})
        # std over a match that holds inf entries is NaN
        yield Case(f"degenerate-std-inf-{fct}", fct, twins, scale="std", ks=(2,), bands={
            "scale is NaN": lambda x: np.isnan(x.scale)})
    one = shares([0.5, FAR], [1, 0])
    none = shares([FAR], [N])
    for est in ("mad", "berg"):
        yield Case(f"degenerate-one-finite-{est}", "cauchy", one, scale=est, tuning=1.0, radius_k1=1.0, bands={
            "one finite entry": lambda x: x.n_finite == 1})
        yield Case(f"degenerate-no-finite-{est}", "cauchy", none, scale=est, tuning=1.0, radius_k1=1.0, raises=True)


def median_ties_cases(dtype):
    """Two distances; n finite entries of which L are low.  The size / 2 index is
    the last low one for L = n / 2 + 1 and the first high one for L = n / 2."""
    for n in (N, N - 1):
        for where, L in (("last-low", n // 2 + 1), ("first-high", n // 2)):
            off = shares([0.25, 0.5], [L, 0], n=n)
            want = 0.0625 if where == "last-low" else 0.25
            band = {f"median on the {where}": lambda x, want=want: x.median == want}
            # mad, nbIterationForScale 1: compute, keep, keep
            yield Case(f"ties-mad-{n}-{where}", "cauchy", off, tuning=1.0, scale="mad", nb=1, calls=3, bands=band)
            # berg, nbIterationForScale 2: first, next, keep
            yield Case(f"ties-berg-{n}-{where}", "cauchy", off, tuning=1.0, scale="berg", nb=2, calls=3, bands=band)


def p2pl_invalid_cases(dtype):
    off = spread([0.125, 0.25, 0.5, 0.75])
    bands = {"invalid entries": _has(lambda x: x.ids < 0), "zero normal": _has(lambda x: (x.e2 == 0) & (x.ids >= 0))}
    yield Case("p2pl-L1", "L1", off, p2pl=True, odd_normals=True, ks=(2,), bands={
        **bands, "inf at an invalid entry": _has(lambda x: np.isinf(x.w) & (x.ids < 0))})
    yield Case("p2pl-cauchy", "cauchy", off, p2pl=True, odd_normals=True, ks=(2,), bands=bands)
    yield Case("p2pl-cauchy-mad", "cauchy", off, scale="mad", tuning=1.0, p2pl=True, odd_normals=True, ks=(2,),
               bands=bands)


GROUPS = {"thresholds": thresholds_cases, "zero_distance": zero_distance_cases, "underflow": underflow_cases,
          "scale_degenerate": scale_degenerate_cases, "median_ties": median_ties_cases,
          "p2pl_invalid": p2pl_invalid_cases}


def case_ids():
    """(group, case name, dtype) of every case, for parametrize"""
    out = []
    for dtype in (np.float32, np.float64):
        for g, gen in GROUPS.items():
            out += [(g, c.name, dtype) for c in gen(dtype)]
    return out


def get_case(group, name, dtype):
    return next(c for c in GROUPS[group](dtype) if c.name == name)


# -------------------------------------------------------------- expected --
@dataclass
class Expected:
    scale: float
    w: np.ndarray
    raw: np.ndarray     # before the clamp and the cut
    e2: np.ndarray
    p: np.ndarray       # exp / pow's result (zeros elsewhere)
    gain: np.ndarray
    has_p: bool
    ids: np.ndarray
    n_finite: int
    median: float


_EXPECTED = {}


def expected(case, dtype, k):
    """[Expected per call of the schedule] on the intended match, or None where
    the estimator throws; computed once per (case, dtype, k) and left unchanged"""
    key = (case.name, np.dtype(dtype).name, k)
    if key not in _EXPECTED:
        sc = scene(case, dtype, k)
        r = NpRobust(dtype, case.fct, case.tuning, case.scale, case.nb, case.approx, case.p2pl)
        fin = sc.d[np.isfinite(sc.d)]
        out = []
        try:
            for _ in range(case.calls):
                w = r.weights(sc.d, sc.ids, sc.rd, sc.ref, sc.nrm)
                has_p = r.p is not None
                for a in (w, r.raw, r.e2):
                    a.setflags(write=False)
                out.append(Expected(float(r.scale), w, r.raw, r.e2, r.p if has_p else np.zeros_like(w),
                                    r.gain if has_p else np.zeros(w.shape), has_p, sc.ids, fin.size,
                                    float(np.sort(fin)[fin.size // 2]) if fin.size else np.nan))
        except ValueError:
            out = None
        _EXPECTED[key] = out
    return _EXPECTED[key]


def scale_mode(P, it, scale, nb):
    """the device's scale mode of filter call `it` (1-based): the host class's schedule"""
    rec = it <= nb or nb == 0
    if scale == "mad":
        return P.RS_MAD if rec else P.RS_KEEP
    if scale == "std":
        return P.RS_STD if rec else P.RS_KEEP
    if scale == "berg":
        return P.RS_KEEP if not rec else (P.RS_BERG_FIRST if it == 1 else P.RS_BERG_NEXT)
    return P.RS_NONE


def device_tuning(case):
    """(tuning, berg target) as the host class hands them to the device"""
    if case.scale == "berg":
        return BERG.get(case.fct, case.tuning), case.tuning
    return case.tuning, 0.0


# ------------------------------------------------------------------ bars --
def check_bands(case, exp):
    """every band the case is about holds entries; returns the populated counts"""
    counts = {}
    for name, pred in case.bands.items():
        ok = [bool(pred(x)) for x in exp]
        assert any(ok), f"{case.name}: band '{name}' is empty"
        counts[name] = sum(ok)
    return counts


def band_counts(x):
    """entries of one call by the bar that applies to them"""
    T = x.w.dtype.type
    tiny = np.finfo(T).tiny
    sub = x.has_p & (x.p > 0) & (x.p < tiny)
    clamp = (x.w == T(1e-50)) if T is np.float64 else np.zeros(x.w.shape, bool)
    return {"w == 0": int((x.w == 0).sum()), "w == 1": int((x.w == 1).sum()), "clamp": int(clamp.sum()),
            "nan": int(np.isnan(x.w).sum()), "inf": int(np.isinf(x.w).sum()),
            "subnormal p": int((sub & ~clamp & (x.w != 0)).sum()),
            "rtol": int((np.isfinite(x.w) & (x.w != 0) & (x.w != 1) & ~clamp & ~sub).sum())}


def check_call(case, x, scale, w, who):
    """scale and weights of one call against the reference's Expected x"""
    T = x.w.dtype.type
    assert w.dtype == x.w.dtype and w.shape == x.w.shape
    # scale
    if np.isnan(x.scale):
        assert np.isnan(scale), (who, case.name, scale)
    elif case.scale == "std":
        assert abs(scale - x.scale) <= STD_TOL[T] * abs(x.scale), (who, case.name, scale, x.scale)
    else:
        assert scale == x.scale, (who, case.name, scale, x.scale)
    # patterns
    for name, f in (("zero", lambda a: a == 0), ("nan", np.isnan), ("inf", np.isinf)):
        bad = f(w) != f(x.w)
        assert not bad.any(), (who, case.name, name, int(bad.sum()), w[bad][:4], x.w[bad][:4], x.e2[bad][:4])
    fin = np.isfinite(x.w)
    assert np.array_equal(np.signbit(w[~fin & ~np.isnan(x.w)]), np.signbit(x.w[~fin & ~np.isnan(x.w)]))
    # exact by construction: 0, the clamp, and 1 from a branch / a division by 1 / exp or pow of 0
    one = (x.w == 1) & ((not x.has_p) | (x.e2 == 0))
    exact = fin & ((x.w == 0) | one)
    if T is np.float64:
        exact |= x.w == T(1e-50)
    bad = exact & (w != x.w)
    assert not bad.any(), (who, case.name, "exact", int(bad.sum()), w[bad][:4], x.w[bad][:4], x.e2[bad][:4])
    # subnormal p: a few quanta of p, carried through what follows it; rtol elsewhere
    quantum = float(np.finfo(T).smallest_subnormal)
    sub = fin & ~exact & x.has_p & (x.p < np.finfo(T).tiny)
    with np.errstate(invalid="ignore"):   # (inf - inf where both are inf: judged by the patterns above)
        err = np.abs(w.astype(np.float64) - x.w.astype(np.float64))
    bound = np.where(sub, SUBNORMAL_QUANTA * quantum * x.gain + TOL[T] * np.abs(x.w), TOL[T] * np.abs(x.w))
    bad = fin & ~exact & ~(err <= bound)
    assert not bad.any(), (who, case.name, "value", int(bad.sum()), w[bad][:4], x.w[bad][:4], x.e2[bad][:4])


def want_counts(d, w):
    finite = np.isfinite(d)
    nz = w != 0     # (NaN and inf included)
    kept = finite & nz
    return dict(nonzero_weights=int(nz.sum()), kept=int(kept.sum()), rejected_matches=int((finite & ~nz).sum()),
                rejected_points=int((~kept.any(axis=1)).sum())), kept
