"""Designed weight sets for the resampling kernels, exact references and a restatement of the kernels' own cumulative sum
(a plain helper module: no GPU, no device import).

The random weights of the other resampling tests, exp(-ll) + 1e-300, never produce what a real track does: a lost track
(every weight at the 1e-300 floor: exactly uniform), one survivor with N copies -- at index 0, at N - 1, on a thread-segment
or wave boundary -- or weights that span 300 orders of magnitude.  CASES(n) names those sets.

Three things are compared on them:

  * exact_systematic / exact_stratified / exact_choice: the resampling in rational arithmetic (fractions.Fraction), with,
    per position, its distance to the nearest cumulative weight;
  * decided(gap, n): a position further than 8 n 2^-53 from every cumulative weight is served by the same source whatever
    the association of the float64 cumulative sum -- an n-term sum of values <= 1 is off by at most n 2^-53 (n - 1
    additions, each rounding a value <= 1 by <= 2^-53, plus the division w / total: 2^-53 relative per term, the total
    itself another n 2^-53 relative), doubled for the two sides compared, doubled again for the position's own rounding
    and slack.  NumPy's sequential np.cumsum, the kernels' segmented scan and the rational sum agree on every decided
    position;
  * kernel_cumsum / kernel_systematic / kernel_stratified / kernel_choice: k_resample's exact arithmetic restated in NumPy
    operation for operation (glh_kernels.h: cumsum_inplace): on a tie only this can be held bit for bit.

tests/test_resample_cases.py admits the cases on the CPU (the restatement equals oracle.resample on every decided
position: it is not tuned to the device); tests/test_gpu_resample_cases.py runs the kernels on them.
"""
from fractions import Fraction

import numpy as np

from tests.fast_math_reference import LD, require_longdouble

BLK = 256   # threads of k_resample (glh_kernels.h)
WAVE = 64
FLOOR = 1e-300   # what exp(-ll) + 1e-300 leaves of a particle whose likelihood underflows
SPIKE = 3e-7
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 5000)
LAST_U = float(np.nextafter(1.0, 0.0))
U_RANDOM = 0.7236548159      # "one fixed random value": decided on every case and count (test_resample_cases.py)
U_DECIDED = (0.5, U_RANDOM)
U_CHOICE = 0.3819660113      # choice compares u itself with the cdf: 0.5 at every position ties with k / n at every even n
U_TIES = (0.0, LAST_U)


def segment(n, blk=BLK):
    """Elements per thread of the kernels' segmented scan."""
    return -(-n // blk)


def segment_edges(n, blk=BLK):
    """First and last index of one thread's segment: thread 65 (the second lane of the second wave) where the count
    reaches it, else the last thread that owns anything."""
    seg = segment(n, blk)
    t = min(65, (n - 1) // seg)
    return t * seg, min(t * seg + seg, n) - 1


def spike_positions(n, blk=BLK):
    """{name: k} of the one-survivor cases at count n (positions beyond n - 1 dropped, duplicates kept once)."""
    first, last = segment_edges(n, blk)
    out = {}
    for name, k in (("0", 0), ("last", n - 1), ("mid", n // 2), ("63", 63), ("64", 64), ("seg_first", first),
                    ("seg_last", last)):
        if 0 <= k < n and k not in out.values():
            out[name] = k
    return out


def CASES(n):
    """[(name, weights (n,))]: the designed weight sets at count n.  The NaN sets come last."""
    rng = np.random.default_rng(1000 + n)
    cases = [("floor", np.full(n, FLOOR)), ("ones", np.ones(n))]
    for name, k in spike_positions(n).items():
        w = np.full(n, FLOOR)
        w[k] = SPIKE
        cases.append((f"spike_{name}", w))
    w = np.full(n, FLOOR)
    w[0] = w[-1] = SPIKE
    cases.append(("ends", w))
    geom = np.geomspace(FLOOR, 1.0, n)
    cases.append(("geom_up", geom))
    cases.append(("geom_down", geom[::-1].copy()))
    cases.append(("wide", np.exp(-700.0 * rng.random(n)) + FLOOR))
    for name, k in (("nan_front", 0), ("nan_back", n - 1)):
        w = np.exp(-rng.random(n)) + FLOOR
        w[k] = np.nan
        cases.append((name, w))
    return cases


def has_nan(w):
    return bool(np.isnan(w).any())


# ---- the exact answer ------------------------------------------------------------------------------------------------
def _scaled(values):
    """Finite float64 values as integers over one common power-of-two denominator: (ints, denominator)."""
    fr = [Fraction(float(v)) for v in values]
    den = max(f.denominator for f in fr)
    return [f.numerator * (den // f.denominator) for f in fr], den


def _exact(w, positions_num, positions_den, side):
    """Positions p_j = positions_num[j] / positions_den against the cumulative weights C_k / T (C: exact running sums of
    w, T = C[-1]): idx_j = #{k : C_k / T < p_j} (side 'left') or <= (side 'right'); gap_j, the distance from p_j to
    the nearest cumulative weight, as float; and lo_j <= idx_j <= hi_j, the same counts at p_j -+ 8 n 2^-53 (`reach`).
    Everything is compared as integers: p_j T <=> C_k positions_den."""
    wi, _ = _scaled(w)
    cum, run = [], 0
    for v in wi:
        run += v
        cum.append(run)
    total = cum[-1]
    keys = [c * positions_den for c in cum]         # C_k den, non-decreasing
    import bisect

    find = bisect.bisect_left if side == "left" else bisect.bisect_right
    tol = Fraction(8 * len(wi), 2 ** 53) * total * positions_den
    tol = -(-tol.numerator // tol.denominator)       # (rounded up to an integer: the keys are integers)
    idx, gap, lo, hi = [], [], [], []
    for num in positions_num:
        x = num * total                              # p_j T den
        i = find(keys, x)
        near = min(abs(x - keys[q]) for q in (i - 1, i) if 0 <= q < len(keys))
        idx.append(i)
        gap.append(float(Fraction(near, total * positions_den)))
        lo.append(find(keys, x - tol))
        hi.append(find(keys, x + tol))
    return np.array(idx), np.array(gap), np.array(lo), np.array(hi)


def _answer(full, reach):
    return full if reach else full[:2]


def exact_systematic(w, u, reach=False):
    """np.searchsorted(cumsum(w / w.sum()), (arange(n) + u) / n) in rational arithmetic: (indices, gaps), with `reach`
    (indices, gaps, lo, hi).  An index n (a position beyond the last cumulative weight) cannot occur: the last cumulative
    weight is exactly 1 > (n - 1 + u) / n."""
    n = len(w)
    (ui,), den = _scaled([u])
    return _answer(_exact(w, [j * den + ui for j in range(n)], den * n, "left"), reach)


def exact_stratified(w, u, reach=False):
    """As exact_systematic with one uniform per position, u (n,)."""
    n = len(w)
    ui, den = _scaled(u)
    return _answer(_exact(w, [j * den + ui[j] for j in range(n)], den * n, "left"), reach)


def exact_choice(w, u, reach=False):
    """RandomState.choice: searchsorted(cdf / cdf[-1], u, side='right') in rational arithmetic, u (n,)."""
    ui, den = _scaled(u)
    return _answer(_exact(w, ui, den, "right"), reach)


def decided(gap, n):
    """Positions whose source does not depend on how the float64 cumulative sum is associated (module docstring)."""
    return np.asarray(gap) > 8.0 * n * 2.0 ** -53


# ---- the kernels' exact arithmetic, restated ---------------------------------------------------------------------------
def kernel_cumsum(w, total, blk=BLK, divide=True):
    """cumsum_inplace of k_resample (glh_kernels.h), exact arithmetic, operation for operation:

      * thread t owns the segment [t seg, (t + 1) seg), seg = ceil(N / blk), and sums it from the left (the quotients
        w / total when `divide`);
      * the segment totals are scanned inside every wave of 64 by the Hillis-Steele shuffle ladder (offsets 1, 2, ... 32:
        lane l adds lane l - off while l >= off);
      * the wave totals are added from the left: wave v starts at ((t_0 + t_1) + ...) + t_{v-1};
      * an element is `excl + run` -- the wave's base plus the lane's exclusive prefix, plus the running sum of its own
        segment; thread 0's running sums are used as they are.
    """
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    seg = segment(n, blk)
    q = np.zeros(blk * seg)
    q[:n] = w / total if divide else w
    run = np.cumsum(q.reshape(blk, seg), axis=1)         # sequential along a segment; the padding adds 0.0
    incl = run[:, -1].reshape(blk // WAVE, WAVE).copy()
    off = 1
    while off < WAVE:
        nxt = incl.copy()
        nxt[:, off:] = incl[:, off:] + incl[:, :-off]
        incl = nxt
        off <<= 1
    prev = np.zeros_like(incl)
    prev[:, 1:] = incl[:, :-1]
    base = np.zeros(blk // WAVE)
    for v in range(1, blk // WAVE):
        base[v] = base[v - 1] + incl[v - 1, -1]
    excl = (base[:, None] + prev).reshape(blk)
    c = excl[:, None] + run
    c[0] = run[0]
    return c.reshape(-1)[:n]


def _bisect(c, keys, right):
    """The kernels' binary search of every key in c, comparison for comparison (a NaN never compares true): #{k : c[k] <
    key} for a sorted c, or <= with `right`."""
    n = len(c)
    lo = np.zeros(len(keys), dtype=np.int64)
    hi = np.full(len(keys), n, dtype=np.int64)
    while (lo < hi).any():
        live = lo < hi
        mid = (lo + hi) >> 1
        cm = c[np.minimum(mid, n - 1)]
        with np.errstate(invalid="ignore"):
            go = (cm <= keys) if right else (cm < keys)
        lo = np.where(live & go, mid + 1, lo)
        hi = np.where(live & ~go, mid, hi)
    return lo


def _clamp(idx, n):
    clamped = bool((idx >= n).any())
    return np.minimum(idx, n - 1).astype(np.int32), clamped


def kernel_systematic(w, u, blk=BLK, contested=False):
    """k_resample, systematic, exact arithmetic: (indices, clamped), with `contested` (indices, clamped, mask).

    The kernel inverts np.searchsorted(side='left'): f(k) = #{j : pos_j <= c[k]} with pos_j = (j + u) * (1 / n) rounded as
    the reference rounds it; thread t walks its segment and writes source k to the outputs [f(k - 1), f(k)), starting from
    f of the element before its segment; the thread that owns the last element writes the last source to the outputs from
    f(n - 1) on and flags the point when there are any (np.searchsorted == n: an IndexError in the reference).  No
    comparison with a NaN is true, so NaN weights give f = 0 throughout: every output is the last source, flagged.

    The segmented cumulative sum is NOT monotone: `excl + run` of a segment's first element can lie one ulp below the
    last element of the segment before it (the two are associated differently).  Where a position ties with such a pair, f
    decreases and two threads write the same output: `mask` marks those outputs.  Their index here is the one the
    highest thread writes (thread order); the device's depends on the order its waves get there."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    c = kernel_cumsum(w, w.sum(), blk)
    pos = (np.arange(n) + u) * (1 / n)
    f = np.where(np.isnan(c), 0, np.searchsorted(pos, np.where(np.isnan(c), 0.0, c), side="right"))
    clamped = bool(f[-1] < n)
    if (np.diff(f) >= 0).all():
        idx = np.minimum(np.searchsorted(f, np.arange(n), side="right"), n - 1)   # #{k : f(k) <= j}
        mask = np.zeros(n, dtype=bool)
    else:
        idx = np.full(n, -1)
        writes = np.zeros(n, dtype=int)
        f_prev = 0
        for k in range(n):   # (f_prev carries over a segment boundary: the next thread starts from f(k0 - 1) as well)
            idx[f_prev:f[k]] = k
            writes[f_prev:f[k]] += 1
            f_prev = f[k]
        idx[f_prev:] = n - 1
        writes[f_prev:] += 1
        assert (idx >= 0).all()
        mask = writes > 1
    idx = idx.astype(np.int32)
    return (idx, clamped, mask) if contested else (idx, clamped)


def kernel_stratified(w, u, blk=BLK):
    """k_resample, stratified: one bisection per position in the segmented cumulative sum; (indices, clamped)."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    c = kernel_cumsum(w, w.sum(), blk)
    pos = (np.arange(n) + np.asarray(u, dtype=np.float64)) * (1 / n)
    return _clamp(_bisect(c, pos, right=False), n)


def kernel_choice(w, u, blk=BLK):
    """k_resample, choice: cdf = cumsum(w / w.sum()); cdf /= cdf[-1]; searchsorted(cdf, u, side='right'); (indices,
    clamped)."""
    w = np.asarray(w, dtype=np.float64)
    n = len(w)
    c = kernel_cumsum(w, w.sum(), blk)
    with np.errstate(invalid="ignore"):
        c = c / c[-1]
    return _clamp(_bisect(c, np.asarray(u, dtype=np.float64), right=True), n)


def uniforms(n, u):
    """The per-position uniforms of stratified / choice for the scalar offset u of the tests: u itself at every position,
    except the fixed random value, which stands for one fixed random vector."""
    if u == U_RANDOM:
        return np.random.default_rng(77 + n).random(n)
    return np.full(n, float(u))


def decided_offsets(name):
    """The two offsets at which every position of a case is decided.  0.5 and the fixed random value, but for "ends": its
    cumulative weights between the two spikes are all 1/2 to 1e-292, which (j + 0.5) / n hits at every odd n."""
    return (0.25 if name == "ends" else 0.5, U_RANDOM)


def choice_uniforms(n, u):
    """As `uniforms` for choice, its constant moved off the multiples of 1 / n."""
    return uniforms(n, u) if u in (U_RANDOM,) + U_TIES else np.full(n, U_CHOICE)


def check_against_exact(got, exact, n, what, monotone=True, where=None):
    """The rule for an arithmetic that is not restated: `exact` = (indices, gaps, lo, hi) of exact_*(..., reach=True).

      * on a decided position the index is the exact one;
      * on an undecided one it is within one source of it -- or, where the cumulative weights of SEVERAL sources lie within
        8 n 2^-53 of the position (a run of floor weights next to a spike is spaced 1e-294 apart: no float64 sum tells them
        apart, np.cumsum's neither), any source between lo and hi, the exact answers at position -+ 8 n 2^-53.  Where the
        cumulative weights are further apart than that, lo and hi are within one source of the exact index, and this is
        the same rule;
      * the indices never decrease (`monotone`).
    An exact index n (side='right', a position ON the last cumulative weight) is the clamped last source.  `where`
    restricts the check to a mask of positions."""
    got = np.asarray(got, dtype=np.int64)
    idx, gap, lo, hi = exact
    sel = np.ones(n, dtype=bool) if where is None else where
    want = np.minimum(idx, n - 1)
    ok = decided(gap, n) & sel
    assert (got[ok] == want[ok]).all(), (what, "decided positions differ", np.nonzero(ok & (got != want))[0][:8])
    near = np.abs(got - want) <= 1
    inside = (np.minimum(lo, n - 1) <= got) & (got <= np.minimum(hi, n - 1))
    bad = sel & ~(near | inside)
    assert not bad.any(), (what, "an undecided position is served from beyond its reach", np.nonzero(bad)[0][:8],
                           got[bad][:8], want[bad][:8])
    if monotone:
        assert (np.diff(got) >= 0).all(), (what, "the indices decrease")


# ---- moments -----------------------------------------------------------------------------------------------------------
def moments_reference(particles, weights, origin=None):
    """Weighted mean and VARIANCE of a particle set (n, 6), two passes in longdouble: (mean - origin (6,), variance (6,)).

    The sums run over x - origin (by default the first particle), which longdouble forms exactly at these scales: at
    6.7e6 m one longdouble ulp of a coordinate is 1e3 times the unit the kernel's mean is measured in, eps max|x - K| --
    the mean is therefore returned RELATIVE to the origin -- and a set of identical particles has variance exactly 0."""
    require_longdouble()
    x = np.asarray(particles, dtype=np.float64).astype(LD)
    w = np.asarray(weights, dtype=np.float64).astype(LD)
    x = x - (x[0] if origin is None else np.asarray(origin, dtype=np.float64).astype(LD))
    s0 = w.sum()
    mean = (w[:, None] * x).sum(axis=0) / s0
    d = x - mean
    var = (w[:, None] * d * d).sum(axis=0) / s0
    return mean, var
