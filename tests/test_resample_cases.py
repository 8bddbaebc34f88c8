"""The admission of the designed resampling cases (tests/resample_cases.py), on the CPU.

For the offsets the GPU test holds to "0 indices differ" (u = 0.5 and one fixed random value) every position of every case
must be DECIDED -- further than 8 n 2^-53 from every cumulative weight -- so that test cannot hide a failure behind
"undecided"; and on them the oracle (np.cumsum, sequential), the restatement of the kernels' segmented scan and the
rational answer agree on every index: the restatement is the reference's arithmetic in another association, not something
tuned to the device.  For u = 0 and nextafter(1, 0) positions tie with cumulative weights; there the restatement equals
the exact answer where decided, stays within reach of it elsewhere (resample_cases.check_against_exact), and never
decreases.
"""
import numpy as np
import pytest

from oracle import resample as oresample
from tests import resample_cases as rc


def _cases(n):
    return [(name, w) for name, w in rc.CASES(n) if not rc.has_nan(w)]


def test_case_table():
    names = [name for name, _ in rc.CASES(5000)]
    assert len(names) == len(set(names)) == 15, names
    assert rc.spike_positions(5000) == {"0": 0, "last": 4999, "mid": 2500, "63": 63, "64": 64, "seg_first": 1300,
                                        "seg_last": 1319}
    assert rc.spike_positions(1) == {"0": 0} and rc.spike_positions(1000)["seg_last"] == 263
    for n in rc.COUNTS:
        for name, w in rc.CASES(n):
            assert w.shape == (n,) and rc.has_nan(w) == name.startswith("nan"), (n, name)


def test_kernel_cumsum_is_a_cumulative_sum():
    """Against the sequential sum to rounding, and exactly where no rounding happens (integers; one thread per element)."""
    rng = np.random.default_rng(3)
    for n in (1, 64, 257, 1000, 5000, 14950):
        w = rng.integers(1, 100, n).astype(float)
        np.testing.assert_array_equal(rc.kernel_cumsum(w, 1.0), np.cumsum(w))
        w = rng.random(n)
        np.testing.assert_allclose(rc.kernel_cumsum(w, w.sum()), np.cumsum(w / w.sum()), rtol=0, atol=n * 2.0 ** -53)


@pytest.mark.parametrize("n", rc.COUNTS)
def test_decided_offsets_admit_every_case(n):
    for name, w in _cases(n):
        for u in rc.decided_offsets(name):
            what = f"n={n} {name} u={u}"
            exact, gap = rc.exact_systematic(w, u)
            assert rc.decided(gap, n).all(), (what, "undecided positions", np.nonzero(~rc.decided(gap, n))[0][:8])
            got, clamped = rc.kernel_systematic(w, u)
            assert not clamped, what
            np.testing.assert_array_equal(got, exact, err_msg=what)
            np.testing.assert_array_equal(oresample.systematic(w, u), exact, err_msg=what)

            uj = rc.uniforms(n, u)
            exact, gap = rc.exact_stratified(w, uj)
            assert rc.decided(gap, n).all(), (what, "stratified: undecided positions")
            got, clamped = rc.kernel_stratified(w, uj)
            assert not clamped, what
            np.testing.assert_array_equal(got, exact, err_msg=what)
            np.testing.assert_array_equal(oresample.stratified(w, uj), exact, err_msg=what)

            uc = rc.choice_uniforms(n, u)
            exact, gap = rc.exact_choice(w, uc)
            assert rc.decided(gap, n).all(), (what, "choice: undecided positions", np.nonzero(~rc.decided(gap, n))[0][:8])
            got, clamped = rc.kernel_choice(w, uc)
            assert not clamped, what
            np.testing.assert_array_equal(got, exact, err_msg=what)
            np.testing.assert_array_equal(oresample.choice(w, uc), exact, err_msg=what)


@pytest.mark.parametrize("n", rc.COUNTS)
def test_tied_offsets_stay_within_reach(n):
    for name, w in _cases(n):
        for u in rc.U_TIES:
            what = f"n={n} {name} u={u!r}"
            got, _ = rc.kernel_systematic(w, u)
            rc.check_against_exact(got, rc.exact_systematic(w, u, reach=True), n, what)
            rc.check_against_exact(np.minimum(oresample.systematic(w, u), n - 1), rc.exact_systematic(w, u, reach=True), n,
                                   what + " oracle")
            uj = rc.uniforms(n, u)
            got, _ = rc.kernel_stratified(w, uj)
            rc.check_against_exact(got, rc.exact_stratified(w, uj, reach=True), n, what + " stratified")
            got, _ = rc.kernel_choice(w, uj)
            rc.check_against_exact(got, rc.exact_choice(w, uj, reach=True), n, what + " choice")


def test_one_source_rule_fails_for_the_reference_itself():
    """Why check_against_exact is stated in cumulative weight and not as "within one index": two spikes at the ends, u = 0,
    n = 64.  Position 32 is exactly 1/2; the exact cumulative weights of sources 0 .. 62 lie within 1e-292 of 1/2, the
    first 31 of them below it.  In float64 all of them ARE 1/2, and np.searchsorted -- the reference -- returns 0."""
    name, w = [c for c in rc.CASES(64) if c[0] == "ends"][0]
    exact, gap, lo, hi = rc.exact_systematic(w, 0.0, reach=True)
    assert exact[32] == 31 and oresample.systematic(w, 0.0)[32] == 0 and (lo[32], hi[32]) == (0, 63)


def test_contested_outputs_are_named():
    """Where the segmented sum steps down by an ulp and a position ties with it, two threads write one output: the
    restatement says which outputs (the GPU test holds only those to the reach rule instead of bit for bit).  Decided
    offsets have none."""
    seen = 0
    for n in rc.COUNTS:
        for name, w in _cases(n):
            for u in rc.decided_offsets(name) + rc.U_TIES:
                idx, clamped, mask = rc.kernel_systematic(w, u, contested=True)
                assert not (mask.any() and u not in rc.U_TIES), (n, name, u)
                seen += int(mask.sum())
                if mask.any():
                    rc.check_against_exact(idx, rc.exact_systematic(w, u, reach=True), n, f"{n} {name} {u!r}")
    assert seen >= 1


def test_the_last_offset_reaches_the_clamp():
    """u = nextafter(1, 0): the last position rounds to 1.0 or beyond, and the float64 cumulative sum may end below it --
    np.searchsorted returns n (an IndexError in the reference), the kernels clamp and flag.  Some case must get there,
    or the GPU test's flag assertion would be vacuous."""
    hits = []
    for n in rc.COUNTS:
        for name, w in _cases(n):
            idx, clamped = rc.kernel_systematic(w, rc.LAST_U)
            if clamped:
                hits.append((n, name))
            assert idx.max() <= n - 1
    assert hits, "no designed case reaches the clamp"


def test_nan_weights_clamp_every_output():
    for n in (1, 65, 1000):
        for name, w in rc.CASES(n):
            if rc.has_nan(w):
                idx, clamped = rc.kernel_systematic(w, 0.5)
                assert clamped and (idx == n - 1).all(), (n, name)


def test_moments_reference():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((500, 6)) * [1, 1, 0.1, 0.2, 0.2, 0.01]
    w = rng.random(500)
    shift = np.array([5e5, 6.7e6, 400, 0.1, 0, 0])
    mean, var = rc.moments_reference(x, w, origin=np.zeros(6))
    np.testing.assert_allclose(mean.astype(float), np.average(x, weights=w, axis=0), rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(var.astype(float), np.average((x - mean.astype(float)) ** 2, weights=w, axis=0), rtol=1e-12)
    # the origin only moves the mean: exactly representable shifts leave the sums' terms what they were
    y = np.round(x * 2 ** 20) / 2 ** 20 + np.round(shift)
    mean1, var1 = rc.moments_reference(y, w, origin=np.round(shift))
    mean0, var0 = rc.moments_reference(y - np.round(shift), w, origin=np.zeros(6))
    np.testing.assert_array_equal(mean1, mean0)
    np.testing.assert_array_equal(var1, var0)
    # N copies of one particle: variance 0, mean the particle, wherever the origin is
    mean, var = rc.moments_reference(np.tile(shift + 0.3, (100, 1)), w[:100])
    assert (var == 0).all() and (mean == 0).all()
