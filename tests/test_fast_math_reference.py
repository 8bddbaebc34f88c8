"""The references of tests/fast_math_reference.py against each other, and the composition of its input sets (CPU).

The GPU tests (tests/test_gpu_fast_primitives.py) trust these references and these inputs; here each reference is checked
by an independent one, and each input set is shown to hold the edge classes it promises, inside the domain the code
claims its bound for.
"""
import decimal
import math
from fractions import Fraction

import numpy as np

from tests import fast_math_reference as fr


def relative_difference(ld, dec):
    """|ld / dec - 1| for longdouble values away from the ends of the double range: a longdouble is hi + lo, two doubles,
    exactly, and decimal holds their sum without rounding."""
    hi = ld.astype(np.float64)
    lo = (ld - hi.astype(fr.LD)).astype(np.float64)
    D = decimal.Decimal
    return np.array([float(abs(fr.DEC.divide(fr.DEC.subtract(fr.DEC.add(D(float(h)), D(float(l))), d), d)))
                     for h, l, d in zip(hi, lo, dec)])


def test_longdouble_carries_64_bits_and_agrees_with_decimal():
    fr.require_longdouble()
    rng = np.random.default_rng(1)
    x = np.concatenate((fr._log_uniform(rng, 2000, -900, 900), [1.0, 3.0, 2.0 - fr.EPS, 1.0 + fr.EPS]))
    for name, ref, dec in (("1/x", fr.ref_rcp(x), [fr.DEC.divide(decimal.Decimal(1), decimal.Decimal(float(v))) for v in x]),
                           ("sqrt", fr.ref_sqrt(x), [fr.DEC.sqrt(decimal.Decimal(float(v))) for v in x])):
        rel = relative_difference(ref, dec)
        print(f"{name}: longdouble against decimal, max relative difference {rel.max():.3g} (2^-64 = {2.0 ** -64:.3g})")
        assert rel.max() <= 2.0 ** -64
    # the ulp measure: a correctly rounded double is within half an ulp, its neighbours between a half and one and a half
    good = (1.0 / x)
    # (rounding the 64-bit reference to a double rounds twice: it misses the correctly rounded double in ~2^-11 of cases)
    assert fr.ulp_error(good, fr.ref_rcp(x)).max() <= 0.5
    assert fr.correctly_rounded_share(good, fr.ref_rcp(x)) > 1.0 - 2.0 ** -9
    off = np.nextafter(good, np.inf)
    e = fr.ulp_error(off, fr.ref_rcp(x))
    assert (e >= 0.5).all() and (e <= 1.5).all() and fr.correctly_rounded_share(off, fr.ref_rcp(x)) < 2.0 ** -9


def test_decimal_exp_agrees_with_longdouble_exp_and_the_table_with_exp2():
    x = -np.concatenate((np.linspace(0.0, 700.0, 1500), np.geomspace(1e-12, 700.0, 500)))  # (normal results)
    ref = fr.dec_exp(x)
    with np.errstate(under="ignore"):
        ld = np.exp(x.astype(fr.LD))
    rel = relative_difference(ld, ref)
    print(f"exp: decimal against longdouble, max relative difference {rel.max():.3g}")
    assert rel.max() < 2.0 ** -60  # (the C library's expl: a few ulp of a longdouble)
    assert fr.dec_relative_error(np.exp(x), ref).max() < 2.3e-16  # and the double exp is within an ulp of it
    tab = fr.dec_exp2_table()
    assert tab[0] == 1 and abs(tab[16] ** 2 - 2) < decimal.Decimal("1e-38")
    assert fr.dec_ulp_error(np.exp2(np.arange(32) / 32.0), tab).max() <= 1.0
    assert fr.LN2_32 == math.log(2.0) / 32.0


def test_fraction_fma_rounds_once():
    rng = np.random.default_rng(2)
    # products whose exact value lies beyond a double: fma differs from the two-rounding form, and equals the exact one
    a = 1.0 + rng.random(3000)
    b = 1.0 + rng.random(3000)
    c = -(a * b)
    got = np.array([fr.fma(p, q, r) for p, q, r in zip(a, b, c)])
    want = np.array([float(Fraction(p) * Fraction(q) + Fraction(r)) for p, q, r in zip(a.tolist(), b.tolist(), c.tolist())])
    # (the results are the rounding errors of a * b)
    assert (got == want).all() and (got != 0.0).mean() > 0.9 and (np.abs(got) <= 2.0 ** -52).all()
    assert ((a * b + c) == 0.0).all()
    if hasattr(math, "fma"):
        x = rng.standard_normal((5000, 3)) * np.exp(rng.uniform(-30, 30, (5000, 3)))
        assert all(fr.fma(p, q, r) == math.fma(p, q, r) for p, q, r in x.tolist())
    # signs of an exact zero
    assert math.copysign(1.0, fr.fma(1.5, 2.0, -3.0)) == 1.0 and math.copysign(1.0, fr.fma(-0.0, 2.0, -0.0)) == -1.0
    assert math.copysign(1.0, fr.fma(0.0, 2.0, -0.0)) == 1.0 and math.copysign(1.0, fr.fma(0.0, 5.0, 7.0)) == 1.0
    # int / int is the IEEE quotient of the two integers
    k, n = rng.integers(0, 65537, 5000), rng.integers(1, 65537, 5000)
    assert (fr.count_fraction_expected(k, n) == np.array([int(p) / int(q) for p, q in zip(k, n)])).all()
    # the expected counts on a case worked by hand: n = 4, total 1: ck * 4 - u = 0.5, 1.5, 3.0, 3.5 -> 1, 2, 4, 4
    got = fr.count_le_expected(np.array([0.25, 0.5, 0.875, 1.0]), np.full(4, 4.0), np.full(4, 0.5), np.full(4, 4.0))
    assert got.tolist() == [1.0, 2.0, 4.0, 4.0]
    # the bilinear interpolant at the corners and the centre of a cell
    z = [np.full(5, v) for v in (1.0, 3.0, 5.0, 11.0)]
    got = fr.bilinear_expected(*z, np.array([0.0, 1.0, 0.0, 1.0, 0.5]), np.array([0.0, 0.0, 1.0, 1.0, 0.5]))
    assert got.tolist() == [1.0, 3.0, 5.0, 11.0, 5.0]


def test_rcp_and_sqrt_inputs_hold_their_edge_classes_inside_the_domain():
    tiny, huge = 2.0 ** -1022, 2.0 ** 1022
    sets = fr.rcp_inputs()
    x = np.concatenate(list(sets.values()))
    assert len(x) % 256 != 0 and len(x) >= 1 << 20
    assert (np.abs(x) >= tiny).all() and (np.abs(x) <= huge).all() and (np.abs(1.0 / x) >= tiny).all()  # x and 1/x normal
    assert len(sets["log-uniform"]) / len(x) > 0.9 and 0.45 < (sets["log-uniform"] < 0).mean() < 0.55
    e = np.frexp(np.abs(sets["log-uniform"]))[1]
    assert e.min() <= -1015 and e.max() >= 1015 and len(np.unique(e)) > 2000  # the whole exponent range
    p2 = sets["powers of two"]
    assert len(p2) == 2 * 2045 and (np.frexp(p2)[0] == 0.5 * np.sign(p2)).all()
    near = sets["1 +- k eps, 2 - k eps"]
    for v in (1.0 + fr.EPS, 1.0 - fr.EPS / 2, 2.0 - fr.EPS, 1.0 + 64 * fr.EPS, -(2.0 - 64 * fr.EPS),
              (2.0 - fr.EPS) * 2.0 ** -1021):
        assert v in near
    assert len(near) == 2 * 5 * 193
    assert sets["depths"].min() == 0.1 and np.isclose(sets["depths"].max(), 1e5)
    assert np.isclose(sets["cell sizes"].min(), 1e-3) and np.isclose(sets["cell sizes"].max(), 1e3)
    assert np.isclose(sets["2 zs^2"].min(), 2e-12) and np.isclose(sets["2 zs^2"].max(), 2e6)
    assert all(len(sets[k]) == 8192 for k in ("depths", "focal lengths", "cell sizes", "2 zs^2"))

    sets = fr.sqrt_inputs()
    x = np.concatenate(list(sets.values()))
    assert len(x) % 256 != 0 and (x >= tiny).all() and np.isfinite(x).all()  # normal and positive
    assert len(sets["log-uniform"]) / len(x) > 0.85
    e = np.frexp(sets["log-uniform"])[1]
    assert e.min() <= -1015 and e.max() >= 1018 and (e % 2 == 0).mean() > 0.45 and (e % 2 == 1).mean() > 0.45
    assert len(sets["powers of two"]) == 2046
    sq = sets["perfect squares"]
    r = fr.perfect_square_roots(sq)
    assert len(sq) > 120000 and (r * r == sq).all() and r.min() < 1e-60 and r.max() > 1e60 and float(1 << 52) in sq
    assert (np.frexp(r)[0] != 0.5).mean() > 0.99  # not merely powers of two
    d = sets["dx^2 + dy^2"]
    assert d.min() < 1e-17 and d.max() > 1e6 and len(d) == 8192


def test_the_other_input_sets_hold_their_edge_classes():
    sets = fr.minmax_inputs()
    a, b = (np.concatenate([sets[k][i] for k in sets]) for i in (0, 1))
    assert len(a) % 256 != 0 and not np.isnan(a).any() and not np.isnan(b).any()
    assert (a == b).mean() > 0.05 and (a < b).mean() > 0.3 and (a > b).mean() > 0.3
    sa, sb = sets["special"]
    for v in (np.inf, -np.inf, 5e-324, -5e-324):
        assert ((sa == v) & (sb == 1.0)).any() and ((sa == 1.0) & (sb == v)).any() and ((sa == v) & (sb == v)).any()
    za, zb = sets["zeros"]
    assert np.signbit(za).tolist() == [False, True] and np.signbit(zb).tolist() == [True, False]

    sets = fr.exp_inputs()
    x = np.concatenate(list(sets.values()))
    assert (x <= 0.0).all() and all(len(c) <= 20000 for c in fr.chunks(x))
    assert len(sets["0 .. -50 dense"]) == 20001 and len(sets["1e-12 .. 745 geometric"]) == 5000
    m = sets["multiples of ln2/32"]
    j = np.rint(m * (32.0 / math.log(2.0)))
    n_multiples = int(746.6 / fr.LN2_32)
    assert len(m) == 3 * n_multiples and set(np.unique(-j).astype(int)) == set(range(1, n_multiples + 1))
    assert sets["-745.2 .. -746.5"].max() == -745.2 and abs(sets["-745.2 .. -746.5"].min() + 746.5) < 1e-9
    h = sets["half multiples"] * (32.0 / math.log(2.0))
    assert np.abs(np.abs(h - np.rint(h)) - 0.5).max() < 1e-9 or (np.abs(h - np.floor(h) - 0.5) < 1e-9).all()

    sets = fr.count_fraction_inputs()
    k, n = (np.concatenate([sets[key][i] for key in sets]) for i in (0, 1))
    assert len(k) % 256 != 0 and (k >= 0).all() and (k <= n).all() and n.min() == 1 and n.max() == 65536
    rk, rn = sets["random"]
    assert len(rk) >= 1 << 20 and (rk == rn).any() and (rk == 0).any()
    for nn in (1, 2, 3, 961, 3969, 65535, 65536):
        assert sets[f"every k of n = {nn}"][0].tolist() == list(range(nn + 1))

    ck, scale, u, n = fr.count_le_inputs()
    assert len(ck) == 9 * (70 + 513 + 5000) and len(ck) % 256 != 0 and set(n.tolist()) == {70.0, 513.0, 5000.0}
    assert (u == 0.0).any() and (u < 1.0).all() and np.isfinite(ck * scale).all()
    want = fr.count_le_expected(ck, scale, u, n)
    assert want.min() >= 0 and (want == n).any() and len(np.unique(want)) > 1000

    z00, z10, z01, z11, tx, ty = fr.bilinear_inputs()
    assert len(tx) % 256 != 0 and (tx == 0).any() and (tx == 1).any() and (ty == 0).any() and (ty == 1).any()
    assert ((tx == 0) & (ty == 1)).any() and tx.min() >= 0 and tx.max() <= 1
    for z in (z00, z10, z01, z11):
        assert 1.0 <= np.abs(z[2000:]).min() and np.abs(z).max() <= 1e4 + 10


def test_projection_reference_reproduces_the_goldens_and_its_cameras_cover_every_term(golden):
    g = golden("g1_projection.npz")
    for cam, xyz, uv, R in zip(g["cams"], g["xyz"], g["uv"], g["R"]):
        np.testing.assert_allclose(fr.rotation(cam[3:6]), R, rtol=0, atol=2.3e-16)
        ref = fr.project_reference(cam, xyz).astype(np.float64)
        assert np.array_equal(np.isnan(ref), np.isnan(uv))
        ok = ~np.isnan(uv[:, 0])
        np.testing.assert_allclose(ref[ok], uv[ok], rtol=1e-13, atol=1e-9)
    cams = fr.projection_cameras()
    assert [name for name, (_, simple) in cams.items() if simple] == ["pinhole", "k1..k3"]
    for name, (cam, simple) in cams.items():
        assert fr.simple_form_accepts(cam) == simple, name
        xyz = fr.projection_points(cam)
        ref = fr.project_reference(cam, xyz).astype(np.float64)
        assert len(xyz) % 256 != 0 and len(xyz) > 10000
        if cam[23] != 0.0:
            assert np.isfinite(ref).all() and ref.min() < 0 and (ref.max(axis=0) > cam[6:8]).all()
            continue
        behind = np.isnan(ref[:, 0])
        assert 0.07 < behind.mean() < 0.1 and np.array_equal(behind, np.isnan(ref[:, 1]))
        inside = (ref[~behind] >= 0).all(axis=1) & (ref[~behind] <= cam[6:8]).all(axis=1)
        assert inside.mean() > 0.7, name
    assert cams["k4..k6"][0][15:18].all() and cams["tangential"][0][18:20].all()
    assert cams["elevation correction"][0][20] == 1.0
    assert sum(fr.simple_form_accepts(c) for c in g["cams"]) >= 2
