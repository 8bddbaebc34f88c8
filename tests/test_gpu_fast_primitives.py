"""The primitives of the fast arithmetic (GLH_MATH_FAST) as the device computes them, each against a reference of higher
precision (tests/fast_math_reference.py), through `glh_stage_fast_math` and `glh_stage_project_fast`: kernels that call
the functions of csrc/glh_math.h and glh_kernels.h themselves, compiled with the library's flags.

tests/test_hostcheck.py compiles the same header for the CPU, where `rcp_nr` is `1.0 / x`, `sqrt_nr` is `sqrt`, `min_nn`
and `max_nn` are ternaries and the table of `exp_fast` comes from the C library; the fused-against-staged tests compare two
callers of the same functions.  Here the Newton and Goldschmidt sequences, the inline assembly, the device-made table and
the device's fused multiply-add are what is measured.  The bounds are the code's own claims (csrc/glh_math.h); every
test prints its measured maximum and the share of correctly rounded results before it asserts.  INPUTS.md ("Fast arithmetic:
the primitives") records the figures of an MI355X and what comes back outside the stated domains.
"""
import decimal

import numpy as np
import pytest

from tests import fast_math_reference as fr

pytestmark = pytest.mark.gpu


def fm(op, *cols):
    from glimpse_amd import _lib

    return _lib.stage_fast_math(op, *cols)


def report(what, err, got, ref, unit="ulp"):
    share = 100 * fr.correctly_rounded_share(got, ref)
    print(f"{what}: max {err.max():.4g} {unit} over {len(err)} rows, correctly rounded {share:.3f} %")


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


# ---- rcp_nr, sqrt_nr -------------------------------------------------------------------------------------------------
def test_rcp_nr_is_within_an_ulp_where_x_and_its_reciprocal_are_normal():
    fr.require_longdouble()
    sets = fr.rcp_inputs()
    x = np.concatenate(list(sets.values()))
    got = fm("RCP", x)
    ref = fr.ref_rcp(x)
    err = fr.ulp_error(got, ref)
    at = 0
    for name, v in sets.items():
        report(f"rcp_nr, {name}", err[at:at + len(v)], got[at:at + len(v)], ref[at:at + len(v)])
        at += len(v)
    report("rcp_nr, all", err, got, ref)
    assert np.isfinite(got).all()
    assert err.max() <= 1.0
    p2 = sets["powers of two"]
    assert np.array_equal(bits(fm("RCP", p2)), bits(1.0 / p2))  # exact on powers of two


def test_sqrt_nr_is_within_an_ulp_for_normal_x_and_exact_on_squares():
    fr.require_longdouble()
    sets = fr.sqrt_inputs()
    x = np.concatenate(list(sets.values()))
    got = fm("SQRT", x)
    ref = fr.ref_sqrt(x)
    err = fr.ulp_error(got, ref)
    at = 0
    for name, v in sets.items():
        report(f"sqrt_nr, {name}", err[at:at + len(v)], got[at:at + len(v)], ref[at:at + len(v)])
        at += len(v)
    report("sqrt_nr, all", err, got, ref)
    assert np.isfinite(got).all()
    assert err.max() <= 1.0
    sq = sets["perfect squares"]
    roots = fm("SQRT", sq)
    print(f"sqrt_nr, perfect squares: {int((roots != fr.perfect_square_roots(sq)).sum())} of {len(sq)} roots inexact")
    assert np.array_equal(bits(roots), bits(fr.perfect_square_roots(sq)))
    # what the code promises beside the bound: 0 -> 0 and NaN -> NaN
    edge = fm("SQRT", np.array([0.0, np.nan]))
    assert bits(edge[:1])[0] == 0 and np.isnan(edge[1])


def test_outside_the_stated_domains():
    """What rcp_nr and sqrt_nr return outside their domains, printed for the table of INPUTS.md.  Asserted: only what a
    caller relies on -- project_simple_fast takes rcp_nr of a depth that may be zero, negative or NaN and discards the result
    by a select (nothing to assert: any value will do, and none may trap -- the call returns); the tangent models take
    sqrt_nr(dx^2 + dy^2) of a displacement that may be exactly 0 or NaN (asserted with sqrt_nr's own test).  The rest
    is a record: rows "reachable" in INPUTS.md say which call site can see the class."""
    sub = 2.0 ** -1040
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, sub, -sub, 2.0 ** -1023, 1e-320, 2e-320, 2.0 ** 1023,
                  1.5 * 2.0 ** 1023, 1.7976931348623157e308, 2.0 ** 1022 * 1.5])
    got = fm("RCP", x)
    with np.errstate(all="ignore"):
        ieee = 1.0 / x
    for v, g, w in zip(x, got, ieee):
        print(f"rcp_nr({v!r}) = {g!r}   (IEEE 1 / x: {w!r})")
    x = np.array([-0.0, np.inf, -np.inf, -1.0, -1e-300, 5e-324, sub, 2.0 ** -1023, 1e-320, 2.0 ** -1022 * 0.75])
    got = fm("SQRT", x)
    with np.errstate(all="ignore"):
        ieee = np.sqrt(x)
    for v, g, w in zip(x, got, ieee):
        print(f"sqrt_nr({v!r}) = {g!r}   (IEEE sqrt: {w!r})")
    # subnormal x in bulk: the worst error, for the record
    rng = np.random.default_rng(31)
    s = np.ldexp(1.0 + rng.random(20011), rng.integers(-1074, -1022, 20011).astype(np.int32))
    s = s[s > 0]
    g = fm("SQRT", s)
    bad = ~np.isfinite(g)
    print(f"sqrt_nr, subnormal x: {int(bad.sum())} of {len(s)} not finite; of the finite, max "
          f"{fr.ulp_error(g[~bad], fr.ref_sqrt(s[~bad])).max() if (~bad).any() else float('nan'):.4g} ulp")
    big = np.ldexp(1.0 + rng.random(20011), rng.integers(1022, 1024, 20011).astype(np.int32))  # 1 / x subnormal
    g = fm("RCP", big)
    print(f"rcp_nr, subnormal result: {int((~np.isfinite(g)).sum())} of {len(big)} not finite, max |got - 1 / x| "
          f"{np.abs(g - 1.0 / big).max() / 5e-324:.4g} subnormal steps")
    # a caller relies on: the hook returns for every such input (no trap), and nothing finite appears for a NaN
    assert np.isnan(fm("RCP", np.array([np.nan]))[0])


# ---- min_nn, max_nn --------------------------------------------------------------------------------------------------
def test_min_nn_and_max_nn_are_the_ieee_minimum_and_maximum_and_return_the_number_beside_a_nan():
    sets = fr.minmax_inputs()
    a, b = (np.concatenate([sets[k][i] for k in sets]) for i in (0, 1))
    lo, hi = fm("MIN_NN", a, b), fm("MAX_NN", a, b)
    n_lo, n_hi = int((lo != np.minimum(a, b)).sum()), int((hi != np.maximum(a, b)).sum())
    print(f"min_nn: {n_lo} of {len(a)} pairs differ from np.minimum; max_nn: {n_hi} differ from np.maximum")
    za, zb = sets["zeros"]
    zl, zh = fm("MIN_NN", za, zb), fm("MAX_NN", za, zb)
    for i in range(2):
        print(f"min_nn({za[i]!r}, {zb[i]!r}) = {zl[i]!r}; max_nn = {zh[i]!r}")  # (the sign of zero: printed, not asserted)
    assert n_lo == 0 and n_hi == 0
    # every result is one of its operands, bit for bit (but for the zero pairs, where == cannot tell)
    nz = (a != 0) | (b != 0)
    assert (((bits(lo) == bits(a)) | (bits(lo) == bits(b))) | ~nz).all()
    assert (((bits(hi) == bits(a)) | (bits(hi) == bits(b))) | ~nz).all()
    # one NaN operand, either position: the number comes back (count_le_fast and spline_cell_offset rely on it)
    num = np.array([0.0, -0.0, 1.0, -1.0, 5e-324, 1e300, -1e300, np.inf, -np.inf, 5000.0])
    nan = np.full(len(num), np.nan)
    for op in ("MIN_NN", "MAX_NN"):
        first, second = fm(op, nan, num), fm(op, num, nan)
        print(f"{op}(NaN, x) = {first.tolist()}; {op}(x, NaN) = {second.tolist()}")
        assert np.array_equal(bits(first), bits(num)) and np.array_equal(bits(second), bits(num))
        assert np.isnan(fm(op, nan[:1], nan[:1])[0])  # (both NaN: nothing else to return)


# ---- exp_fast, weight_of ---------------------------------------------------------------------------------------------
EXP_ARGUMENTS = np.concatenate(list(fr.exp_inputs().values()))
EXP_CHUNKS = fr.chunks(EXP_ARGUMENTS)


@pytest.fixture(scope="module")
def exp_on_device():
    """exp_fast of the whole argument set in one launch (the chunks below only split the decimal reference)."""
    return fm("EXP", EXP_ARGUMENTS)


@pytest.mark.parametrize("chunk", range(len(EXP_CHUNKS)))
def test_exp_fast_against_decimal(exp_on_device, chunk):
    x = EXP_CHUNKS[chunk]
    assert len(x) <= 20000
    got = exp_on_device[chunk * 20000: chunk * 20000 + len(x)]
    ref = fr.dec_exp(x)
    ok = np.array([r > decimal.Decimal("1e-290") for r in ref])
    rel = np.append(fr.dec_relative_error(got[ok], [r for r, o in zip(ref, ok) if o]), 0.0)
    correct = int((got[ok] == np.array([float(r) for r, o in zip(ref, ok) if o])).sum())
    print(f"exp_fast, arguments {x.max():.6g} .. {x.min():.6g}: max relative error {rel.max():.4g} over {int(ok.sum())} "
          f"rows ({correct} correctly rounded); {int((~ok).sum())} rows below 1e-290, largest "
          f"{np.append(got[~ok], 0.0).max():.4g}")
    assert rel.max() <= 4e-15
    assert (got[~ok] >= 0).all() and (got[~ok] < 2e-290).all()


def test_exp_fast_of_positive_arguments_and_its_table():
    pos = np.array([1e-9, 0.5, 3.0])
    rel = fr.dec_relative_error(fm("EXP", pos), fr.dec_exp(pos))
    print(f"exp_fast(1e-9, 0.5, 3): relative errors {rel.tolist()}")
    assert rel.max() <= 4e-15
    # The 32 table entries, read through exp_fast at x = RN(j ln2 / 32): rint(x 32 / ln2) = j, the remainder |r| is the
    # rounding error of x (<= 2^-54), the polynomial rounds to 1.0 exactly (|r| < 2^-53) and the scaling is by 2^0: the
    # result is T[j] itself.
    j = np.arange(32)
    ln2_32 = fr.DEC.divide(fr.DEC.ln(decimal.Decimal(2)), decimal.Decimal(32))
    x = np.array([float(fr.DEC.multiply(decimal.Decimal(int(v)), ln2_32)) for v in j])
    table = fm("EXP", x)
    err = fr.dec_ulp_error(table, fr.dec_exp2_table())
    print(f"exp table (device exp2): max {err.max():.4g} ulp of 2^(j/32), {int((err <= 0.5).sum())} of 32 correctly rounded")
    assert table[0] == 1.0 and err.max() <= 1.0


def test_weight_of_clamps_and_floors():
    ll = np.concatenate((np.linspace(0.0, 700.0, 1999), [746.0, 746.5, 750.0, 800.0, 1e6, 1e300, np.inf, np.nan]))
    got = fm("WEIGHT", ll)
    n = 1999
    ref = [fr.DEC.add(r, decimal.Decimal(1e-300)) for r in fr.dec_exp(-ll[:n])]
    rel = fr.dec_relative_error(got[:n], ref)
    print(f"weight_of, ll 0 .. 700: max relative error {rel.max():.4g}")
    assert rel.max() <= 4e-15
    print(f"weight_of{ll[n:].tolist()} = {got[n:].tolist()}")
    assert (got[n:-1] == 1e-300).all()  # ll >= 746, 1e6, +inf: the floor weight exactly
    assert np.isnan(got[-1])
    between = fm("WEIGHT", np.linspace(745.0, 746.0, 101))  # the exponential's last subnormals: the floor, within rounding
    assert (between >= 1e-300).all() and (between <= 1e-300 * (1 + 1e-15)).all()


# ---- the IEEE-exact pieces: bit for bit ------------------------------------------------------------------------------
def test_count_fraction_is_the_ieee_quotient_on_the_device():
    sets = fr.count_fraction_inputs()
    k, n = (np.concatenate([sets[key][i] for key in sets]) for i in (0, 1))
    got = fm("COUNT_FRACTION", k.astype(np.float64), n.astype(np.float64))
    want = fr.count_fraction_expected(k, n)
    differ = int((bits(got) != bits(want)).sum())
    print(f"count_fraction: {differ} of {len(k)} pairs differ from k / n")
    assert differ == 0


def test_count_le_fast_is_the_clipped_floor_of_one_fused_operation():
    ck, scale, u, n = fr.count_le_inputs()
    got = fm("COUNT_LE", ck, scale, u, n)
    want = fr.count_le_expected(ck, scale, u, n)
    differ = int((got != want).sum())
    print(f"count_le_fast: {differ} of {len(ck)} rows differ; counts {int(want.min())} .. {int(want.max())}")
    assert differ == 0
    # a NaN cumulative weight gives 0; a product far above n gives n; one far below gives 0
    edge = fm("COUNT_LE", np.array([np.nan, 1e300, np.inf, 3.0, -1e300, 0.0]), np.array([1.0, 1e5, 1.0, 1e9, 1.0, 1.0]),
              np.array([0.5, 0.5, 0.5, 0.25, 0.5, 0.75]), np.full(6, 5000.0))
    print(f"count_le_fast, edges: {edge.tolist()}")
    assert edge.tolist() == [0.0, 5000.0, 5000.0, 5000.0, 0.0, 0.0]


def test_raster_bilinear_fast_is_three_fused_operations():
    cols = fr.bilinear_inputs()
    got = fm("BILINEAR", *cols)
    want = fr.bilinear_expected(*cols)
    differ = int((bits(got) != bits(want)).sum())
    print(f"raster_bilinear_fast: {differ} of {len(got)} rows differ from the three fused operations")
    assert differ == 0


# ---- the projection --------------------------------------------------------------------------------------------------
def projection_cases(golden):
    g = golden("g1_projection.npz")
    cases = [(f"g1 camera {i}", cam, xyz, False) for i, (cam, xyz) in enumerate(zip(g["cams"], g["xyz"]))]
    cases += [(name, cam, fr.projection_points(cam), False) for name, (cam, _) in fr.projection_cameras().items()]
    # ray directions (the general form takes them, as glh_stage_project_directions does): no camera offset, no correction
    for name in ("k1..k3", "elevation correction"):
        cam = fr.projection_cameras()[name][0]
        cases.append((name + ", ray directions", cam, fr.projection_points(cam) - cam[0:3], True))
    return cases


def test_project_fast_stays_within_four_times_the_exact_kernel_s_error(golden):
    """Reference: the projection formula in longdouble.  The exact kernel (glh_stage_project, pinned to the reference project
    by g1 / g14) sets the scale: on the same inputs its worst error against that reference is measured, and the fast path
    is granted 4 x that plus 2 ulp of the largest |u|, |v| -- each of its operations is within an ulp like the exact
    one, and every quotient gains one rounding from the reciprocal."""
    from glimpse_amd import _lib

    fr.require_longdouble()
    for name, cam, xyz, directions in projection_cases(golden):
        ref = fr.project_reference(cam, xyz, directions)
        exact = _lib.stage_project(cam, xyz, directions=directions)
        fast = _lib.stage_project_fast(cam, xyz, directions=directions)
        behind = np.isnan(ref[:, 0].astype(np.float64))
        for what, got in (("exact", exact), ("fast", fast)):  # NaN for both coordinates, exactly as glh_stage_project
            assert np.array_equal(np.isnan(got[:, 0]), behind) and np.array_equal(np.isnan(got[:, 1]), behind), (name, what)
        ok = ~behind
        e_exact = np.abs(exact[ok].astype(fr.LD) - ref[ok]).max().astype(np.float64)
        e_fast = np.abs(fast[ok].astype(fr.LD) - ref[ok]).max().astype(np.float64)
        largest = float(np.abs(ref[ok]).max())
        allowed = 4.0 * e_exact + 2.0 * np.spacing(largest)
        print(f"projection, {name}: {int(ok.sum())} points in front, {int(behind.sum())} behind; worst error exact "
              f"{e_exact:.4g}, fast {e_fast:.4g}, allowed {allowed:.4g} px (largest |uv| {largest:.4g}, its ulp "
              f"{np.spacing(largest):.3g})")
        assert e_fast <= allowed, name


def test_project_simple_fast_is_project_fast_bit_for_bit(golden):
    from glimpse_amd import _lib

    accepted = 0
    for name, cam, xyz, directions in projection_cases(golden):
        if directions or not fr.simple_form_accepts(cam):
            with pytest.raises(_lib.GlhError) as info:
                _lib.stage_project_fast(cam, xyz, directions=directions, simple=True)
            assert info.value.code == -1 and "CAM_F_NOT_SIMPLE" in str(info.value), name
            continue
        accepted += 1
        general, simple = _lib.stage_project_fast(cam, xyz), _lib.stage_project_fast(cam, xyz, simple=True)
        differ = int((bits(general) != bits(simple)).any(axis=1).sum())
        print(f"project_simple_fast, {name}: {differ} of {len(xyz)} points differ from project_fast")
        assert differ == 0, name
    assert accepted >= 4


# ---- the one out-of-domain class an API call can reach ---------------------------------------------------------------
def test_fast_arithmetic_refuses_a_dem_sigma_outside_the_reciprocal_s_domain():
    """dem_log_likelihood<true> scales the DEM term of a point with a gridded surface by rcp_nr(2 zs^2).  For a non-zero zs
    below 1.06e-154 (2 zs^2 subnormal or rounded to 0) or above 9.4e153 (2 zs^2 infinite) rcp_nr returns NaN (printed
    below, as measured) where the exact arithmetic's division gives inf or 0 and the particle the floor weight.  Nothing
    is added to the particle loops for it: the library notices such a value where it is set -- the constant beside a dem
    raster in glh_set_motion, a node of the dem_sigma raster in glh_set_raster -- and glh_update_weights, glh_step and
    glh_track refuse to run FAST arithmetic on it (GLH_E_UNSUPPORTED, before any kernel).  Exact arithmetic, a constant
    sigma beside a constant dem (an IEEE division in both arithmetics), 0 and NaN are not refused."""
    import ctypes as C

    import glimpse_amd
    from glimpse_amd import _lib

    zs = np.array([1e-160, 1e-170, 1.0e-154, 1e154, 1.06e-154, 9.4e153])
    with np.errstate(all="ignore"):
        scale = 2.0 * (zs * zs)
        print(f"rcp_nr(2 zs^2) for zs = {zs.tolist()}: {fm('RCP', scale).tolist()}; IEEE: {(1.0 / scale).tolist()}")
    assert np.isfinite(fm("RCP", scale[4:])).all()  # the two ends of the accepted range are inside rcp_nr's domain

    lib = _lib.load()
    UNSUPPORTED = -5
    lim = (-40.0, 40.0)
    dem = glimpse_amd.Raster(np.zeros((4, 5)), x=lim, y=lim)

    def outcome(ctx, sigma=0.0, dem_raster=False, node=None, math="fast", kind=0):
        """The return codes of the three entry points (called with null arrays: an accepted sigma ends in GLH_E_INVALID)."""
        ctx.begin_sequence(1, 64, (15, 15))
        params = np.zeros((1, _lib.MOTION_FULL_LEN))
        params[0, 17], params[0, 18] = sigma, kind
        ctx.set_raster(_lib.RASTER_DEM, dem if dem_raster else None)
        params[0, 20] = float(dem_raster)
        z = np.full((4, 5), 0.3)
        z[2, 3] = 0.3 if node is None else node
        ctx.set_raster(_lib.RASTER_DEM_SIGMA, None if node is None else glimpse_amd.Raster(z, x=lim, y=lim))
        params[0, 21] = float(node is not None)
        ctx.set_motion(params)
        ctx.set_math(math)
        rcs = []
        for call in (lambda: lib.glh_update_weights(ctx.handle, None),
                     lambda: lib.glh_step(ctx.handle, 1, 1.0, None, _lib.RNG_PHILOX, None, None, 0),
                     lambda: lib.glh_track(ctx.handle, 1, None, None, None, 0)):
            rc = call()
            rcs.append((rc, "dem_sigma" in lib.glh_last_error().decode()))
        return rcs

    refused, accepted = [(UNSUPPORTED, True)] * 3, [(-1, False)] * 3
    with _lib.Context(1, 64, 1, max_search_dim=64, max_frames=2) as ctx:
        for bad in (1e-160, -1e-160, 1e-170, 1.0e-154, 1e154, np.inf):
            assert outcome(ctx, sigma=bad, dem_raster=True) == refused, bad
            assert outcome(ctx, node=bad) == refused, bad
            assert outcome(ctx, sigma=bad, dem_raster=True, math="exact") == accepted, bad
            assert outcome(ctx, node=bad, math="exact") == accepted, bad
            assert outcome(ctx, sigma=bad) == accepted, bad  # constant dem and sigma: an IEEE division in either arithmetic
            assert outcome(ctx, sigma=bad, dem_raster=True, kind=2) == accepted, bad  # a tangent model has no DEM term
        for good in (0.0, 1.06e-154, 0.3, 9.4e153, np.nan):
            assert outcome(ctx, sigma=good, dem_raster=True) == accepted, good
            assert outcome(ctx, node=good) == accepted, good


# ---- argument errors -------------------------------------------------------------------------------------------------
def test_argument_errors_need_no_kernel():
    from glimpse_amd import _lib

    lib = _lib.load()
    INVALID = -1
    args, out = np.ones((3, _lib.FM_ARGS)), np.full(3, -7.0)
    p = _lib._ptr
    assert lib.glh_stage_fast_math(0, 0, None, 3, p(out)) == INVALID and "bad argument" in lib.glh_last_error().decode()
    assert lib.glh_stage_fast_math(0, 0, p(args), 3, None) == INVALID
    assert lib.glh_stage_fast_math(0, 0, p(args), 0, p(out)) == INVALID
    assert lib.glh_stage_fast_math(0, 0, p(args), -5, p(out)) == INVALID
    for op in (-1, 9, 1000):
        assert lib.glh_stage_fast_math(0, op, p(args), 3, p(out)) == INVALID and "GLH_FM_" in lib.glh_last_error().decode()
    assert (out == -7.0).all()
    assert sorted(code for code, _ in _lib.FM_OPS.values()) == list(range(9))
    with pytest.raises(ValueError):
        _lib.stage_fast_math("RCP", np.ones(3), np.ones(3))
    with pytest.raises(ValueError):
        _lib.stage_fast_math("MIN_NN", np.ones(3), np.ones(4))

    cam = fr.projection_cameras()["pinhole"][0]
    grid = fr.projection_cameras()["raster grid"][0]
    xyz, uv = np.ones((3, 3)), np.full((3, 2), -7.0)
    assert lib.glh_stage_project_fast(0, None, p(xyz), 3, 0, 0, p(uv)) == INVALID
    assert lib.glh_stage_project_fast(0, p(cam), None, 3, 0, 0, p(uv)) == INVALID
    assert lib.glh_stage_project_fast(0, p(cam), p(xyz), 3, 0, 0, None) == INVALID
    assert lib.glh_stage_project_fast(0, p(cam), p(xyz), 0, 0, 0, p(uv)) == INVALID
    assert lib.glh_stage_project_fast(0, p(grid), p(xyz), 3, 1, 0, p(uv)) == INVALID
    assert "raster grid" in lib.glh_last_error().decode()
    assert lib.glh_stage_project_fast(0, p(grid), p(xyz), 3, 0, 1, p(uv)) == INVALID
    assert "CAM_F_NOT_SIMPLE" in lib.glh_last_error().decode()
    assert lib.glh_stage_project_fast(0, p(cam), p(xyz), 3, 1, 1, p(uv)) == INVALID
    assert (uv == -7.0).all()
    assert lib.glh_stage_fast_math(0, 0, p(args), 3, p(out)) == 0 and (out == 1.0).all()  # and the valid call works
