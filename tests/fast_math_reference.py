"""References and input sets for the primitives of the fast arithmetic (GLH_MATH_FAST; csrc/glh_math.h, glh_kernels.h).

Used by tests/test_fast_math_reference.py (CPU: the references against each other, the input sets' composition) and by
tests/test_gpu_fast_primitives.py (the device's answers against them).  Nothing here is a restatement of the code under
test where a higher precision is available:

* `1 / x`, `sqrt(x)` and the projection: `numpy.longdouble` with a 64-bit significand (asserted: `require_longdouble`),
  so a reference value is within 2^-11 ulp of a double of the true one;
* `exp(x)`, `2^(j/32)`: the standard library's `decimal` at 40 digits;
* the pieces that are IEEE-exact by construction (`count_fraction`, the count of `count_le_fast`, the three fused
  operations of `raster_bilinear_fast`): the same operations with ONE rounding each, from `fractions.Fraction`
  (`float(Fraction)` is `int / int`, correctly rounded) -- compared bit for bit.

Errors are in ulp of the correctly rounded double: |got - ref| / spacing(|ref rounded to double|).
"""
import decimal
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
DEC = decimal.Context(prec=40)
EPS = 2.0 ** -52
LN2_32 = float(DEC.divide(DEC.ln(decimal.Decimal(2)), decimal.Decimal(32)))  # ln 2 / 32, correctly rounded


def require_longdouble():
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble has no 64-bit significand here: no reference for 1/x and sqrt"


# ---- errors ----------------------------------------------------------------------------------------------------------
def ulp_error(got, ref):
    """|got - ref| in ulp of ref rounded to double; `ref` longdouble, `got` float64 (finite, ref != 0)."""
    ref = np.asarray(ref, dtype=LD)
    rounded = ref.astype(np.float64)
    difference = np.abs(np.asarray(got, dtype=np.float64).astype(LD) - ref)
    return (difference / np.spacing(np.abs(rounded)).astype(LD)).astype(np.float64)


def correctly_rounded_share(got, ref):
    """The share of `got` equal to `ref` rounded to double (which, rounded twice, is the correctly rounded double except
    where the 64-bit value lies within 2^-11 ulp of a tie: about one case in 2000)."""
    return float(np.mean(np.asarray(got, dtype=np.float64) == np.asarray(ref, dtype=LD).astype(np.float64)))


def ref_rcp(x):
    return LD(1) / np.asarray(x, dtype=np.float64).astype(LD)


def ref_sqrt(x):
    return np.sqrt(np.asarray(x, dtype=np.float64).astype(LD))


def dec_exp(x):
    """[Decimal] exp(x) at 40 digits for float64 x (each converted exactly)."""
    return [DEC.exp(decimal.Decimal(float(v))) for v in np.asarray(x, dtype=np.float64)]


def dec_relative_error(got, ref):
    """|got / ref - 1| as float64, for float64 got (converted exactly) against [Decimal] ref (all non-zero)."""
    return np.array([float(abs(DEC.divide(DEC.subtract(decimal.Decimal(float(g)), r), r))) for g, r in zip(got, ref)])


def dec_ulp_error(got, ref):
    """|got - ref| in ulp of ref rounded to double, ref [Decimal]."""
    return np.array([float(abs(DEC.subtract(decimal.Decimal(float(g)), r))) / float(np.spacing(abs(float(r))))
                     for g, r in zip(got, ref)])


def dec_exp2_table():
    """[Decimal] 2^(j/32), j < 32."""
    return [DEC.power(decimal.Decimal(2), DEC.divide(decimal.Decimal(j), decimal.Decimal(32))) for j in range(32)]


# ---- one rounding per operation --------------------------------------------------------------------------------------
def fma(a, b, c):
    """RN(a * b + c) for finite doubles, with IEEE's sign of an exact zero."""
    a, b, c = float(a), float(b), float(c)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        # round to nearest: x + (-x) = +0; a zero product plus a zero keeps a sign only when both have it
        both_negative_zeros = (a == 0.0 or b == 0.0) and c == 0.0 and math.copysign(1.0, c) < 0 and \
            math.copysign(1.0, a) * math.copysign(1.0, b) < 0
        return -0.0 if both_negative_zeros else 0.0
    return exact.numerator / exact.denominator  # int / int: correctly rounded


def count_fraction_expected(k, n):
    """k / n, the IEEE quotient: integers below 2^53 are exact doubles, and NumPy's float64 division is IEEE's."""
    return np.asarray(k, dtype=np.float64) / np.asarray(n, dtype=np.float64)


def count_le_expected(ck, scale, u, n):
    """clip(floor(fma(ck, scale, -u)) + 1, 0, n) row by row (finite arguments)."""
    out = np.empty(len(ck))
    for i, (c, s, uu, nn) in enumerate(zip(ck.tolist(), scale.tolist(), u.tolist(), n.tolist())):
        out[i] = min(max(math.floor(fma(c, s, -uu)) + 1.0, 0.0), nn)
    return out


def bilinear_expected(z00, z10, z01, z11, tx, ty):
    """The three fused operations of raster_bilinear_fast; the corner differences are plain (rounded) subtractions."""
    out = np.empty(len(z00))
    rows = zip(z00.tolist(), z10.tolist(), z01.tolist(), z11.tolist(), tx.tolist(), ty.tolist())
    for i, (a00, a10, a01, a11, x, y) in enumerate(rows):
        a = fma(x, a10 - a00, a00)
        b = fma(x, a11 - a01, a01)
        out[i] = fma(y, b - a, a)
    return out


# ---- input sets: {class name: float64 array}; the tests concatenate them ---------------------------------------------
# Both `x` and `1 / x` normal: 2^-1022 <= |x| <= 2^1022.
RCP_EXPONENTS = (-1022, 1022)
N_BULK = (1 << 20) + 37  # rows of the log-uniform class: not a multiple of the workgroup's 256 (nor is any total below)


def _log_uniform(rng, n, lo_exp, hi_exp):
    """m * 2^e, m uniform in [1, 2), e uniform over the integers [lo_exp, hi_exp)."""
    return np.ldexp(1.0 + rng.random(n), rng.integers(lo_exp, hi_exp, n).astype(np.int32))


def _near_one(scales):
    k = np.arange(1, 65, dtype=np.float64)
    base = np.concatenate((1.0 + k * EPS, 1.0 - k * (EPS / 2), 2.0 - k * EPS, [1.0]))
    return np.concatenate([base * s for s in scales])


def caller_values(rng, n=8192):
    """What the kernels feed to rcp_nr: depths along the optical axis, focal lengths, raster cell sizes, and 2 zs^2 for a
    surface sigma zs."""
    zs = np.geomspace(1e-6, 1e3, n)
    return {"depths": np.geomspace(0.1, 1e5, n), "focal lengths": rng.uniform(300.0, 3.0e4, n),
            "cell sizes": np.geomspace(1e-3, 1e3, n), "2 zs^2": 2.0 * (zs * zs)}


def rcp_inputs(seed=11):
    rng = np.random.default_rng(seed)
    lo, hi = RCP_EXPONENTS
    sets = {"log-uniform": _log_uniform(rng, N_BULK, lo, hi) * rng.choice([-1.0, 1.0], N_BULK)}
    p2 = np.ldexp(1.0, np.arange(lo, hi + 1, dtype=np.int32))
    sets["powers of two"] = np.concatenate((p2, -p2))
    near = _near_one([1.0, 2.0 ** -1021, 2.0 ** 1020, 2.0 ** 100, 3.0 * 2.0 ** -700])
    sets["1 +- k eps, 2 - k eps"] = np.concatenate((near, -near))
    sets.update(caller_values(rng))
    return sets


def sqrt_inputs(seed=12):
    rng = np.random.default_rng(seed)
    sets = {"log-uniform": _log_uniform(rng, N_BULK, -1022, 1024)}
    sets["powers of two"] = np.ldexp(1.0, np.arange(-1022, 1024, dtype=np.int32))
    sets["1 +- k eps, 2 - k eps"] = _near_one([1.0, 2.0, 2.0 ** -1021, 2.0 ** -1020, 2.0 ** 1021, 2.0 ** 1022, 2.0 ** 101])
    m = np.concatenate((np.arange(1.0, 4097.0), rng.integers(1, 1 << 26, 60000).astype(np.float64),
                        [float((1 << 26) - 1), float(1 << 26)]))
    e = rng.integers(-240, 240, len(m)).astype(np.int32)
    sets["perfect squares"] = np.concatenate((m * m, np.ldexp(m * m, 2 * e)))  # (m < 2^26.1: m^2 is exact)
    d = np.geomspace(1e-9, 1e4, 8192)
    dx, dy = d * rng.uniform(-1.0, 1.0, len(d)), d * rng.uniform(-1.0, 1.0, len(d))
    sets["dx^2 + dy^2"] = dx * dx + dy * dy
    return sets


def perfect_square_roots(x):
    """For the 'perfect squares' class: the exact roots (a float64 each)."""
    r = np.sqrt(x)  # IEEE: correctly rounded, hence exact on exact squares
    assert (r * r == x).all()
    return r


def minmax_inputs(seed=13):
    """Pairs (a, b) of non-NaN doubles; the class 'zeros' holds (+0.0, -0.0) in both orders."""
    rng = np.random.default_rng(seed)
    n = N_BULK
    a = _log_uniform(rng, n, -1022, 1024) * rng.choice([-1.0, 1.0], n)
    b = np.where(rng.random(n) < 0.5, a * (1.0 + rng.integers(-2, 3, n) * EPS), _log_uniform(rng, n, -1022, 1024) *
                 rng.choice([-1.0, 1.0], n))
    special = np.array([np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 2.0 ** -1040, -2.0 ** -1040, 2.2250738585072014e-308,
                        1.7976931348623157e308, -1.7976931348623157e308, 1.0, -1.0, 2.5, -2.5])
    sa, sb = [v.ravel() for v in np.meshgrid(special, special)]
    return {"random": (a, b), "equal": (a[:4096], a[:4096].copy()), "special": (sa, sb),
            "zeros": (np.array([0.0, -0.0]), np.array([-0.0, 0.0]))}


EXP_EDGES = np.array([0.0, 1e-300, 744.9, 746.5, 1e6])


def exp_inputs():
    """Arguments of exp_fast (all <= 0): the set of tests/test_hostcheck.py's fast-arithmetic test, every multiple of
    ln 2 / 32 down to -746.6 with its two neighbouring doubles (rint changes the table index there), and -745.2 .. -746.5
    in steps of 0.01 (where the result leaves the double range)."""
    sets = {"0 .. -50 dense": -np.linspace(0, 50, 20001), "1e-12 .. 745 geometric": -np.geomspace(1e-12, 745.0, 5000),
            "edge values": -EXP_EDGES}
    m = -np.arange(1, int(746.6 / LN2_32) + 1, dtype=np.float64) * LN2_32
    sets["multiples of ln2/32"] = np.concatenate((m, np.nextafter(m, -np.inf), np.nextafter(m, np.inf)))
    sets["-745.2 .. -746.5"] = -(745.2 + 0.01 * np.arange(131))
    # halfway between the multiples, where |r| is largest and the polynomial's truncation shows most
    sets["half multiples"] = (-np.arange(0, int(746.0 / LN2_32), dtype=np.float64) - 0.5) * LN2_32
    return sets


def chunks(x, size=20000):
    return [x[i:i + size] for i in range(0, len(x), size)]


def count_fraction_inputs(seed=14):
    rng = np.random.default_rng(seed)
    n = rng.integers(1, 65537, N_BULK)
    k = (rng.random(N_BULK) * (n + 1)).astype(np.int64)  # 0 <= k <= n
    sets = {"random": (k, n)}
    for nn in (1, 2, 3, 961, 3969, 65535, 65536):
        sets[f"every k of n = {nn}"] = (np.arange(nn + 1), np.full(nn + 1, nn))
    return sets


def count_le_inputs(seed=15):
    """(ck, scale, u, n) rows as the resampling kernels see them: w = exp(-ll) + 1e-300 for log likelihoods up to 200,
    ck the running sums, scale = n / sum(w), one u per vector."""
    rng = np.random.default_rng(seed)
    cols = [[], [], [], []]
    for n in (70, 513, 5000):
        for spread in (3.0, 40.0, 200.0):
            ll = rng.random(n) * spread
            if spread == 200.0:
                ll[rng.integers(0, n)] = 0.0  # one dominant particle: long runs of equal counts
            w = np.exp(-ll) + 1e-300
            ck = np.cumsum(w)
            for u in (rng.random(), 0.0, np.nextafter(1.0, 0.0)):
                cols[0].append(ck)
                cols[1].append(np.full(n, n / w.sum()))
                cols[2].append(np.full(n, u))
                cols[3].append(np.full(n, float(n)))
    return tuple(np.concatenate(c) for c in cols)


def bilinear_inputs(seed=16, n=30011):
    rng = np.random.default_rng(seed)
    z = [np.exp(rng.uniform(0.0, np.log(1e4), n)) * rng.choice([-1.0, 1.0], n) for _ in range(4)]
    z[1][:2000] = z[0][:2000] + rng.standard_normal(2000)  # neighbouring heights of a DEM: corners that nearly cancel
    z[3][:2000] = z[2][:2000] + rng.standard_normal(2000)
    z[2][:1000] = z[0][:1000]
    tx, ty = rng.random(n), rng.random(n)
    tx[::7], ty[::11] = 0.0, 1.0
    tx[3::13], ty[5::17] = 1.0, 0.0
    return (*z, tx, ty)


# ---- the projection --------------------------------------------------------------------------------------------------
def rotation(viewdir):
    """Camera.R as the library's host expands it (csrc/glh_host.h: expand_camera): the C library's cos / sin, which are
    `math`'s, and the same float64 expressions in the same order."""
    d2r = math.pi / 180.0
    C = [math.cos(v * d2r) for v in viewdir]
    S = [math.sin(v * d2r) for v in viewdir]
    return np.array([[C[0] * C[2] + S[0] * S[1] * S[2], C[0] * S[1] * S[2] - C[2] * S[0], -C[1] * S[2]],
                     [C[2] * S[0] * S[1] - C[0] * S[2], S[0] * S[2] + C[0] * C[2] * S[1], -C[1] * C[2]],
                     [C[1] * S[0], C[0] * C[1], S[1]]])


def project_reference(cam, xyz, directions=False):
    """Camera.xyz_to_uv (or Grid.xyz_to_uv for a raster grid) of the 24-double camera vector in longdouble: every
    operation after the float64 inputs (the vector, the rotation matrix made from it, the points) carries 64 bits.
    `directions`: xyz are ray directions from the camera (no offset, no elevation correction).
    Returns longdouble [n][2], NaN behind the camera."""
    require_longdouble()
    cam = np.asarray(cam, dtype=np.float64)
    p = np.asarray(xyz, dtype=np.float64).astype(LD)
    if cam[23] != 0.0:
        return np.stack(((p[:, 0] - LD(cam[0])) / LD(cam[8]), (p[:, 1] - LD(cam[1])) / LD(cam[9])), axis=1)
    R = rotation(cam[3:6]).astype(LD)
    d = p if directions else p - cam[0:3].astype(LD)
    if cam[20] != 0.0 and not directions:
        d[:, 2] = d[:, 2] + (LD(cam[22]) - 1) * (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) / (2 * LD(cam[21]))
    c = d @ R.T
    front = c[:, 2] > 0
    with np.errstate(all="ignore"):
        px, py = c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]
        r2 = px * px + py * py
        k = cam[12:18].astype(LD)
        dr = 1 + k[0] * r2 + k[1] * r2 ** 2 + k[2] * r2 ** 3
        if (cam[15:18] != 0.0).any():
            dr = dr / (1 + k[3] * r2 + k[4] * r2 ** 2 + k[5] * r2 ** 3)
        p1, p2 = LD(cam[18]), LD(cam[19])
        qx = px * dr + 2 * px * py * p1 + p2 * (r2 + 2 * px * px)
        qy = py * dr + p1 * (r2 + 2 * py * py) + 2 * px * py * p2
        u = qx * LD(cam[8]) + (LD(cam[6]) / 2 + LD(cam[10]))
        v = qy * LD(cam[9]) + (LD(cam[7]) / 2 + LD(cam[11]))
    nan = LD(np.nan)
    return np.stack((np.where(front, u, nan), np.where(front, v, nan)), axis=1)


def _camera_vector(imgsz, f, c=(0, 0), k=(0,) * 6, p=(0, 0), xyz=(0, 0, 0), viewdir=(0, 0, 0), correction=None):
    v = np.zeros(24)
    v[0:3], v[3:6], v[6:8], v[8:10], v[10:12] = xyz, viewdir, imgsz, f, c
    v[12:12 + len(k)] = k
    v[18:20] = p
    if correction:
        v[20], v[21], v[22] = 1.0, correction[0], correction[1]
    return v


def projection_cameras():
    """{name: (camera vector, accepted by the simple form)}: beside the goldens' cameras, one of each kind of term."""
    utm = (499000.5, 6781000.25, 450.0)
    cams = {
        "pinhole": (_camera_vector((4288, 2848), (3000.0, 3010.0), xyz=utm, viewdir=(120.0, -12.0, 1.5)), True),
        "k1..k3": (_camera_vector((2048, 1536), (1800.0, 1795.0), c=(3.5, -2.25), k=(-0.12, 0.03, -0.004), xyz=utm,
                                  viewdir=(-40.0, 5.0, -2.0)), True),
        "k4..k6": (_camera_vector((1000, 700), (1200.0, 1200.0), k=(0.05, -0.01, 0.002, 0.02, -0.01, 0.003),
                                  xyz=(40.0, -30.0, 90.0), viewdir=(30.0, -20.0, 0.0)), False),
        "tangential": (_camera_vector((800, 536), (700.0, 690.0), p=(1e-3, -2e-3), xyz=(-5.0, 4.0, 20.0),
                                      viewdir=(200.0, 3.0, 5.0)), False),
        "elevation correction": (_camera_vector((4288, 2848), (3000.0, 3010.0), k=(-0.1, 0.02), xyz=utm,
                                                viewdir=(75.0, -3.0, 0.0), correction=(6.3781e6, 0.13)), False),
    }
    grid = np.zeros(24)
    grid[0:2], grid[6:8], grid[8:10], grid[23] = (446000.0, 7396000.0), (2000.0, 1500.0), (10.0, -10.0), 1.0
    cams["raster grid"] = (grid, False)
    return cams


def simple_form_accepts(cam):
    """No raster grid, no k4..k6, no tangential terms, no elevation correction (glh_math.h: CAM_F_NOT_SIMPLE)."""
    cam = np.asarray(cam)
    return bool(cam[23] == 0.0 and not cam[15:18].any() and not cam[18:20].any() and cam[20] == 0.0)


def projection_points(cam, n=10007, seed=17):
    """World points for a camera: in front at depths 1 .. 1e5 along the optical axis across (and a little beyond) the
    image, a twelfth of them behind the camera; for a raster grid, points over and around the grid."""
    rng = np.random.default_rng(seed)
    cam = np.asarray(cam, dtype=np.float64)
    if cam[23] != 0.0:
        xy = cam[0:2] + rng.uniform(-0.1, 1.1, (n, 2)) * cam[6:8] * cam[8:10]
        return np.column_stack((xy, rng.uniform(0.0, 1500.0, n)))
    depth = np.geomspace(1.0, 1e5, n)
    rng.shuffle(depth)
    depth[::12] *= -1.0
    xn = rng.uniform(-0.55, 0.55, n) * cam[6] / cam[8]
    yn = rng.uniform(-0.55, 0.55, n) * cam[7] / cam[9]
    c = np.column_stack((xn * depth, yn * depth, depth))
    return c @ rotation(cam[3:6]) + cam[0:3]
