"""Ray casting: the rule (INPUTS.md, "Ray casting: the rule"), restated in NumPy.

The reference has no function that casts rays onto a DEM, so this restatement is the contract of `glh_stage_raycast`
(csrc/glh_raycast.hip): the kernel performs the same float64 operations in the same order, and
tests/test_gpu_raycast.py holds it to `cast` bit for bit.  Rays are marched in lockstep, one array element per ray; every
expression below is one rounded operation per operator, as NumPy evaluates it, and every minimum and maximum is written
as a comparison and a choice (`_lower`, `_upper`) so that the device can make the same one.

A ray is P(t) = o + t d.  The surface is the bilinear patches between the DEM's cell centres; in grid coordinates
p = (x - x[0]) / d0, q = (y - y[0]) / d1 patch (i, j) is [i, i + 1] x [j, j + 1] and the domain is
[0, nx - 1] x [0, ny - 1].  g(t) = ray height - apparent surface is a quadratic in t inside a patch (`_patch`).
"""
import numpy as np

HIT, MISS, BELOW, LEAVES, INVALID = 0, 1, 2, 3, 4
STATUS = ("hit", "misses the domain", "enters below the surface", "leaves without a hit", "invalid")

# A block is skipped when the ray clears its highest cell by more than this fraction of the magnitudes involved: 2^22
# times the rounding of the heights compared, so that a skipped patch is one the plain march would not have hit either.
SKIP_MARGIN = 2.0 ** -30


def _lower(a, b):
    """b where b < a, else a."""
    return np.where(b < a, b, a)


def _upper(a, b):
    """b where b > a, else a."""
    return np.where(b > a, b, a)


def crossing(line, p0, dp):
    """The time at which a ray crosses an integer line of an axis: a pure function of the line's index."""
    return (line - p0) / dp


def _entered(c, p0, dp):
    """The time at which a ray enters column c of an axis: through line c when it travels up the axis, c + 1 when down."""
    return crossing(np.where(dp > 0, c, c + 1).astype(np.float64), p0, dp)


def column_at(T, p0, dp, n, strict):
    """The column (patch index along one axis of n cells) a ray is in once every line crossing with a time <= T (< T when
    `strict`) has been made: the furthest column along its travel that it has entered by then, the first one if it has
    entered none.  A ray that does not move along the axis stays in min(floor(p0), n - 2)."""
    last = n - 2
    still = dp == 0
    dps = np.where(still, 1.0, dp)
    s = np.where(dps > 0, 1, -1)
    guess = np.floor(p0 + T * dps)
    c = np.where(guess > 0, np.where(guess < last, guess, last), 0).astype(np.int64)

    def reached(col):
        e = _entered(col, p0, dps)
        return e < T if strict else e <= T

    for _ in range(n):  # (the guess is off by a rounding: one pass; the bound is what the device's loop has)
        nxt = c + s
        go = ~still & (nxt >= 0) & (nxt <= last)
        go &= reached(np.clip(nxt, 0, last))
        if not go.any():
            break
        c = np.where(go, nxt, c)
    for _ in range(n):
        prv = c - s
        back = ~still & (prv >= 0) & (prv <= last) & ~reached(c)
        if not back.any():
            break
        c = np.where(back, prv, c)
    fixed = np.floor(np.where(still, p0, 0.0))
    fixed = np.where(fixed > 0, np.where(fixed < last, fixed, last), 0).astype(np.int64)
    return np.where(still, fixed, c)


def block_max(z, block):
    """The NaN-ignoring maximum over the cells of every block of `block` x `block` patches (one more cell than patches
    each way; -inf for a block without a value), (nby, nbx)."""
    ny, nx = z.shape
    nbx, nby = -(-(nx - 1) // block), -(-(ny - 1) // block)
    out = np.full((nby, nbx), -np.inf)
    for bj in range(nby):
        for bi in range(nbx):
            cells = z[bj * block: min(bj * block + block, ny - 1) + 1, bi * block: min(bi * block + block, nx - 1) + 1]
            cells = cells[~np.isnan(cells)]
            if cells.size:
                out[bj, bi] = cells.max()
    return out


def _patch(z, i, j, p0, q0, dp, dq, oz, dz, K):
    """(A, B, C, whole) of g(t) = (A t + B) t + C in patch (i, j); `whole`: none of its corners is NaN."""
    z00, z10, z01, z11 = z[j, i], z[j, i + 1], z[j + 1, i], z[j + 1, i + 1]
    e1 = z10 - z00
    e2 = z01 - z00
    e3 = (z11 - z01) - e1
    u0 = p0 - i
    v0 = q0 - j
    C = (oz - z00) - ((u0 * e1 + v0 * e2) + (u0 * v0) * e3)
    B = dz - ((dp * e1 + dq * e2) + (u0 * dq + v0 * dp) * e3)
    A = -((dp * dq) * e3) - K
    whole = ~(np.isnan(z00) | np.isnan(z10) | np.isnan(z01) | np.isnan(z11))
    return A, B, C, whole


def _g(A, B, C, t):
    return (A * t + B) * t + C


def _root(A, B, C, t0, t1):
    """The root of the patch's quadratic nearest [t0, t1], clamped into it: q = -(B + copysign(sqrt(disc), B)) / 2 with
    roots q / A and C / q, the linear form -C / B when A == 0."""
    disc = B * B - (4.0 * A) * C
    disc = np.where(disc > 0, disc, 0.0)
    qq = (B + np.copysign(np.sqrt(disc), B)) * -0.5
    ra = qq / A
    rb = np.where(qq != 0, C / qq, ra)
    lo = np.where(rb < ra, rb, ra)
    hi = np.where(rb < ra, ra, rb)

    def outside(r):
        return np.where(r < t0, t0 - r, np.where(r > t1, r - t1, 0.0))

    t = np.where(outside(hi) < outside(lo), hi, lo)
    t = np.where(A == 0, -C / B, t)
    t = np.where(t >= t0, t, t0)
    return np.where(t > t1, t1, t)


def cast(origins, directions, z, x0, y0, d0, d1, correction=None, block=0, return_steps=False):
    """The rule for n rays.  origins (3,) or (n, 3), directions (n, 3); z (ny, nx) elevations (float32 is widened);
    x0, y0 the centre of cell (0, 0); d0, d1 the signed cell sizes; correction None or (radius, refraction); block 0 or
    a power of two.  Returns t (n,), xyz (n, 3), patch (n,) int32 (row * (nx - 1) + column, -1 without a hit) and
    status (n,) uint8; with `return_steps` also how many patches each ray evaluated."""
    z = np.asarray(z, dtype=np.float64)
    ny, nx = z.shape
    d = np.asarray(directions, dtype=np.float64).reshape(-1, 3)
    n = len(d)
    o = np.broadcast_to(np.asarray(origins, dtype=np.float64).reshape(-1, 3), (n, 3))
    if block and (block & (block - 1)):
        raise ValueError("block is 0 or a power of two")
    with np.errstate(all="ignore"):
        ox, oy, oz = o[:, 0], o[:, 1], o[:, 2]
        dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
        p0, q0 = (ox - x0) / d0, (oy - y0) / d1
        dp, dq = dx / d0, dy / d1
        if correction is None:
            K = np.zeros(n)
        else:
            radius, refraction = correction
            K = ((refraction - 1.0) * (dx * dx + dy * dy)) / (2.0 * radius)
        valid = np.isfinite(o).all(axis=1) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)
        valid &= np.isfinite(p0) & np.isfinite(q0) & np.isfinite(dp) & np.isfinite(dq) & np.isfinite(K)
        status = np.where(valid, LEAVES, INVALID).astype(np.uint8)
        p0, q0, dp, dq, K = (np.where(valid, v, 0.0) for v in (p0, q0, dp, dq, K))  # (an invalid ray marches nowhere)
        t = np.full(n, np.nan)
        patch = np.full(n, -1, dtype=np.int32)
        steps = np.zeros(n, dtype=np.int64)

        # the domain: the 2-D slab test, the entry clamped to t >= 0
        def slab(c0, dc, cells):
            a, b = crossing(0.0, c0, dc), crossing(float(cells - 1), c0, dc)
            moving = dc != 0
            near = np.where(moving, _lower(a, b), -np.inf)
            far = np.where(moving, _upper(a, b), np.inf)
            return near, far, moving | ((c0 >= 0) & (c0 <= cells - 1))

        near_p, far_p, in_p = slab(p0, dp, nx)
        near_q, far_q, in_q = slab(q0, dq, ny)
        t_in = _upper(near_p, near_q)
        t_in = np.where(t_in > 0, t_in, 0.0)
        t_out = _lower(far_p, far_q)
        misses = valid & ~(in_p & in_q & (t_in <= t_out))
        status[misses] = MISS
        active = valid & ~misses

        # where the ray enters: every crossing with a time <= t_in has been made
        i = column_at(t_in, p0, dp, nx, strict=False)
        j = column_at(t_in, q0, dq, ny, strict=False)
        A, B, C, whole = _patch(z, i, j, p0, q0, dp, dq, oz, dz, K)
        below = active & (_g(A, B, C, t_in) <= 0)
        status[below] = BELOW
        active &= ~below
        # a vertical ray: one patch, g linear
        vertical = active & (dp == 0) & (dq == 0)
        falls = vertical & whole & (B < 0)
        tv = -C / B
        tv = np.where(tv >= t_in, tv, t_in)
        t[falls], status[falls] = tv[falls], HIT
        patch[falls] = (j * (nx - 1) + i)[falls]
        steps[vertical] += 1
        active &= ~vertical

        t0 = t_in.copy()
        sp, sq = np.where(dp > 0, 1, -1), np.where(dq > 0, 1, -1)
        if block:
            shift = block.bit_length() - 1
            zmax = block_max(z, block)
            nbx = zmax.shape[1]
            tested = np.full(n, -1, dtype=np.int64)
        for _ in range(2 * (nx + ny) + 8):
            if not active.any():
                break
            stepping = active.copy()
            if block:
                bi, bj = i >> shift, j >> shift
                blk = bj * nbx + bi
                fresh = active & (blk != tested)
                tested = np.where(fresh, blk, tested)
                Lp = np.where(dp > 0, np.minimum((bi + 1) * block, nx - 1), bi * block).astype(np.float64)
                Lq = np.where(dq > 0, np.minimum((bj + 1) * block, ny - 1), bj * block).astype(np.float64)
                tLp = np.where(dp != 0, crossing(Lp, p0, dp), np.inf)
                tLq = np.where(dq != 0, crossing(Lq, q0, dq), np.inf)
                te = _lower(_lower(tLp, tLq), t_out)
                h0, h1 = oz + t0 * dz, oz + te * dz
                hmin = _lower(h0, h1)
                cmax = _upper(K * (t0 * t0), K * (te * te))
                zm = zmax[bj, bi]
                margin = SKIP_MARGIN * ((((np.abs(oz) + np.abs(t0 * dz)) + np.abs(te * dz)) + np.abs(zm)) + np.abs(cmax))
                skip = fresh & ((zm == -np.inf) | (hmin - (zm + cmax) > margin))
                gone = skip & (te >= t_out)
                active &= ~gone  # (status stays LEAVES)
                move = skip & ~gone
                p_first = tLp <= tLq
                ip = np.where(dp > 0, Lp, Lp - 1).astype(np.int64)
                jq = np.where(dq > 0, Lq, Lq - 1).astype(np.int64)
                i_new = np.where(p_first, ip, column_at(tLq, p0, dp, nx, strict=False))
                j_new = np.where(p_first, column_at(tLp, q0, dq, ny, strict=True), jq)
                i = np.where(move, np.clip(i_new, 0, nx - 2), i)
                j = np.where(move, np.clip(j_new, 0, ny - 2), j)
                t0 = np.where(move, te, t0)
                stepping = active & ~skip
            # one patch
            tnp = np.where(dp != 0, crossing((i + (dp > 0)).astype(np.float64), p0, dp), np.inf)
            tnq = np.where(dq != 0, crossing((j + (dq > 0)).astype(np.float64), q0, dq), np.inf)
            t1 = _lower(_lower(tnp, tnq), t_out)
            A, B, C, whole = _patch(z, i, j, p0, q0, dp, dq, oz, dz, K)
            steps[stepping] += 1
            hit = stepping & whole & (_g(A, B, C, t1) <= 0)
            th = np.where(_g(A, B, C, t0) <= 0, t0, _root(A, B, C, t0, t1))
            t[hit], status[hit] = th[hit], HIT
            patch[hit] = (j * (nx - 1) + i)[hit]
            active &= ~hit
            on = stepping & ~hit
            ends = on & (t1 >= t_out)
            active &= ~ends
            on &= ~ends
            step_p = tnp <= tnq  # (on a tie the p line is taken first)
            i = np.where(on & step_p, i + sp, i)
            j = np.where(on & ~step_p, j + sq, j)
            out = on & ((i < 0) | (i > nx - 2) | (j < 0) | (j > ny - 2))
            active &= ~out
            i, j = np.clip(i, 0, nx - 2), np.clip(j, 0, ny - 2)
            t0 = np.where(on, t1, t0)
        xyz = o + t[:, None] * d
    if return_steps:
        return t, xyz, patch, status, steps
    return t, xyz, patch, status


def camera_rays(cam, uv):
    """(origin, directions) of the pixels `uv` of a camera without distortion, on the host: what
    `cam.uv_to_xyz(uv, directions=True)` computes on the device for such a camera (glh_math.h: unproject)."""
    if cam.k.any() or cam.p.any():
        raise ValueError("camera_rays restates the unprojection of an undistorted camera only")
    xy = (np.asarray(uv, dtype=np.float64) - (cam.imgsz / 2 + cam.c)) * (1.0 / cam.f)
    return np.array(cam.xyz, dtype=np.float64), cam._xy_to_xyz(xy)


def grid_uv(imgsz, step):
    """The pixel centres step / 2 + k step of `Camera.xyz_map`: (rows, cols, 2)."""
    cols, rows = int(imgsz[0]) // step, int(imgsz[1]) // step
    u, v = (np.arange(cols) + 0.5) * step, (np.arange(rows) + 0.5) * step
    return np.stack(np.meshgrid(u, v), axis=2)
