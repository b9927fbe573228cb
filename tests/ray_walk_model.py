"""A plain, per-pixel model of HOW the ray-cast kernel walks (rn_cast_kernel, vacancy_amd/csrc/render.hip), as opposed to
the flat definition restated in tests/render_ref.py: the start cell by bisection (init_axis), the one-crossing step, the
jump over a brick of 8 x 8 x 8 voxels without a solid one (bricks and occupancy bits counted from the slab's z0), the
entry jump from outside the grid, the count of an axis' planes that sort before an event (count_before / jump), the slab
narrowing of "inside" to zlo <= i_z < zhi, and "rayskip" on and off.  It is written from the definition in
include/vacancy_hip.h and the kernel's comments, in Python; no device code is in it.

Every t_a(k) = (P_a[k] - o_a) * inv_a is computed once, in float32, from the integer k (numpy); the walk then compares
those float32 values (held as Python floats, which represent them exactly, signed zeros included).

The model takes named MUTANTS, each one comparison of the kernel turned:
  step_le     the one-crossing step gives a tie to the higher axis (<= where the kernel has <)
  brick_le    the brick jump picks its event with <=: a tie goes to the higher axis
  count_flip  count_before's axis_first inverted
  count_lt    count_before without its t == tE term
  entry_gt    the entry jump picks its event with >: a tie goes to the lower axis
  neg_zero    the depth of a hit is t as it stands, -0.0 included
  start_le    a plane with t <= 0 counts as behind the start
  still_lt    on an axis without crossings the start cell counts the planes with P[k] < o
tests/test_ray_lattice_cpu.py shows that the unmutated model equals the restatement and which mutants the scenes of
tests/ray_lattice_scenes.py tell apart."""
import numpy as np

import render_ref as RR

F = np.float32
INF = float("inf")
MUTANTS = ("step_le", "brick_le", "count_flip", "count_lt", "entry_gt", "neg_zero", "start_le", "still_lt")


class Rays:
    """The rays of a view over a grid: per pixel and axis the direction of travel s, the origin o and the table t_a(k)."""

    def __init__(self, view, planes, dims):
        self.w, self.h, self.dims = view.width, view.height, tuple(dims)
        o, d, roi = RR.rays(view)
        self.ok = (roi & np.isfinite(o).all(0) & np.isfinite(d).all(0)).tolist()
        self.P = [np.asarray(p, F).astype(np.float64).tolist() for p in planes]
        self.o, self.s, self.T = [], [], []
        with np.errstate(all="ignore"):
            for a in range(3):
                inv = F(1.0) / d[a]
                moves = (d[a] != 0) & np.isfinite(inv)
                inv = np.where(moves, inv, F(0.0)).astype(F)
                t = (np.asarray(planes[a], F)[None, :] - o[a][:, None]) * inv[:, None]
                assert t.dtype == F
                self.o.append(o[a].astype(np.float64).tolist())
                self.s.append(np.where(moves, np.where(d[a] > 0, 1, -1), 0).tolist())
                self.T.append(t.astype(np.float64).tolist())


def occupancy(solid, dims, zlo, zhi):
    """One flag per brick of the slices [zlo, zhi), bricks counted from zlo: a voxel of the brick is solid."""
    nx, ny, _ = dims
    s3 = np.asarray(solid, bool).reshape(dims[2], ny, nx)[zlo:zhi]
    nbx, nby, nbz = (nx + 7) // 8, (ny + 7) // 8, (zhi - zlo + 7) // 8
    occ = [False] * (nbx * nby * nbz)
    for bz in range(nbz):
        for by in range(nby):
            for bx in range(nbx):
                occ[(bz * nby + by) * nbx + bx] = bool(s3[bz * 8:bz * 8 + 8, by * 8:by * 8 + 8, bx * 8:bx * 8 + 8].any())
    return occ, nbx, nby


def cast(rays, solid, z_range=None, rayskip=1, mutant=None):
    """(depth float32, voxel int64, axis uint8) images: what the kernel's walk gives for the flat boolean array `solid`
    (voxel-id order, whole grid), on a context that owns the slices z_range (default: all of them)."""
    assert mutant is None or mutant in MUTANTS, mutant
    n = rays.dims
    nx, ny, nz = n
    zlo, zhi = z_range if z_range is not None else (0, nz)
    lo, hi = (0, 0, zlo), (nx, ny, zhi)   # the range of cells a voxel can be hit in; the bricks start at lo
    sol = np.asarray(solid, bool).reshape(-1).tolist()
    occ, nbx, nby = occupancy(solid, n, zlo, zhi)
    step_le, brick_le, count_flip, count_lt = (mutant == m for m in ("step_le", "brick_le", "count_flip", "count_lt"))
    entry_gt, neg_zero, start_le, still_lt = (mutant == m for m in ("entry_gt", "neg_zero", "start_le", "still_lt"))
    n_px = rays.w * rays.h
    depth = np.full(n_px, np.inf, F)
    voxel = np.full(n_px, -1, np.int64)
    axis = np.full(n_px, 255, np.uint8)

    for px in range(n_px):
        if not rays.ok[px]:
            continue
        T = (rays.T[0][px], rays.T[1][px], rays.T[2][px])
        s = (rays.s[0][px], rays.s[1][px], rays.s[2][px])
        i, tn = [0, 0, 0], [INF, INF, INF]

        def next_t(a):
            k = i[a] + 1 if s[a] > 0 else i[a]
            return INF if s[a] == 0 or k < 0 or k > n[a] else T[a][k]

        # init_axis: the first k of 0 .. n at which the planes stop lying on the low side of the start, minus one
        for a in range(3):
            first, last = 0, n[a] + 1
            while first < last:
                mid = (first + last) >> 1
                t = T[a][mid]
                behind = t <= 0.0 if start_le else t < 0.0
                if s[a] > 0:
                    low = behind
                elif s[a] < 0:
                    low = not behind
                else:
                    low = rays.P[a][mid] < rays.o[a][px] if still_lt else rays.P[a][mid] <= rays.o[a][px]
                if low:
                    first = mid + 1
                else:
                    last = mid
            i[a] = first - 1
            tn[a] = next_t(a)

        def jump(aE, tE, kE, m):
            """Moves the ray to just behind the event on plane kE[aE] of axis aE; m[b]: the planes of b that may lie before it."""
            for b in range(3):
                if b == aE:
                    i[b] = kE[b] if s[b] > 0 else kE[b] - 1
                elif s[b] != 0 and m[b] > 0:
                    axis_first = (b > aE) if count_flip else (b < aE)
                    first, last = 0, m[b]                       # count_before
                    while first < last:
                        mid = (first + last + 1) >> 1
                        t = T[b][i[b] + mid if s[b] > 0 else i[b] - mid + 1]
                        if t < tE or (not count_lt and t == tE and axis_first):
                            first = mid
                        else:
                            last = mid - 1
                    i[b] += s[b] * first
                tn[b] = next_t(b)

        t_in, a_in = 0.0, 3
        for _ in range(4 * (nx + ny + nz) + 16):   # (every round but a first look into a brick crosses a plane)
            if lo[0] <= i[0] < hi[0] and lo[1] <= i[1] < hi[1] and lo[2] <= i[2] < hi[2]:
                if rayskip and not occ[(((i[2] - zlo) >> 3) * nby + (i[1] >> 3)) * nbx + (i[0] >> 3)]:
                    # the brick planes ahead, and the earliest of them
                    kE, m, aE, tE = [0, 0, 0], [0, 0, 0], -1, INF
                    for a in range(3):
                        rel = i[a] - lo[a]
                        if s[a] > 0:
                            kE[a] = min(lo[a] + (rel | 7) + 1, hi[a])
                            m[a] = kE[a] - 1 - i[a]
                        else:
                            kE[a] = lo[a] + (rel & ~7)
                            m[a] = i[a] - kE[a]
                        if s[a] != 0:
                            t = T[a][kE[a]]
                            if (t <= tE) if brick_le else (t < tE):
                                tE, aE = t, a
                    if aE < 0:
                        break
                    jump(aE, tE, kE, m)
                    t_in, a_in = tE, aE
                    continue
                if sol[(i[2] * ny + i[1]) * nx + i[0]]:
                    depth[px] = t_in if neg_zero else (0.0 if t_in == 0.0 else t_in)
                    voxel[px] = (i[2] * ny + i[1]) * nx + i[0]
                    axis[px] = a_in
                    break
            else:
                gone = waiting = False
                for a in range(3):
                    below, above = i[a] < lo[a], i[a] >= hi[a]
                    gone = gone or (below and s[a] <= 0) or (above and s[a] >= 0)
                    waiting = waiting or below or above
                if gone:
                    break
                if rayskip and waiting:
                    # the planes through which the out-of-range axes come into range, and the latest of them
                    kE, m, aE, tE = [0, 0, 0], [0, 0, 0], -1, -INF
                    for a in range(3):
                        kE[a] = lo[a] if s[a] > 0 else hi[a]
                        m[a] = n[a] - i[a] if s[a] > 0 else i[a] + 1
                        if i[a] < lo[a] or i[a] >= hi[a]:
                            t = T[a][kE[a]]
                            if (t > tE) if entry_gt else (t >= tE):
                                tE, aE = t, a
                    if aE < 0 or tE == INF:
                        break
                    jump(aE, tE, kE, m)
                    t_in, a_in = tE, aE
                    continue
            # one crossing: the smallest (t, axis)
            a, t = 0, tn[0]
            if (tn[1] <= t) if step_le else (tn[1] < t):
                t, a = tn[1], 1
            if (tn[2] <= t) if step_le else (tn[2] < t):
                t, a = tn[2], 2
            if t == INF:
                break
            i[a] += s[a]
            tn[a] = next_t(a)
            t_in, a_in = t, a
        else:
            raise AssertionError("pixel %d: the walk does not end" % px)
    shape = (rays.h, rays.w)
    return depth.reshape(shape), voxel.reshape(shape), axis.reshape(shape)
