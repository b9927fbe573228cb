"""Scenes in which the plane crossings of a ray TIE -- shared by test_ray_lattice_cpu.py (which shows, from the numpy
restatement alone, that the ties are reached, and that a per-pixel model of the kernel's walk with one comparison turned
gives other images on them) and test_gpu_ray_lattice.py (which compares the device with the restatement on them).  No GPU
is needed here.

The definition of the ray-cast orders a ray's crossings "by (t, axis) ascending" (include/vacancy_hip.h).  A tie needs two
axes with the same float t, which random look-at views never produce.  Here the grids are those of lattice_scenes.py
(resolution 1, box centred on the origin: every plane is an integer), the rotations are signed permutation matrices, fx
and fy are powers of two, cx and cy integers, and the camera centre has integer coordinates: d_c = ((u - cx) / f,
(v - cy) / f, 1) and its reciprocals are exact for the pixels whose offset from the principal point is a power of two, and
the rays through a lattice point go on meeting lattice edges and corners.

trace() is the walk of tests/render_ref.py with notes taken: which pixels tie, where, and which cells a path enters and
leaves at one t between two brick planes (the `corner_cut` states make exactly those solid)."""
import functools

import numpy as np

import lattice_scenes as L
import render_ref as RR
from vacancy_amd.capi import make_view

F = np.float32
INF = F(np.inf)
LOWEST = np.finfo(np.float32).min
W, H = 48, 40
GRIDS = L.GRIDS
GRID_NAMES = list(GRIDS)
IDENT = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
# the viewing axis (row 2) is +x, the image's u runs along y and its v along z
PERM = ((0, 1, 0), (0, 0, 1), (1, 0, 0))
# where the view corner_in stands: a lattice corner inside both grids, 2 below the brick planes y = 0 and z = 0, so that
# the row v == cy + 16 ties on two brick planes
CORNER = (-4, -2, -2)


def dims_of(grid):
    return (GRIDS[grid], 16, 16)


def option(grid):
    return L.grid_option(grid)


@functools.lru_cache(maxsize=None)
def planes_of(grid):
    """The plane tables of the grid; every plane is an integer, k - n / 2."""
    planes = RR.option_planes(option(grid))
    for p, n in zip(planes, dims_of(grid)):
        assert np.array_equal(p, (np.arange(n + 1) - n // 2).astype(F)) and n % 2 == 0, p
    return planes


def view_specs(nx):
    """name -> (rotation rows, camera centre, fx, fy, cx, cy, roi).
      corner_out      outside, equal offsets from three faces: two or three axes come into range at one t
      corner_in       inside, on a lattice corner: every ray starts on planes (t == 0, and -0.0 where an axis travels down)
      negz            s_y, s_z < 0
      perm            the viewing axis is x; a wide field
      neg_all         s_x, s_z < 0; a narrow field, long paths
      on_face         the camera on the grid's corner: the column u == cx and the row v == cy have d == 0 on an axis whose
                      origin equals P[0] (inside: P[k] <= o)
      on_far_face     the same at P[n]: such rays are outside on that axis and miss
      corner_out_roi  corner_out with a shrunk ROI
      negz_fxfy       negz with fx = 16, fy = 32: along v every second plane ties"""
    h = nx // 2
    return {
        "corner_out": (IDENT, (-h - 2, -10, -10), 16.0, 16.0, 8.0, 4.0, None),
        "corner_in": (IDENT, CORNER, 16.0, 16.0, 24.0, 20.0, None),
        "negz": (((1, 0, 0), (0, -1, 0), (0, 0, -1)), (-h - 2, 10, 12), 16.0, 16.0, 8.0, 4.0, None),
        "perm": (PERM, (-h - 4, -10, -10), 8.0, 8.0, 8.0, 4.0, None),
        "neg_all": (((-1, 0, 0), (0, 1, 0), (0, 0, -1)), (h + 2, -10, 12), 32.0, 32.0, 4.0, 2.0, None),
        "on_face": (IDENT, (-h, -8, -8), 16.0, 16.0, 8.0, 4.0, None),
        "on_far_face": (IDENT, (h, 8, -12), 16.0, 16.0, 40.0, 36.0, None),
        "corner_out_roi": (IDENT, (-h - 2, -10, -10), 16.0, 16.0, 8.0, 4.0, ((9, 5), (44, 36))),
        "negz_fxfy": (((1, 0, 0), (0, -1, 0), (0, 0, -1)), (-h - 2, 10, 12), 16.0, 32.0, 8.0, 4.0, None),
    }


VIEW_NAMES = list(view_specs(24))


def make(spec):
    rot, centre, fx, fy, cx, cy, roi = spec
    r = np.array(rot, np.float64)
    w2c = np.zeros((3, 4), F)
    w2c[:, :3] = r
    w2c[:, 3] = 0.0 - r @ np.array(centre, np.float64)
    assert abs(np.linalg.det(r)) == 1.0 and np.array_equal(np.abs(r).sum(0), np.ones(3))
    for f in (fx, fy):
        assert np.log2(f) == int(np.log2(f))
    assert cx == int(cx) and cy == int(cy) and all(c == int(c) for c in centre)
    rmin, rmax = roi if roi else (None, None)
    return make_view(w2c, fx, fy, cx, cy, W, H, rmin, rmax)


@functools.lru_cache(maxsize=None)
def views(grid):
    return {name: make(spec) for name, spec in view_specs(GRIDS[grid]).items()}


# ---- the walk of the restatement, with notes -------------------------------------------------------------------------

FLAGS = ("tie2", "tie3", "tie_inside", "tie_brick", "tie_at_cut", "start_on_plane", "still_on_plane")


def trace(view, planes, dims, solid=None, z_cuts=()):
    """render_ref.render's walk, round for round, with notes.  A path is followed until it hits or has left the grid for
    good (an axis out of range that does not travel back).  Returns a dict:
      depth, voxel, axis   the images, as render_ref.render gives them
      raw_t                the t of the crossing that entered the hit voxel before the -0 -> +0 rule (NaN on a miss)
      corner_cells         bool [nz, ny, nx]: cells inside the grid that a path enters and leaves at the same t, both
                           crossings on interior brick planes (k % 8 == 0, 0 < k < n)
      and bool [pixels] per name of FLAGS:
      tie2 / tie3          a crossing of the path has two / three axes at its t
      tie_inside           such a tie while the state is inside the grid
      tie_brick            such a tie, inside, with two of the tied planes interior brick planes
      tie_at_cut           such a tie with the z plane among the tied ones and its index in z_cuts
      start_on_plane       a moving axis has t_a(k) == 0 for some k
      still_on_plane       a still axis' origin equals one of its planes"""
    w, h = view.width, view.height
    n_px = w * h
    o, d, roi = RR.rays(view)
    solid3 = (np.zeros(dims[::-1], bool) if solid is None else np.asarray(solid, bool).reshape(dims[2], dims[1], dims[0]))
    alive = roi & np.isfinite(o).all(0) & np.isfinite(d).all(0)
    out = {name: np.zeros(n_px, bool) for name in FLAGS}
    T, S, I = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = F(1.0) / d[a]
            moves = (d[a] != 0) & np.isfinite(inv)
            inv = np.where(moves, inv, F(0.0)).astype(F)
            s = np.where(moves, np.where(d[a] > 0, 1, -1), 0)
            P = planes[a]
            t = ((P[None, :] - o[a][:, None]) * inv[:, None]).astype(F)
            behind = t < 0
            low = np.where((s > 0)[:, None], behind, np.where((s < 0)[:, None], ~behind, P[None, :] <= o[a][:, None]))
            T.append(t)
            S.append(s)
            I.append(low.sum(1) - 1)
            out["start_on_plane"] |= alive & moves & (t == 0).any(1)
            out["still_on_plane"] |= alive & ~moves & (P[None, :] == o[a][:, None]).any(1)
    depth = np.full(n_px, INF, F)
    raw_t = np.full(n_px, np.nan, F)
    voxel = np.full(n_px, -1, np.int64)
    axis = np.full(n_px, 255, np.uint8)
    t_in = np.zeros(n_px, F)
    a_in = np.full(n_px, 3, np.uint8)
    prev_brick = np.zeros(n_px, bool)
    corner = np.zeros(dims[::-1], bool)
    px = np.arange(n_px)
    cuts = np.array(sorted(z_cuts), np.int64)
    while alive.any():
        inside = np.ones(n_px, bool)
        gone = np.zeros(n_px, bool)
        for a in range(3):
            inside &= (I[a] >= 0) & (I[a] < dims[a])
            gone |= ((I[a] < 0) & (S[a] <= 0)) | ((I[a] >= dims[a]) & (S[a] >= 0))
        cx, cy, cz = (np.clip(I[a], 0, dims[a] - 1) for a in range(3))
        hit = alive & inside & solid3[cz, cy, cx]
        depth[hit] = np.where(t_in[hit] == 0, F(0.0), t_in[hit])
        raw_t[hit] = t_in[hit]
        voxel[hit] = (cz[hit].astype(np.int64) * dims[1] + cy[hit]) * dims[0] + cx[hit]
        axis[hit] = a_in[hit]
        alive &= ~hit & ~gone
        tn, ks = [], []
        for a in range(3):
            k = np.where(S[a] > 0, I[a] + 1, I[a])
            ok = (S[a] != 0) & (k >= 0) & (k <= dims[a])
            tn.append(np.where(ok, T[a][px, np.clip(k, 0, dims[a])], INF))
            ks.append(k)
        tn = np.stack(tn)
        a_next = np.argmin(tn, axis=0)
        t_next = tn[a_next, px]
        alive &= t_next != INF
        tied = [tn[a] == t_next for a in range(3)]
        brick = [tied[a] & (ks[a] % 8 == 0) & (ks[a] > 0) & (ks[a] < dims[a]) for a in range(3)]
        n_tied = tied[0].astype(int) + tied[1] + tied[2]
        n_brick = brick[0].astype(int) + brick[1] + brick[2]
        out["tie2"] |= alive & (n_tied >= 2)
        out["tie3"] |= alive & (n_tied == 3)
        out["tie_inside"] |= alive & inside & (n_tied >= 2)
        out["tie_brick"] |= alive & inside & (n_brick >= 2)
        if len(cuts):
            out["tie_at_cut"] |= alive & (n_tied >= 2) & tied[2] & np.isin(ks[2], cuts)
        this_brick = (brick[0] & (a_next == 0)) | (brick[1] & (a_next == 1)) | (brick[2] & (a_next == 2))
        between = alive & inside & (a_in != 3) & (t_next == t_in) & prev_brick & this_brick
        corner[cz[between], cy[between], cx[between]] = True
        prev_brick = np.where(alive, this_brick, prev_brick)
        for a in range(3):
            go = alive & (a_next == a)
            I[a] = np.where(go, I[a] + S[a], I[a])
        t_in = np.where(alive, t_next, t_in).astype(F)
        a_in = np.where(alive, a_next, a_in).astype(np.uint8)
    out.update(depth=depth.reshape(h, w), voxel=voxel.reshape(h, w), axis=axis.reshape(h, w), raw_t=raw_t.reshape(h, w),
               corner_cells=corner)
    return out


def render_by_sorting(view, planes, dims, solid):
    """render_ref.render's images by another reading of the same definition: per pixel, ALL crossings ahead are sorted by
    (t, axis) at once -- a stable sort, every axis in its order of travel -- and the states of the path are the running
    sums.  Its cost does not grow with the rounds of render_ref.render (one per crossing of the longest path), which is
    what a ray along an axis of 12 000 cells needs; test_ray_lattice_cpu.py holds it against render_ref.render."""
    w, h = view.width, view.height
    o, d, roi = RR.rays(view)
    solid3 = np.asarray(solid, bool).reshape(dims[2], dims[1], dims[0])
    alive = roi & np.isfinite(o).all(0) & np.isfinite(d).all(0)
    depth = np.full(w * h, INF, F)
    voxel = np.full(w * h, -1, np.int64)
    axis = np.full(w * h, 255, np.uint8)
    for px in np.nonzero(alive)[0]:
        start, ts, axs, sign = [], [], [], []
        with np.errstate(all="ignore"):
            for a in range(3):
                inv = F(1.0) / d[a, px]
                moves = bool(d[a, px] != 0) and bool(np.isfinite(inv))
                s = 0 if not moves else (1 if d[a, px] > 0 else -1)
                t = ((planes[a] - o[a, px]) * (inv if moves else F(0.0))).astype(F)
                low = t < 0 if s > 0 else (~(t < 0) if s < 0 else planes[a] <= o[a, px])
                i = int(low.sum()) - 1
                ahead = np.arange(i + 1, dims[a] + 1) if s > 0 else (np.arange(i, -1, -1) if s < 0 else np.arange(0))
                ahead = ahead[(ahead >= 0) & (ahead <= dims[a])]
                ahead = ahead[t[ahead] != INF]                         # crossings at +inf are never reached
                start.append(i)
                sign.append(s)
                ts.append(t[ahead])
                axs.append(np.full(len(ahead), a))
        ts, axs = np.concatenate(ts), np.concatenate(axs)
        order = np.argsort(ts, kind="stable")                          # (equal t: the lower axis, then the order of travel)
        ts, axs = ts[order], axs[order]
        cell = [start[a] + sign[a] * np.concatenate([[0], np.cumsum(axs == a)]) for a in range(3)]
        inside = np.ones(len(ts) + 1, bool)
        for a in range(3):
            inside &= (cell[a] >= 0) & (cell[a] < dims[a])
        c = [np.clip(cell[a], 0, dims[a] - 1) for a in range(3)]
        hits = np.nonzero(inside & solid3[c[2], c[1], c[0]])[0]
        if len(hits):
            j = int(hits[0])
            t_in = F(0.0) if j == 0 else ts[j - 1]
            depth[px] = F(0.0) if t_in == 0 else t_in
            voxel[px] = (int(cell[2][j]) * dims[1] + int(cell[1][j])) * dims[0] + int(cell[0][j])
            axis[px] = 3 if j == 0 else axs[j - 1]
    return depth.reshape(h, w), voxel.reshape(h, w), axis.reshape(h, w)


def classify(view, planes, dims, solid, z_cuts=()):
    """Per-pixel counts from the flat walk: name -> pixels, for FLAGS and
      hit_zero     hits with depth bits 0x00000000 that did not start inside (axis != 3)
      hit_negzero  those of them whose crossing had t == -0.0: the -0 -> +0 rule shows
      hit_inside   hits with axis 3
      rays         pixels inside the ROI"""
    tr = trace(view, planes, dims, solid, z_cuts)
    out = {name: int(tr[name].sum()) for name in FLAGS}
    zero = (tr["voxel"] >= 0) & (tr["axis"] != 3) & (tr["depth"].view(np.uint32) == 0)
    out["hit_zero"] = int(zero.sum())
    out["hit_negzero"] = int((zero & np.signbit(tr["raw_t"])).sum())
    out["hit_inside"] = int((tr["axis"] == 3).sum())
    out["rays"] = int(RR.rays(view)[2].sum())
    return out


# ---- states ----------------------------------------------------------------------------------------------------------

RANDOM = {"random_0.3": (0.3, -0.05, 41), "random_0.03": (0.03, 0.0125, 42), "random_0.004": (0.004, 0.0, 43)}
COMMON_STATES = list(RANDOM) + ["all_solid", "empty_hull"]
STATE_NAMES = COMMON_STATES + ["corner_cut"]


def from_solid(solid):
    solid = np.asarray(solid, bool).reshape(-1)
    return np.where(solid, F(-0.5), F(0.5)).astype(F), np.ones(len(solid), np.int32), 0.0


@functools.lru_cache(maxsize=None)
def states(grid):
    """name -> (sdf, update_num, iso) for COMMON_STATES, as test_gpu_render.states_for makes them.  The random ones hold
    untouched voxels, NaNs, a count of 0 over a solid sdf, and sdf == (float)iso, which is solid iff (float)iso < iso:
    at iso -0.05 it is, at 0.0125 and 0 it is not."""
    nx, ny, nz = dims_of(grid)
    n = nx * ny * nz
    out = {}
    for name, (density, iso, seed) in RANDOM.items():
        rng = np.random.RandomState(seed)
        solid = rng.rand(n) < density
        mag = (0.1 + 0.9 * rng.rand(n)).astype(F)
        sdf = np.where(solid, -mag, mag).astype(F)
        cnt = rng.randint(1, 4, n).astype(np.int32)
        r = rng.rand(n)
        sdf[r < 0.02], cnt[r < 0.02] = LOWEST, 0
        sdf[(r >= 0.02) & (r < 0.03)] = np.nan
        sdf[(r >= 0.03) & (r < 0.032)] = F(iso)
        cnt[(r >= 0.04) & (r < 0.05)] = 0
        out[name] = (sdf, cnt, iso)
    # The eight cells round CORNER decide all of corner_in's image at this density, so they are set by hand: below the
    # plane z = -2 the two cells on the low side of x = -4 are solid and the two on the high side are not.  A ray with
    # d_x < 0 starts in an empty cell and enters a solid one through x at t == -0.0; with d_x > 0 it starts inside a solid
    # one; with d_x == 0 it reaches the solid cells above z = -2 at t == +0.0.
    sdf, cnt, _ = out["random_0.3"]
    kx, ky, kz = (CORNER[a] + (nx, ny, nz)[a] // 2 for a in range(3))
    for x, z, solid in ((kx - 1, kz - 1, True), (kx, kz - 1, False), (kx - 1, kz, True), (kx, kz, True)):
        for y in (ky - 1, ky):
            sdf[(z * ny + y) * nx + x], cnt[(z * ny + y) * nx + x] = (-0.5 if solid else 0.5), 1
    out["all_solid"] = from_solid(np.ones(n, bool))
    out["empty_hull"] = from_solid(np.zeros(n, bool))
    return out


@functools.lru_cache(maxsize=None)
def corner_cut(grid, view_name):
    """The state in which exactly the cells are solid that the paths of `view_name` through the empty grid enter and leave
    at one t between two interior brick planes: a brick jump whose tie rule is wrong lands on such a cell or hops over it."""
    cells = trace(views(grid)[view_name], planes_of(grid), dims_of(grid))["corner_cells"]
    return from_solid(cells)


def state(grid, name, view_name=None):
    return corner_cut(grid, view_name) if name == "corner_cut" else states(grid)[name]


@functools.lru_cache(maxsize=None)
def solid_of(grid, name, view_name=None):
    sdf, cnt, iso = state(grid, name, view_name)
    return RR.solid_mask(sdf, cnt, iso)


def slab_solid(solid, dims, z0, z1):
    """`solid` with every voxel outside the slices [z0, z1) cleared (slab_render_cases.slab_solid)."""
    z = np.arange(dims[0] * dims[1] * dims[2]) // (dims[0] * dims[1])
    return np.asarray(solid, bool) & (z >= z0) & (z < z1)


# the cuts of the z-slab tests: on a brick plane, off one (a slab's bricks are counted from its z0), and three slabs
CUT_SETS = {"at_8": [0, 8, 16], "at_5": [0, 5, 16], "at_5_11": [0, 5, 11, 16]}
SLAB_STATES = ["random_0.03", "corner_cut", "random_0.3"]   # (0.3: what corner_in's hits at t == -0.0 need)


@functools.lru_cache(maxsize=None)
def want(grid, view_name, state_name, own_view=None, z_range=None):
    """The restatement's (depth, voxel, axis) of a scene -- for `corner_cut`, the state of `own_view` (default: the view
    itself) --, of the whole grid or of the slab z_range: computed once."""
    own = (own_view or view_name) if state_name == "corner_cut" else None
    solid = solid_of(grid, state_name, own)
    dims = dims_of(grid)
    if z_range is not None and tuple(z_range) != (0, dims[2]):
        solid = slab_solid(solid, dims, *z_range)
    return RR.render(views(grid)[view_name], planes_of(grid), dims, solid)
