"""numpy restatement of the ray-cast of the hull (the section "ray-cast of the hull into a view" of include/vacancy_hip.h),
float32 operation for float32 operation.  Every pixel walks its ray crossing by crossing: nothing is skipped, nothing is
searched -- start cells are COUNTED over all planes, the next crossing is the smallest (t, axis) of the three axes.  The
pixels of an image advance together, one crossing per round, which is only a way of running the per-pixel walk in numpy."""
import numpy as np

F = np.float32
INF = F(np.inf)


def grid_dims(bb_min, bb_max, resolution):
    """VoxelGrid::Init: n = (int)(diff / resolution) in float."""
    return tuple(int((F(bb_max[a]) - F(bb_min[a])) / F(resolution)) for a in range(3))


def axis_positions(bb_min, bb_max, resolution, axis, n):
    """Voxel::pos: diff * ((float)i / (float)n) + bb_min + resolution * 0.5f, left to right."""
    diff = F(bb_max[axis]) - F(bb_min[axis])
    i = np.arange(n, dtype=F)
    return (diff * (i / F(n)) + F(bb_min[axis]) + F(resolution) * F(0.5)).astype(F)


def cell_planes(bb_min, bb_max, resolution, axis):
    """n + 1 planes: midpoints of neighbouring centres in double, the outer two extrapolated by half the neighbouring
    pitch (half of `resolution` when n == 1), rounded to float."""
    n = grid_dims(bb_min, bb_max, resolution)[axis]
    p = axis_positions(bb_min, bb_max, resolution, axis, n).astype(np.float64)
    out = np.empty(n + 1, np.float64)
    out[1:n] = (p[:-1] + p[1:]) * 0.5
    lo = (p[1] - p[0]) * 0.5 if n > 1 else float(F(resolution)) * 0.5
    hi = (p[n - 1] - p[n - 2]) * 0.5 if n > 1 else float(F(resolution)) * 0.5
    out[0] = p[0] - lo
    out[n] = p[n - 1] + hi
    return out.astype(F)


def option_planes(opt):
    return [cell_planes(list(opt.bb_min), list(opt.bb_max), opt.resolution, a) for a in range(3)]


def solid_mask(sdf, cnt, iso):
    with np.errstate(invalid="ignore"):
        return (np.asarray(cnt) >= 1) & (np.asarray(sdf, F).astype(np.float64) < iso)


def rays(view):
    """World rays of every pixel, row-major: o [3, n], d [3, n] (float32) and the ROI mask [n]."""
    w, h = view.width, view.height
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    uu, vv = uu.reshape(-1), vv.reshape(-1)
    roi = (uu >= view.roi_min[0]) & (uu <= view.roi_max[0]) & (vv >= view.roi_min[1]) & (vv <= view.roi_max[1])
    m = np.array(list(view.w2c), F).reshape(3, 4)
    u, v = uu.astype(F), vv.astype(F)
    zero = np.zeros(len(u), F)
    with np.errstate(all="ignore"):
        if view.is_ortho:
            oc0, oc1, dc0, dc1 = u, v, zero, zero
        else:
            oc0, oc1 = zero, zero
            dc0 = (u - F(view.cx)) / F(view.fx)
            dc1 = (v - F(view.cy)) / F(view.fy)
        q0, q1, q2 = oc0 - m[0, 3], oc1 - m[1, 3], F(0.0) - m[2, 3]
        o = np.stack([m[0, a] * q0 + m[1, a] * q1 + m[2, a] * q2 for a in range(3)])
        d = np.stack([m[0, a] * dc0 + m[1, a] * dc1 + m[2, a] * F(1.0) for a in range(3)])
    assert o.dtype == F and d.dtype == F
    return o, d, roi


def render(view, planes, dims, solid):
    """(depth float32, voxel int64, axis uint8) images of `view` over the grid `dims` = (nx, ny, nz) with the plane
    tables `planes` and the flat boolean array `solid` in voxel-id order."""
    w, h = view.width, view.height
    n_px = w * h
    o, d, roi = rays(view)
    solid3 = np.asarray(solid, bool).reshape(dims[2], dims[1], dims[0])
    alive = roi & np.isfinite(o).all(0) & np.isfinite(d).all(0)
    T, S, I = [], [], []
    with np.errstate(all="ignore"):
        for a in range(3):
            inv = F(1.0) / d[a]
            moves = (d[a] != 0) & np.isfinite(inv)
            inv = np.where(moves, inv, F(0.0)).astype(F)
            s = np.where(moves, np.where(d[a] > 0, 1, -1), 0)
            P = planes[a]
            t = ((P[None, :] - o[a][:, None]) * inv[:, None]).astype(F)     # t_a(k) of every plane, from k
            behind = t < 0
            low = np.where((s > 0)[:, None], behind, np.where((s < 0)[:, None], ~behind, P[None, :] <= o[a][:, None]))
            T.append(t)
            S.append(s)
            I.append(low.sum(1) - 1)
    depth = np.full(n_px, INF, F)
    voxel = np.full(n_px, -1, np.int64)
    axis = np.full(n_px, 255, np.uint8)
    t_in = np.zeros(n_px, F)
    a_in = np.full(n_px, 3, np.uint8)
    px = np.arange(n_px)
    while alive.any():
        inside = np.ones(n_px, bool)
        for a in range(3):
            inside &= (I[a] >= 0) & (I[a] < dims[a])
        cx, cy, cz = (np.clip(I[a], 0, dims[a] - 1) for a in range(3))
        hit = alive & inside & solid3[cz, cy, cx]
        depth[hit] = np.where(t_in[hit] == 0, F(0.0), t_in[hit])
        voxel[hit] = (cz[hit].astype(np.int64) * dims[1] + cy[hit]) * dims[0] + cx[hit]
        axis[hit] = a_in[hit]
        alive &= ~hit
        tn = []
        for a in range(3):
            k = np.where(S[a] > 0, I[a] + 1, I[a])
            ok = (S[a] != 0) & (k >= 0) & (k <= dims[a])
            tn.append(np.where(ok, T[a][px, np.clip(k, 0, dims[a])], INF))
        tn = np.stack(tn)
        a_next = np.argmin(tn, axis=0)                  # the first minimum: ties go to the lower axis
        t_next = tn[a_next, px]
        alive &= t_next != INF                           # crossings at +inf are never reached
        for a in range(3):
            go = alive & (a_next == a)
            I[a] = np.where(go, I[a] + S[a], I[a])
        t_in = np.where(alive, t_next, t_in).astype(F)
        a_in = np.where(alive, a_next, a_in).astype(np.uint8)
    return depth.reshape(h, w), voxel.reshape(h, w), axis.reshape(h, w)


def agreement(view, voxel_image, mask):
    """The three counts of vcy_hull_agreement from a voxel-id image and a silhouette."""
    h, w = voxel_image.shape
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    roi = (uu >= view.roi_min[0]) & (uu <= view.roi_max[0]) & (vv >= view.roi_min[1]) & (vv <= view.roi_max[1])
    m, hull = (np.asarray(mask) != 0) & roi, (voxel_image >= 0) & roi
    return [int((m & hull).sum()), int((m & ~hull).sum()), int((~m & hull).sum())]
