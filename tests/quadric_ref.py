"""The definition of vcy_decimate_mesh_quadric (include/vacancy_hip.h, "mesh decimation, quadric representatives") restated
in numpy: cells, clusters, member rows and the mean from decimate_ref; the quadrics in float64, one numpy operation -- one
rounding -- at a time, the two levels of sums by one numpy add per position in the corner row and in the member row."""
import numpy as np

import decimate_ref as DR

F = np.float32
D = np.float64


def face_quadrics(p, tri, m):
    """q(f) [k, 9] of the faces tri [k, 3] over positions p (float32), each seen from its row of m (float32 [k, 3])."""
    m = m.astype(D)
    a, b, c = (p[tri[:, j]].astype(D) - m for j in range(3))
    e, g = b - a, c - a
    nx = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1]
    ny = e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2]
    nz = e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
    d = -((nx * a[:, 0] + ny * a[:, 1]) + nz * a[:, 2])
    return np.stack([nx * nx, nx * ny, nx * nz, ny * ny, ny * nz, nz * nz, nx * d, ny * d, nz * d], axis=-1)


def vertex_quadrics(p, f, cluster, mean):
    """Qv [n, 9]: through every vertex's corner row (ascending face, then corner), seen from its cluster's mean."""
    n = len(p)
    flat = f.reshape(-1)
    corner = np.argsort(flat, kind="stable")                 # corners 3 f + j, by vertex, ascending within a vertex
    cnt = np.bincount(flat, minlength=n)
    off = np.concatenate([[0], np.cumsum(cnt)])
    qv = np.zeros((n, 9), D)
    for j in range(int(cnt.max()) if n else 0):
        v = np.nonzero(cnt > j)[0]
        face = corner[off[v] + j] // 3
        qv[v] = qv[v] + face_quadrics(p, f[face], mean[cluster[v]])
    return qv


def cluster_quadrics(qv, off, member):
    cnt = off[1:] - off[:-1]
    q = np.zeros((len(cnt), 9), D)
    for j in range(int(cnt.max()) if len(cnt) else 0):
        c = np.nonzero(cnt > j)[0]
        q[c] = q[c] + qv[member[off[c] + j]]
    return q


def solve_or_mean(q, mean, regularize, origin, cell, keys_of_clusters):
    """(positions float32 [n, 3], fallback bool [n])."""
    with np.errstate(all="ignore"):
        t = (q[:, 0] + q[:, 3]) + q[:, 5]
        w = D(F(regularize)) * t
        a00, a11, a22, a01, a02, a12 = q[:, 0] + w, q[:, 3] + w, q[:, 5] + w, q[:, 1], q[:, 2], q[:, 4]
        r0, r1, r2 = -q[:, 6], -q[:, 7], -q[:, 8]
        d0 = a00
        l10 = a01 / d0
        l20 = a02 / d0
        d1 = a11 - l10 * a01
        u = a12 - l20 * a01
        l21 = u / d1
        d2 = (a22 - l20 * a02) - l21 * u
        y0 = r0
        y1 = r1 - l10 * y0
        y2 = (r2 - l20 * y0) - l21 * y1
        z0, z1, z2 = y0 / d0, y1 / d1, y2 / d2
        x2 = z2
        x1 = z1 - l21 * x2
        x0 = (z0 - l10 * x1) - l20 * x2
        pos = (mean.astype(D) + np.stack([x0, x1, x2], axis=-1)).astype(F)
        good = np.isfinite(t) & (t > 0) & (d0 > 0) & (d1 > 0) & (d2 > 0) & np.isfinite(pos).all(axis=1)
        keys, ok = DR.cell_keys(np.where(good[:, None], pos, F(0)), origin, cell)
        good &= ok & (keys == keys_of_clusters).all(axis=1)
    return np.where(good[:, None], pos, mean), ~good


def decimate(vertices, faces, cell, origin, regularize):
    """decimate_ref.decimate with MEAN, the positions replaced; plus "n_fallback", "fallback" (per output vertex), "mean"
    (the MEAN positions of the output vertices)."""
    out = DR.decimate(vertices, faces, cell, origin, DR.MEAN)
    if out is None or out["vertex_map"] is None:
        if out is not None:
            out["n_fallback"] = 0
        return out
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    cluster = out["clusters"]
    n_clusters = len(out["members"])
    off, member = DR.member_rows(cluster, n_clusters)
    rep = member[off[:-1]]
    mean = DR.positions(p, off, member, rep, DR.MEAN)
    q = cluster_quadrics(vertex_quadrics(p, f, cluster, mean), off, member)
    pos, fallback = solve_or_mean(q, mean, regularize, origin, cell, out["keys"][rep])
    used = np.zeros(n_clusters, bool)
    used[cluster[out["vertex_map"] >= 0]] = True               # the clusters that became output vertices, in cluster order
    assert np.array_equal(out["vertices"].view(np.uint32), mean[used].view(np.uint32))
    out["mean"] = out["vertices"]
    out["vertices"] = np.ascontiguousarray(pos[used], F)
    out["fallback"] = fallback[used]
    out["n_fallback"] = int(fallback[used].sum())
    return out
