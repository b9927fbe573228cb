"""The definition of vcy_decimate_mesh (include/vacancy_hip.h, "mesh decimation") restated in numpy: cells by float32
operations one at a time, clusters and duplicate faces by np.unique over rows, member sums by one numpy add per position in
the member row (a Python loop over members), one rounding per operation."""
import numpy as np

F = np.float32
MEAN, NEAREST, FIRST = 0, 1, 2


def cell_keys(vertices, origin, cell):
    """(k int64 [n, 3], ok bool [n]): k_c = floor((p_c - origin_c) / cell); ok is the cell rule."""
    p = np.asarray(vertices, F).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d = p - np.asarray(origin, F)[None, :]
        t = d / F(cell)
        ok = np.isfinite(p) & (np.abs(t) < F(2.0 ** 30))
        k = np.where(ok, np.floor(np.where(ok, t, F(0))), F(0)).astype(np.int64)
    return k, ok.all(axis=1)


def clusters(keys):
    """(cluster [n], rep [n_clusters]): numbers by ascending lowest member index."""
    if len(keys) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    _, first, inverse = np.unique(keys, axis=0, return_index=True, return_inverse=True)
    inverse = inverse.reshape(-1)
    order = np.argsort(first, kind="stable")          # unique rows in the order of their first vertex
    rank = np.empty(len(first), np.int64)
    rank[order] = np.arange(len(first))
    return rank[inverse], first[order]


def canonical(tri):
    """Rows of three different numbers rotated so that the smallest comes first."""
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    s = np.argmin(tri, axis=1)
    idx = (s[:, None] + np.arange(3)[None, :]) % 3
    return np.take_along_axis(tri, idx, axis=1)


def member_rows(cluster, n_clusters):
    """(off [n_clusters + 1], member [n]): the row of a cluster holds its vertices in ascending index."""
    member = np.argsort(cluster, kind="stable")
    off = np.zeros(n_clusters + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(cluster, minlength=n_clusters))
    return off, member


def positions(p, off, member, rep, mode):
    n = len(rep)
    if mode == FIRST:
        return p[rep].copy()
    cnt = off[1:] - off[:-1]
    sums = np.zeros((n, 3), F)
    longest = int(cnt.max()) if n else 0
    with np.errstate(all="ignore"):
        for j in range(longest):
            m = np.nonzero(cnt > j)[0]
            sums[m] = sums[m] + p[member[off[m] + j]]
        mean = sums / cnt.astype(F)[:, None]
        if mode == MEAN:
            return mean
        best = member[off[:-1]].copy()
        dbest = None
        for j in range(longest):
            m = np.nonzero(cnt > j)[0]
            i = member[off[m] + j]
            d = p[i] - mean[m]
            sq = d * d
            dist = (sq[:, 0] + sq[:, 1]) + sq[:, 2]
            if j == 0:
                dbest = dist.copy()
                continue
            win = dist < dbest[m]
            best[m[win]] = i[win]
            dbest[m[win]] = dist[win]
    return p[best].copy()


def decimate(vertices, faces, cell, origin, mode):
    """The outputs of the definition as a dict, plus "clusters" (cluster number per input vertex), "members" (sizes of the
    clusters) and "n_noncollapsed"; None when a vertex fails the cell rule."""
    p = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if len(p) == 0 or len(f) == 0:
        return {"vertices": np.zeros((0, 3), F), "faces": np.zeros((0, 3), np.int32), "vertex_map": None, "face_source": None}
    keys, ok = cell_keys(p, origin, cell)
    if not ok.all():
        return None
    cluster, rep = clusters(keys)
    tri = cluster[f]
    alive = np.nonzero((tri[:, 0] != tri[:, 1]) & (tri[:, 1] != tri[:, 2]) & (tri[:, 2] != tri[:, 0]))[0]
    if len(alive):
        _, first = np.unique(canonical(tri[alive]), axis=0, return_index=True)
        source = alive[np.sort(first)]
    else:
        source = np.zeros(0, np.int64)
    used = np.zeros(len(rep), bool)
    used[tri[source].reshape(-1)] = True
    out_id = np.where(used, np.cumsum(used) - 1, -1)
    off, member = member_rows(cluster, len(rep))
    pos = positions(p, off, member, rep, mode)
    return {"vertices": np.ascontiguousarray(pos[used], F), "faces": out_id[tri[source]].astype(np.int32),
            "vertex_map": out_id[cluster].astype(np.int32), "face_source": source.astype(np.int32),
            "clusters": cluster, "members": off[1:] - off[:-1], "n_noncollapsed": len(alive), "keys": keys}
