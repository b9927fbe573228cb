"""The definition of vcy_smooth_mesh (include/vacancy_hip.h, "mesh smoothing") restated in numpy: rows by a stable sort of
the corners by vertex, float32 sums in row order (one numpy add per position in the row, over all vertices whose row is
that long), one rounding per operation."""
import numpy as np

F = np.float32


def rows(n_vertices, faces):
    """(off [n + 1], corners [3 * n_faces]): the row of v is corners[off[v]:off[v + 1]], corner ids 3f + j ascending."""
    flat = np.ascontiguousarray(faces, np.int64).reshape(-1)
    corners = np.argsort(flat, kind="stable")
    off = np.zeros(n_vertices + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(flat, minlength=n_vertices))
    return off, corners


def gather_rows(n_vertices, faces):
    """(off, ids [6 * n_faces]): the ids a pass gathers for v are ids[2 * off[v]:2 * off[v + 1]], in the sum's order."""
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    off, corners = rows(n_vertices, f)
    face, j = corners // 3, corners % 3
    ids = np.empty(2 * len(corners), np.int64)
    ids[0::2] = f[face, (j + 1) % 3] if len(corners) else 0
    ids[1::2] = f[face, (j + 2) % 3] if len(corners) else 0
    return off, ids


def pinned(n_vertices, faces):
    off, ids = gather_rows(n_vertices, faces)
    out = np.zeros(n_vertices, bool)
    for v in range(n_vertices):
        u, c = np.unique(ids[2 * off[v]:2 * off[v + 1]], return_counts=True)
        out[v] = bool(np.any((c == 1) & (u != v)))
    return out


def one_pass(p, off, ids, fixed, s):
    n = len(p)
    cnt = 2 * (off[1:] - off[:-1])
    sums = np.zeros((n, 3), F)
    for k in range(int(cnt.max()) if n else 0):
        m = np.nonzero(cnt > k)[0]
        sums[m] = sums[m] + p[ids[2 * off[m] + k]]
    q = p.copy()
    move = np.nonzero((cnt > 0) & ~fixed)[0]
    mean = sums[move] / cnt[move].astype(F)[:, None]
    d = mean - p[move]
    q[move] = p[move] + F(s) * d
    return q


def smooth(vertices, faces, iterations, lam, mu, pin_boundary, keep=()):
    """The positions after `iterations` iterations; `keep`: iteration counts whose positions are returned as well, as
    {count: positions}."""
    p = np.array(vertices, F).reshape(-1, 3)
    n = len(p)
    off, ids = gather_rows(n, faces)
    fixed = pinned(n, faces) if pin_boundary else np.zeros(n, bool)
    kept = {0: p.copy()} if 0 in keep else {}
    with np.errstate(all="ignore"):
        for it in range(1, iterations + 1):
            p = one_pass(p, off, ids, fixed, lam)
            p = one_pass(p, off, ids, fixed, mu)
            if it in keep:
                kept[it] = p.copy()
    return (p, kept) if keep else p
