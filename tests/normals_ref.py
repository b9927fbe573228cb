"""numpy float32 restatement of the reference's Mesh::CalcFaceNormal + Mesh::CalcNormal (src/vacancy/mesh.cc:197-240),
the yardstick of the normals tests.  Written from the reference text, independent of the library under test:

  face i = (f0, f1, f2):  v1 = (p[f1] - p[f0]).normalized(), v2 = (p[f2] - p[f0]).normalized(),
                          fn[i] = v1.cross(v2).normalized()
  vertex k:               n = 0; for faces in ascending index, corners j = 0, 1, 2: if the corner is k: n += fn[i], count++
                          n /= float(count); n.normalize()

with Eigen's fixed-size evaluation as include/vacancy/linalg.h restates it: squaredNorm = x*x + (y*y + z*z),
normalized() = n2 > 0 ? v / sqrt(n2) : v, true division per component.  Every operation below is one float32 numpy
operation (correctly rounded, no contraction), so the bits are those of the scalar code.
"""
import numpy as np

F = np.float32


def _normalized(v):
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    n2 = x * x + (y * y + z * z)
    pos = n2 > 0
    n = np.sqrt(np.where(pos, n2, F(1)))
    out = v.copy()
    out[pos] = v[pos] / n[pos, None]
    return out


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                     a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def face_normals(vertices, faces):
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros((0, 3), F)
    p0 = v[f[:, 0]]
    v1 = _normalized(v[f[:, 1]] - p0)
    v2 = _normalized(v[f[:, 2]] - p0)
    fn = _normalized(_cross(v1, v2))
    assert fn.dtype == F
    return fn


def mesh_normals(vertices, faces):
    """(vertex normals, face normals), float32.  Asserts what makes a comparison of bits well defined: finite positions,
    every vertex named by a face (count >= 1), no NaN in the result."""
    v = np.ascontiguousarray(vertices, F).reshape(-1, 3)
    f = np.ascontiguousarray(faces, np.int64).reshape(-1, 3)
    assert np.isfinite(v).all(), "positions must be finite"
    fn = face_normals(v, f)
    nv = len(v)
    if nv == 0:
        assert len(f) == 0
        return np.zeros((0, 3), F), fn
    # the (face, corner) pairs in the order the reference adds them, grouped by vertex: a stable sort by vertex id keeps
    # ascending face index (and corner order inside a face) within each vertex
    corner_vertex = f.reshape(-1)
    corner_face = np.repeat(np.arange(len(f), dtype=np.int64), 3)
    order = np.argsort(corner_vertex, kind="stable")
    cv, cf = corner_vertex[order], corner_face[order]
    count = np.bincount(cv, minlength=nv)
    assert (count >= 1).all(), "every vertex must be named by a face"
    start = np.concatenate([[0], np.cumsum(count)[:-1]])
    n = np.zeros((nv, 3), F)
    # rank by rank: the r-th addend of every vertex that has one (the valence of a marching-cubes vertex is small)
    for r in range(int(count.max())):
        has = np.nonzero(count > r)[0]
        n[has] = n[has] + fn[cf[start[has] + r]]
    n = n / count.astype(F)[:, None]
    n = _normalized(n)
    assert n.dtype == F and not np.isnan(n).any() and not np.isnan(fn).any()
    return n, fn


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)
