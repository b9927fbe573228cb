"""The slab stitch as vacancy_amd.dist.merge_meshes computed it in numpy before vcy_merge_meshes_host existed, kept unchanged
as the yardstick of tests/test_merge_meshes_host.py.  Nothing outside tests/ may import it."""
import numpy as np


def merge_meshes(meshes):
    """Stitches per-slab meshes (in slab order) into the mesh a single-GPU extraction returns.

    A slab's first n_foreign vertices duplicate vertices owned by the slab below (edges on the
    shared plane); they are dropped and the faces that use them are re-pointed by edge key.  Own
    vertices keep their order, so the result is vertex-for-vertex the serial scan's numbering.

    Parts that all carry "normals", "face_normals" and "layer_faces" (VoxelCarver.ExtractIsoSurfaceSlab) give
    "normals" and "face_normals" of the merged mesh as well, bit-equal to Mesh::CalcNormal of it: the slabs' normals
    concatenated with the merged numbering (foreign entries dropped), then per seam the seam finish
    (vcy_mesh_normals_seam_sum, on the host, over the slabs' own face normals) for the vertices the upper slab's foreign vertices were mapped to, over
    the faces of the lower slab's last and the upper slab's first cell layer.  Without those keys the result has
    exactly the three arrays above.
    """
    with_normals = bool(meshes) and all("normals" in m and "face_normals" in m and "layer_faces" in m for m in meshes)
    verts, keys, faces, vnorm, fnorm, seams = [], [], [], [], [], []
    offset = face_offset = 0
    prev_keys, prev_offset = np.zeros((0, 2), np.int64), 0
    prev_last_layer = 0
    for m in meshes:
        nf_ = int(m["n_foreign"])
        v, k, f = m["vertices"], m["keys"], m["faces"]
        nown = len(v) - nf_
        remap = np.empty(len(v), np.int64)
        if nf_:
            # only vertices on the previous slab's top plane can be referenced: its keys within the range of the foreign ones
            lo, hi = k[:nf_, 0].min(), k[:nf_, 1].max()
            cand = np.nonzero((prev_keys[:, 0] >= lo) & (prev_keys[:, 1] <= hi))[0]
            prev_key_to_gid = {(int(prev_keys[i, 0]), int(prev_keys[i, 1])): prev_offset + int(i) for i in cand}
        for i in range(nf_):
            remap[i] = prev_key_to_gid[(int(k[i, 0]), int(k[i, 1]))]
        remap[nf_:] = offset + np.arange(nown)
        verts.append(v[nf_:])
        keys.append(k[nf_:])
        faces.append(remap[f] if len(f) else f.astype(np.int64))
        if with_normals:
            vnorm.append(m["normals"][nf_:])
            fnorm.append(m["face_normals"])
            if nf_:
                seams.append((face_offset - prev_last_layer, face_offset + int(m["layer_faces"][0]), remap[:nf_].copy()))
            prev_last_layer = int(m["layer_faces"][1])
        prev_keys, prev_offset = k[nf_:], offset
        offset += nown
        face_offset += len(f)
    out = {
        "vertices": np.concatenate(verts) if verts else np.zeros((0, 3), np.float32),
        "keys": np.concatenate(keys) if keys else np.zeros((0, 2), np.int64),
        "faces": (np.concatenate(faces) if faces else np.zeros((0, 3), np.int64)).astype(np.int32),
    }
    if with_normals:
        out["normals"] = np.ascontiguousarray(np.concatenate(vnorm), np.float32)
        out["face_normals"] = np.ascontiguousarray(np.concatenate(fnorm), np.float32)
        from vacancy_amd import carver as _vc
        for begin, end, ids in seams:
            _vc.mesh_normals_seam_sum(len(out["vertices"]), out["faces"], out["face_normals"], begin, end, ids, out["normals"])
    return out
