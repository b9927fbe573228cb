import ctypes as C, sys, time, os
sys.path.insert(0, os.getcwd()); sys.path.insert(0, "tests")
import numpy as np
from vacancy_amd import capi, carver as vc, synth
import bunny_data as B
lib = capi.load()
def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5); views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q))); masks = B.load_masks()
    else:
        n = int(name); opt = synth.sphere_option(n); views, masks = synth.sphere_views(n, 16, 640, 480)
    d = vc.VoxelCarver(opt); assert d.Init(), vc.last_error()
    for v, m in zip(views, masks): assert d.CarveSilhouette(v, m)
    d.sync(); return d
def med(x): x = sorted(x); return "%.3f [%.3f..%.3f]" % (x[len(x)//2], x[0], x[-1])
for name in ("bunny2.5", "512", "1024"):
    d = scene(name)
    for _ in range(3): d.ExtractIsoSurface(0.0, True); d.ExtractIsoSurface(0.0, True, normals=True)
    pw, pd, nw, nd, nn, hw = [], [], [], [], [], []
    ms = C.c_float()
    for rep in range(10):
        m = capi.Mesh(); t = time.perf_counter(); assert lib.vcy_extract_iso(d.ctx, 0.0, 1, C.byref(m)) == 0; pw.append((time.perf_counter() - t) * 1e3)
        lib.vcy_last_extract_ms(d.ctx, C.byref(ms)); pd.append(ms.value)
        nv, nf = m.n_vertices, m.n_faces
        if rep < 3:
            vn = np.empty((nv, 3), np.float32); t = time.perf_counter()
            assert lib.vcy_mesh_normals_host(nv, nf, m.vertices, m.faces, vn.ctypes.data, None) == 0; hw.append((time.perf_counter() - t) * 1e3)
        lib.vcy_mesh_free(C.byref(m))
        m = capi.Mesh(); mn = capi.MeshNormals(); t = time.perf_counter()
        assert lib.vcy_extract_iso_normals(d.ctx, 0.0, 1, capi.VCY_NORMALS_VERTEX, C.byref(m), C.byref(mn)) == 0; nw.append((time.perf_counter() - t) * 1e3)
        lib.vcy_last_extract_ms(d.ctx, C.byref(ms)); nd.append(ms.value); lib.vcy_last_normals_ms(d.ctx, C.byref(ms)); nn.append(ms.value)
        lib.vcy_mesh_free(C.byref(m)); lib.vcy_mesh_normals_free(C.byref(mn))
    both = []
    for rep in range(5):
        x = d.ExtractIsoSurface(0.0, True, normals=True); both.append(x["normals_device_ms"])
    print("%s: %d vertices %d faces | vcy_extract_iso wall %s ms, device %s | vcy_extract_iso_normals(vertex) wall %s, mesh kernels %s, normals kernels %s | vertex+face normals kernels %s | vcy_mesh_normals_host (vertex only) %s ms | extract+host walk / device path = %.1f"
          % (name, nv, nf, med(pw), med(pd), med(nw), med(nd), med(nn), med(both), med(hw), (sorted(pw)[5] + sorted(hw)[1]) / sorted(nw)[5]), flush=True)
    d.close()
