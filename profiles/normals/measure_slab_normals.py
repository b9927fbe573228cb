"""Wall time of ShardedVoxelCarver.ExtractIsoSurface(normals=True) on ONE device with 2, 4 and 8 z-slabs, and the host
time of the seam finish per seam.

    python profiles/normals/measure_slab_normals.py [--tree DIR] [--label TEXT] [--scenes bunny2.5,512,1024]

--tree: the checkout whose vacancy_amd (with its built library) is measured -- this one by default, a checkout of the
parent commit for the other column.  Scenes and carve as profiles/normals/measure_normals.py: the bunny's six views at
resolution 2.5, a sphere from 16 views at 512^3 and 1024^3.  10 calls after 3 of warm-up, median [min..max] in ms.
"""
import argparse
import os
import socket
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=os.getcwd())
ap.add_argument("--label", default="")
ap.add_argument("--scenes", default="bunny2.5,512,1024")
ap.add_argument("--slabs", default="2,4,8")
args = ap.parse_args()
tree = os.path.abspath(args.tree)
sys.path.insert(0, tree)
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))

import numpy as np  # noqa: E402,F401
import bunny_data as B  # noqa: E402
from vacancy_amd import capi, carver as vc, sharded, synth  # noqa: E402

assert os.path.abspath(capi.LIB_PATH).startswith(tree), capi.LIB_PATH
lib = capi.load()


def med(x):
    x = sorted(x)
    return "%.3f [%.3f..%.3f]" % (x[len(x) // 2], x[0], x[-1])


def scene(name):
    if name == "bunny2.5":
        opt = B.bunny_option(2.5)
        views = B.bunny_views(lambda t, q: synth.affine_inverse(synth.pose_from_tum(t, q)))
        masks = B.load_masks()
    else:
        n = int(name)
        opt = synth.sphere_option(n)
        views, masks = synth.sphere_views(n, 16, 640, 480)
    return opt, views, masks


seam_ms = []
if hasattr(vc, "mesh_normals_host_seam"):
    inner = vc.mesh_normals_host_seam

    def timed(*a, **kw):
        t = time.perf_counter()
        r = inner(*a, **kw)
        seam_ms.append((time.perf_counter() - t) * 1e3)
        return r

    vc.mesh_normals_host_seam = timed

print("box %s | %s | %s | tree %s" % (socket.gethostname(), lib.vcy_version().decode(), args.label, tree))
for name in args.scenes.split(","):
    opt, views, masks = scene(name)
    for slabs in [int(s) for s in args.slabs.split(",")]:
        sh = sharded.ShardedVoxelCarver(opt, devices=[0], slabs_per_device=slabs)
        assert sh.Init(), vc.last_error()
        for c in sh.slabs:
            for v, m in zip(views, masks):
                assert c.CarveSilhouette(v, m), vc.last_error()
        sh.sync()
        for _ in range(3):
            mesh = sh.ExtractIsoSurface(0.0, True, normals=True)
        del seam_ms[:]
        wall, dev = [], []
        for _ in range(10):
            t = time.perf_counter()
            mesh = sh.ExtractIsoSurface(0.0, True, normals=True)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(mesh.get("normals_device_ms", 0.0))
        plain = []
        for _ in range(5):
            t = time.perf_counter()
            sh.ExtractIsoSurface(0.0, True)
            plain.append((time.perf_counter() - t) * 1e3)
        print("%s: %d slabs: %d vertices %d faces | ExtractIsoSurface(normals=True) wall %s ms | without normals %s ms | "
              "normals kernels, sum over slabs %s ms | seam finish on the host, per seam %s"
              % (name, slabs, len(mesh["vertices"]), len(mesh["faces"]), med(wall), med(plain), med(dev),
                 (med(seam_ms) + " ms (%d calls)" % len(seam_ms)) if seam_ms else "n/a (host walk over the merged mesh)"))
        sys.stdout.flush()
        sh.close()
