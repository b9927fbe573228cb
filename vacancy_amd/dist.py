"""z-slab sharding of the voxel grid across the GPUs of one node (one process per GPU).

Carving needs no communication: voxels are independent (reference voxel_carver.cc:442-491
touches only its own voxel) and z is the slowest index, so a contiguous z-range is one slab of
HBM.  The grid is cut into S = world * k slabs and slab s belongs to rank s % world (cyclic).  With view
dropping the slabs through the object cost 1.6x the outer ones; the cuts are therefore placed where
the slab planner predicts equal COST (plan_bounds -> vcy_plan_z_slabs), one slab per rank -- round 3
paired an outer with a central slab of equal thickness instead (k = 2), which doubles the fixed cost
per launch and still left the ranks 5 % apart.
Marching cubes needs the two slices below each slab: ONE all-gather of every slab's last two
slices (RCCL when the backend is nccl), after which every slab is extracted on its own GPU.
The per-slab meshes are stitched on the host by edge key (merge_meshes).
Connected components of the hull are labelled per slab on its GPU; one plane of labels per seam and the lists of label
pairs travel, and every rank joins the pieces on the host (label_components_slabs, merge_components).
"""
import ctypes as C

import numpy as np


def slab_range(nz, index, count):
    """Contiguous z-range of slab `index` of `count`; the first nz % count slabs get one extra."""
    base, rem = divmod(nz, count)
    z0 = index * base + min(index, rem)
    z1 = z0 + base + (1 if index < rem else 0)
    return z0, z1


def slabs_of_rank(nz, rank, world, k=1, bounds=None):
    """[(slab_id, z0, z1)] owned by `rank` under the cyclic distribution.  `bounds` (world * k + 1 cuts, e.g. from
    plan_bounds): slabs of equal predicted COST instead of equal thickness."""
    count = world * k
    if bounds is not None:
        assert len(bounds) == count + 1 and bounds[0] == 0 and bounds[-1] == nz, (bounds, count, nz)
        return [(s, int(bounds[s]), int(bounds[s + 1])) for s in range(rank, count, world)]
    return [(s, *slab_range(nz, s, count)) for s in range(rank, count, world)]


def equal_bounds(nz, count):
    return [slab_range(nz, s, count)[0] for s in range(count)] + [nz]


def plan_bounds(option, device_id, views, sdf_host_images, count, stride=0, brick_cost=0.0):
    """Cuts for `count` z-slabs of equal predicted carve cost for these views (vcy_plan_z_slabs), computed on
    `device_id` with a small planning context that is destroyed again.  Deterministic: every rank of a job that calls
    this with the same inputs gets the same cuts.  Returns (bounds, layer_cost, info)."""
    import time
    import warnings
    from . import carver as vc
    t0 = time.perf_counter()
    p = vc.VoxelCarver(option, device_id=device_id, z_range=(0, 8))
    if not p.Init():
        raise RuntimeError("vcy_create failed (planning context): " + vc.last_error())
    nz = p.dims[2]
    try:
        uniq, ptrs = {}, []
        for img in sdf_host_images:  # (the same array object for several views is uploaded once)
            if id(img) not in uniq:
                uniq[id(img)] = p.upload_sdf(img)
            ptrs.append(uniq[id(img)])
        t1 = time.perf_counter()
        why = None
        try:
            bounds, cost = p.plan_z_slabs(views, ptrs, count, stride=stride, brick_cost=brick_cost)
            if any(b1 - b0 < 2 for b0, b1 in zip(bounds[:-1], bounds[1:])):
                why = "planned cuts %s leave a slab of fewer than 2 slices" % (bounds,)
        except RuntimeError as e:  # (the planner cuts at whole brick layers: nz = 32 cannot give 8 planned slabs)
            why = str(e)
        t2 = time.perf_counter()
        for d in uniq.values():
            p.free_device(d)
    finally:
        p.close()
    if why is not None:
        # slabs of equal thickness always exist when nz >= 2 * count; say so instead of failing the whole job
        warnings.warn("slab planner: %s -- falling back to slabs of equal thickness" % why)
        return equal_bounds(nz, count), None, {"plan_ms": round((t2 - t1) * 1e3, 3), "fallback": "equal thickness",
                                               "reason": why[:200], "in_timed_region": False}
    parts = [float(cost[bounds[s] // 8:(bounds[s + 1] + 7) // 8].sum()) for s in range(count)]
    mean = sum(parts) / max(1, count)
    info = {"plan_ms": round((t2 - t1) * 1e3, 3), "setup_ms": round((t1 - t0) * 1e3, 3),
            "predicted_cost_share": [round(x / (mean * count), 4) for x in parts],
            "predicted_spread": round((max(parts) - min(parts)) / mean, 4) if mean > 0 else 0.0,
            # once per view set, before the timed steps (a camera rig that stays put is planned once)
            "in_timed_region": False}
    return bounds, cost, info


def _pack_offset(slab_id, world, k, nbytes):
    """Offset of slab `slab_id`'s pack in the rank-major all-gather output."""
    rank, kk = slab_id % world, slab_id // world
    return (rank * k + kk) * nbytes


def exchange_halo(carvers, rank, world):
    """carvers: this rank's slab contexts ordered by slab id (slab ids rank, rank+world, ...).
    Installs, for every slab but the first of the grid, the last two slices of the slab below.
    Returns what the exchange was, for the benchmark record: {"backend", "ranks", "bytes_per_rank", "op"}
    (None when there is a single slab and nothing to exchange)."""
    if not isinstance(carvers, (list, tuple)):
        carvers = [carvers]
    k = len(carvers)
    lib = carvers[0]._lib
    if world * k == 1:
        return None
    nbytes = int(lib.vcy_halo_bytes(carvers[0].ctx))
    slab_ids = [rank + i * world for i in range(k)]
    if world == 1:
        # all slabs live in this process: the library's own RCCL all-gather (one communicator rank per
        # distinct device, vcy_halo_allgather)
        if hasattr(lib, "vcy_halo_allgather"):
            from . import carver as _vc
            return _vc.halo_exchange(carvers)  # (peer copies, and says so, if librccl cannot be loaded)
        packs = [c.halo_pack_host() for c in carvers]  # host stand-ins of the CPU tests
        for i, c in enumerate(carvers):
            if slab_ids[i] > 0:
                c.halo_install_host(packs[i - 1])
        return {"backend": "host", "op": "copy", "ranks": 1, "bytes_per_rank": nbytes * k}
    import torch
    import torch.distributed as dist

    on_gpu = dist.get_backend() == "nccl"
    version = None
    if on_gpu:
        try:  # (2, 22, 7)-like: the RCCL build behind torch's nccl backend
            version = ".".join(str(x) for x in torch.cuda.nccl.version())
        except Exception:  # noqa: BLE001
            version = None
    result = {"backend": "rccl (torch.distributed nccl)" if on_gpu else "gloo (host staging)", "version": version,
              "op": "all_gather_into_tensor" if on_gpu else "all_gather", "ranks": dist.get_world_size(),
              "bytes_per_rank": nbytes * k, "bytes_received_per_rank": nbytes * k * dist.get_world_size(),
              "bytes_needed_per_slab": nbytes, "slabs_per_rank": k}
    if on_gpu:
        send = torch.empty(nbytes * k, dtype=torch.uint8, device="cuda")
        recv = torch.empty(nbytes * k * world, dtype=torch.uint8, device="cuda")
        for i, c in enumerate(carvers):
            rc = lib.vcy_halo_pack(c.ctx, C.c_void_p(send.data_ptr() + i * nbytes))
            assert rc == 0, lib.vcy_last_error()
            c.sync()
        dist.all_gather_into_tensor(recv, send)   # the single RCCL collective of the path
        torch.cuda.synchronize()
        for i, c in enumerate(carvers):
            s = slab_ids[i]
            if s > 0:
                off = _pack_offset(s - 1, world, k, nbytes)
                rc = lib.vcy_halo_install(c.ctx, C.c_void_p(recv.data_ptr() + off))
                assert rc == 0, lib.vcy_last_error()
                c.sync()
    else:
        # gloo (CPU tests / several ranks on one GPU): stage the same bytes through the host
        send = torch.from_numpy(np.concatenate([c.halo_pack_host() for c in carvers]))
        parts = [torch.empty_like(send) for _ in range(world)]
        dist.all_gather(parts, send)
        flat = np.concatenate([p.numpy() for p in parts])
        for i, c in enumerate(carvers):
            s = slab_ids[i]
            if s > 0:
                off = _pack_offset(s - 1, world, k, nbytes)
                c.halo_install_host(flat[off:off + nbytes])
    return result


def carve_silhouettes_sharded(carvers, rank, world, views, silhouettes, chunk=32):
    """Carve(vector<Camera>, vector<Image1b>) (voxel_carver.cc:516-528 around :394-413) in a one-process-per-GPU job:
    the ranks SHARE the producer.  Per chunk of `chunk` views rank r uploads and transforms the silhouettes r, r + world,
    ... (vcy_make_sdf_batch_device, its share only), ONE all-gather (RCCL when the backend is nccl) hands every rank all
    the SDF images of the chunk (W * H * 4 bytes each), and the rank's slabs carve them in one fused launch; the carve
    of chunk i is queued asynchronously, so chunk i + 1 is produced and gathered while it runs.  Every rank passes the
    SAME views and silhouettes.  Results are those of CarveBatchSilhouettes on every slab (every rank building every
    SDF), which is what round 4 did and what left the streamed path producer-bound at 8 GPUs.
    Returns {"producer_ms", "gather_ms", "carve_enqueue_ms", "wall_ms"} of this rank (host clock)."""
    import time
    import torch
    import torch.distributed as dist
    from .carver import VoxelCarver

    if not isinstance(carvers, (list, tuple)):
        carvers = [carvers]
    c0 = carvers[0]
    n = len(views)
    on_gpu = world > 1 and dist.get_backend() == "nccl"
    dev = torch.device("cuda", c0._device) if torch.cuda.is_available() else None
    max_px = max(v.width * v.height for v in views)
    stride = (max_px + 63) // 64 * 64  # floats per image slot
    per = (min(chunk, n) + world - 1) // world
    t_all = time.perf_counter()
    t_prod = t_gather = t_carve = 0.0
    # two sets of gathered images: chunk i + 1 is gathered while chunk i is still being carved
    recv = [torch.empty(world * per * stride, dtype=torch.float32, device=dev) for _ in range(2)]
    send = torch.empty(per * stride, dtype=torch.float32, device=dev)
    for ci, first in enumerate(range(0, n, chunk)):
        m = min(chunk, n - first)
        rv = recv[ci & 1]
        if ci >= 2:
            for c in carvers:
                c.sync()  # the launches of chunk ci - 2 read this set
        t0 = time.perf_counter()
        mine = list(range(rank, m, world))
        if mine:
            # (vcy_make_sdf_batch_device returns with the images complete: it waits for the context's stream.  A job of ONE
            # rank builds them in place in the set the carve reads -- there is nothing to exchange, and a device copy on
            # torch's stream would be ordered against neither the carvers' own streams nor the next chunk's producer)
            target = rv if world == 1 else send
            outs = [target.data_ptr() + 4 * k * stride for k in range(len(mine))]
            ok = c0.make_sdf_batch_into([views[first + j] for j in mine], [silhouettes[first + j] for j in mine], outs)
            if not ok:
                from .carver import last_error
                raise RuntimeError("vcy_make_sdf_batch_device: " + last_error())
        t1 = time.perf_counter()
        if world == 1:
            pass  # built in place, above
        elif on_gpu:
            torch.cuda.current_stream().synchronize()
            dist.all_gather_into_tensor(rv, send)  # the exchange step of the streamed path
            torch.cuda.synchronize()
        else:  # gloo (CPU rendezvous / several ranks on one GPU): the same bytes through the host
            h = send.cpu()
            parts = [torch.empty_like(h) for _ in range(world)]
            dist.all_gather(parts, h)
            rv.copy_(torch.cat(parts).to(rv.device))
            if dev is not None:
                torch.cuda.synchronize()
        t2 = time.perf_counter()
        ptrs = [C.c_void_p(rv.data_ptr() + 4 * ((j % world) * per + j // world) * stride) for j in range(m)]
        batch = VoxelCarver.prepare_batch(views[first:first + m], ptrs)
        for c in carvers:
            if not c.CarveBatchDevice(batch):
                from .carver import last_error
                raise RuntimeError(last_error())
        t3 = time.perf_counter()
        t_prod, t_gather, t_carve = t_prod + (t1 - t0), t_gather + (t2 - t1), t_carve + (t3 - t2)
    for c in carvers:
        c.sync()
    return {"producer_ms": t_prod * 1e3, "gather_ms": t_gather * 1e3, "carve_enqueue_ms": t_carve * 1e3,
            "wall_ms": (time.perf_counter() - t_all) * 1e3, "views_built_by_this_rank": len(range(rank, n, world)) if chunk >= n
            else sum(len(range(rank, min(chunk, n - f), world)) for f in range(0, n, chunk))}


def merged_mesh_check(my_meshes, my_slab_ids, rank, world, n_slabs, reference_fn, barrier, tag=None):
    """The slabs' meshes of a one-node job merged by edge key and compared, array for array, with the mesh of ONE context
    holding the whole grid (`reference_fn()`, called on rank 0 only).  The meshes travel through files in shared memory
    (a pickle through the collective backend would serialise them into device tensors under nccl); `barrier()` must
    synchronise the ranks (bench.py: device sync + dist.barrier).  Returns the comparison on rank 0, None elsewhere.
    What `bench.py --gpus N` runs on a small grid BEFORE its timed region, so that the first record a multi-GPU node
    produces says by itself whether the exchange + merge gave the single-GPU mesh."""
    import os
    import shutil
    base = "/dev/shm" if os.path.isdir("/dev/shm") else "/tmp"
    tag = tag or os.path.join(base, "vcy_verify_%s_%s" % (os.environ.get("MASTER_PORT", "0"), os.getuid()))
    os.makedirs(tag, exist_ok=True)
    for sid, m in zip(my_slab_ids, my_meshes):
        np.savez(os.path.join(tag, "slab_%d.npz" % sid), vertices=m["vertices"], faces=m["faces"], keys=m["keys"],
                 n_foreign=np.int64(m["n_foreign"]))
    barrier()
    check = None
    if rank == 0:
        parts = []
        for sid in range(n_slabs):
            z = np.load(os.path.join(tag, "slab_%d.npz" % sid))
            parts.append({"vertices": z["vertices"], "faces": z["faces"], "keys": z["keys"], "n_foreign": int(z["n_foreign"])})
        merged, ref = merge_meshes(parts), reference_fn()
        same = (merged["vertices"].shape == ref["vertices"].shape and merged["faces"].shape == ref["faces"].shape
                and np.array_equal(merged["vertices"].view(np.uint32), ref["vertices"].view(np.uint32))
                and np.array_equal(merged["faces"], ref["faces"]) and np.array_equal(merged["keys"], ref["keys"]))
        check = {"merged_equals_single_context": bool(same), "vertices": int(len(merged["vertices"])),
                 "faces": int(len(merged["faces"])), "single_context_vertices": int(len(ref["vertices"])),
                 "single_context_faces": int(len(ref["faces"])), "slabs": int(n_slabs),
                 "note": "slab meshes merged by edge key (vacancy_amd.dist.merge_meshes) against one context holding the "
                         "whole grid on rank 0's device: vertex bits, faces and edge keys, array for array"}
    barrier()
    if rank == 0:
        shutil.rmtree(tag, ignore_errors=True)
    return check


def merge_meshes(meshes):
    """Stitches per-slab meshes (dicts of ExtractIsoSurface / ExtractIsoSurfaceSlab, in slab order) into the mesh a
    single-GPU extraction returns: {"vertices", "keys", "faces"}, and "normals" and "face_normals" as well when every
    part carries "normals", "face_normals" and "layer_faces".  One call of vcy_merge_meshes_host; the rule and its errors
    (RuntimeError) are stated in include/vacancy_hip.h."""
    from . import carver as _vc
    keys = ["vertices", "faces", "keys", "n_foreign"]
    if meshes and all("normals" in m and "face_normals" in m and "layer_faces" in m for m in meshes):
        keys += ["normals", "face_normals", "layer_faces"]
    return _vc.merge_meshes_host(*[[m[k] for m in meshes] for k in keys])


# ---- connected components of a grid in z-slabs (the order of the calls: include/vacancy_hip.h) ----------------------

def merge_components(lists, pairs):
    """The seam merge on the host (vcy_merge_components_host, no GPU): `lists` = every slab's LabelComponentsSlab dict
    in z order, `pairs` = per seam the int64 [n, 2] array of (label below, label above), duplicates allowed.  Returns
    (the merged list as VoxelCarver.LabelComponents returns it, [per slab: the merged label of each of its pieces])."""
    from . import carver as _vc
    return _vc.merge_components_host(lists, pairs)


def _each(carvers, fn):
    return [fn(i, c) for i, c in enumerate(carvers)]


def _gather_by_slab(mine, world):
    """{slab id: object} of every rank joined into one dict on every rank (Python objects through the process group)."""
    if world == 1:
        return dict(mine)
    import torch.distributed as dist
    parts = [None] * world
    dist.all_gather_object(parts, mine)
    out = {}
    for part in parts:
        out.update(part)
    return out


def label_components_slabs(carvers, rank=0, world=1, iso_level=0.0, each=_each):
    """LabelComponents of a grid cut into z-slabs.  `carvers`: this rank's slab contexts ordered by slab id (slab ids
    rank, rank + world, ...; one process holding every slab: rank 0 of 1).  Every slab labels its own slices on its
    device; the lists, the slabs' top planes of labels (nx * ny int64 per seam) and the seams' pair lists are gathered
    as Python objects -- never a slab's label volume --, every rank runs the same host merge and installs its slabs'
    maps, so that download_labels() on a slab returns merged labels.  `each(carvers, fn)` runs fn(i, carver) for
    every local slab and returns the results in order (ShardedVoxelCarver: a host thread per device).
    Returns {"merged": the list as VoxelCarver.LabelComponents returns it, "lists", "maps": per slab of the GRID,
    "device_ms": the sum over this rank's slabs}."""
    k = len(carvers)
    ids = [rank + i * world for i in range(k)]
    count = world * k
    ms = [0.0] * k

    def label(i, c):
        part = c.LabelComponentsSlab(iso_level)
        ms[i] += part.pop("device_ms")
        return part, (c.component_top_plane() if ids[i] + 1 < count else None)

    labelled = _gather_by_slab(dict(zip(ids, each(carvers, label))), world)

    def seam(i, c):
        if ids[i] == 0:
            return None
        pairs = c.component_seam_pairs(labelled[ids[i] - 1][1])
        ms[i] += c.last_components_ms()
        return pairs

    seams = _gather_by_slab(dict(zip(ids, each(carvers, seam))), world)
    lists = [labelled[s][0] for s in range(count)]
    merged, maps = merge_components(lists, [seams[s] for s in range(1, count)])
    each(carvers, lambda i, c: c.resolve_components(lists[ids[i]]["label"], maps[ids[i]]))
    return {"merged": merged, "lists": lists, "maps": maps, "device_ms": float(sum(ms))}


def select_components(merged, largest, min_voxels, maps=()):
    """vcy_select_components_host (no GPU), the keep rule of vcy_keep_components: `merged` a list as LabelComponents returns
    it, `maps` per slab the merged label of each of its pieces (merge_components).  Returns (bool per component: it goes,
    [bool per piece of slab s: it goes], removed components, removed voxels)."""
    from . import capi, carver as _vc
    flat = np.zeros(len(merged["label"]), _vc._COMPONENT_REC)
    for key in flat.dtype.names:
        flat[key] = merged[key]
    glob = np.ascontiguousarray(np.concatenate([np.zeros(0, np.int64)] + list(maps)), np.int64)
    gone, pieces = np.zeros(len(flat), np.uint8), np.zeros(len(glob), np.uint8)
    nc, nv = C.c_int64(0), C.c_int64(0)
    rc = capi.load().vcy_select_components_host(_vc._p(flat), len(flat), int(largest), int(min_voxels), _vc._p(gone),
                                                C.byref(nc), C.byref(nv), _vc._p(glob), len(glob), _vc._p(pieces))
    if rc != 0:
        _vc._raise_rc(rc)
    ends = np.cumsum([len(m) for m in maps], dtype=np.int64)
    return gone != 0, [pieces[e - len(m):e] != 0 for e, m in zip(ends, maps)], nc.value, nv.value


def keep_components_slabs(carvers, rank=0, world=1, iso_level=0.0, largest=1, min_voxels=0, fill_sdf=1.0, each=_each):
    """KeepComponents of a grid cut into z-slabs: label_components_slabs, the library's keep rule on the merged list
    (vcy_select_components_host, through select_components), then every slab's own filter kernel over its pieces that go.
    A slab's halo below an upper slab is stale afterwards, as after a carve: every extraction path here exchanges halos
    first.  Returns {"removed_components", "removed_voxels" (of the whole grid), "device_ms" (labelling, seams and filter,
    summed over this rank's slabs)}."""
    import math
    if not math.isfinite(fill_sdf) or not float(np.float32(fill_sdf)) >= float(iso_level):
        raise RuntimeError("keep_components_slabs: fill_sdf %g must be finite and not below the iso level %g"
                           % (fill_sdf, iso_level))
    r = label_components_slabs(carvers, rank, world, iso_level, each)
    _, pieces, n_gone, gone_voxels = select_components(r["merged"], largest, min_voxels, r["maps"])
    ids = [rank + i * world for i in range(len(carvers))]

    def drop(i, c):
        mine = r["lists"][ids[i]]["label"][pieces[ids[i]]]
        return c.KeepComponentsSlab(mine, fill_sdf)["device_ms"] if n_gone else 0.0

    ms = each(carvers, drop)
    return {"removed_components": n_gone, "removed_voxels": gone_voxels, "device_ms": r["device_ms"] + float(sum(ms))}


# ---- ray-cast of the hull of a grid in z-slabs (the slab image and the merge rule: include/vacancy_hip.h) -----------

def _as_views(views):
    from .capi import View
    single = isinstance(views, View)
    return single, ([views] if single else list(views))


def render_hull_slabs(carvers, rank=0, world=1, views=(), iso_level=0.0, voxel_ids=False, axes=False, each=_each,
                      render=None):
    """RenderHull of a grid cut into z-slabs.  `carvers` as for label_components_slabs.  Every slab renders its own
    image of every view on its device (RenderHullSlab; no halo exchange), the images -- depth, voxel ids and, with
    axes=True, entry axes -- are gathered as Python objects, and rank 0 merges them on the host by the rule of
    vcy_render_merge_host.  Returns what VoxelCarver.RenderHull returns (plus "device_ms" per view list: the sum over
    this rank's slabs) on rank 0, None elsewhere.  `render(i, carver, views)` replaces the slab's render (tests)."""
    from . import carver as _vc
    single, vs = _as_views(views)
    k = len(carvers)
    ids = [rank + i * world for i in range(k)]
    ms = [0.0] * k

    def cast(i, c):
        if render is not None:
            return render(i, c, vs)
        parts = c.RenderHullSlab(vs, iso_level, voxel_ids=True, axes=axes)
        ms[i] = c.last_render_ms()
        return parts

    images = _gather_by_slab(dict(zip(ids, each(carvers, cast))), world)
    if rank != 0:
        return None
    out = []
    for j, v in enumerate(vs):
        m = _vc.render_merge_host(v, [images[s][j] for s in range(world * k)])
        if not voxel_ids:
            del m["voxel"]
        if not axes:
            m.pop("axis", None)
        m["device_ms"] = float(sum(ms))
        out.append(m)
    return out[0] if single else out


def hull_agreement_slabs(carvers, rank=0, world=1, views=(), masks=(), iso_level=0.0, each=_each, render=None):
    """HullAgreement of a grid cut into z-slabs: every slab renders its packed hit bits (one bit per pixel crosses to
    the host, no image), they are gathered, and rank 0 ORs them and counts against the silhouettes
    (vcy_hull_agreement_host).  int64 [n_views, 3] as VoxelCarver.HullAgreement on rank 0, None elsewhere."""
    from . import carver as _vc
    vs = list(views)
    ms = list(masks)
    if len(ms) != len(vs):
        raise ValueError("one height x width silhouette per view")
    k = len(carvers)
    ids = [rank + i * world for i in range(k)]

    def cast(i, c):
        parts = render(i, c, vs) if render is not None else c.RenderHullSlab(vs, iso_level, hits=True)
        return [p["hits"] for p in parts]

    bits = _gather_by_slab(dict(zip(ids, each(carvers, cast))), world)
    if rank != 0:
        return None
    counts = np.zeros((len(vs), 3), np.int64)
    for j, (v, m) in enumerate(zip(vs, ms)):
        counts[j] = _vc.hull_agreement_host(v, [bits[s][j] for s in range(world * k)], m)
    return counts


# ---- distance field of the hull of a grid in z-slabs (the order of the calls: include/vacancy_hip.h) ------------------

def distance_halos(z_ranges, radius, bottoms, tops):
    """The assembly of the seam planes, by vcy_distance_halo_host (no GPU) once per slab.  `z_ranges`: [(z0, z1)] of every
    slab of the grid in z order; bottoms[s] / tops[s]: the lowest / highest min(radius, z1 - z0) planes of slab s, uint16
    [planes, nx * ny] in ascending z (None where nobody needs them: the bottom of the first slab, the top of the last).
    Returns [(below, above)] per slab: the planes of the global slices [z0 - min(radius, z0), z0) and
    [z1, z1 + min(radius, nz - z1)), from as many neighbours as that takes, None where there are none."""
    from . import capi, carver as _vc
    ns, nz = len(z_ranges), z_ranges[-1][1]
    edges = [[None if p is None else np.ascontiguousarray(p, np.uint16) for p in side] for side in (bottoms, tops)]
    sl = max([p.shape[-1] for side in edges for p in side if p is not None], default=1)
    ptrs = [(C.c_void_p * ns)(*[None if p is None else p.ctypes.data for p in side]) for side in edges]
    bounds = np.array([0] + [z1 for _, z1 in z_ranges], np.int32)
    out = []
    for s in range(ns):
        below, above = np.empty((min(radius, nz), sl), np.uint16), np.empty((min(radius, nz), sl), np.uint16)
        nb, na = C.c_int(0), C.c_int(0)
        rc = capi.load().vcy_distance_halo_host(ns, _vc._p(bounds), int(radius), sl, ptrs[0], ptrs[1], s, _vc._p(below),
                                                _vc._p(above), C.byref(nb), C.byref(na))
        if rc != 0:
            _vc._raise_rc(rc)
        out.append((below[:nb.value] if nb.value else None, above[:na.value] if na.value else None))
    return out


def _distance_slabs(carvers, rank, world, iso_level, radius, each, finish):
    """begin on every slab, the planes through the host, finish(i, carver, below, above) on every slab.  Returns
    ([finish's results], device ms of this rank's begins, bytes of planes this rank's slabs handed out)."""
    k = len(carvers)
    ids = [rank + i * world for i in range(k)]
    count = world * k

    def begin(i, c):
        ms = c.DistanceSlabBegin(iso_level, radius)
        z0, z1 = c.z_range
        m = min(radius, z1 - z0)
        bottom = c.DistanceSlabPlanes(z0, z0 + m) if ids[i] > 0 else None
        top = c.DistanceSlabPlanes(z1 - m, z1) if ids[i] + 1 < count else None
        return (z0, z1), bottom, top, ms

    begun = each(carvers, begin)
    got = _gather_by_slab(dict(zip(ids, [b[:3] for b in begun])), world)
    halos = distance_halos([got[s][0] for s in range(count)], radius, [got[s][1] for s in range(count)],
                           [got[s][2] for s in range(count)])
    done = each(carvers, lambda i, c: finish(i, c, *halos[ids[i]]))
    nbytes = sum(p.nbytes for b in begun for p in b[1:3] if p is not None)
    return done, float(sum(b[3] for b in begun)), int(nbytes)


def distance_field_slabs(carvers, rank=0, world=1, iso_level=0.0, radius=8, each=_each):
    """DistanceField of a grid cut into z-slabs.  `carvers`, `each` as for label_components_slabs.  Every slab runs the x
    and the y pass over its own slices on its device; its lowest and highest min(radius, own slices) planes of 16-bit
    values are gathered as Python objects -- never a slab's volume --, every rank puts its slabs' halos together
    (distance_halos) and every slab finishes with the z pass.  Every slab finishes one step before any slab begins the
    next.  Returns {"fields": [the int32 field of each of this rank's slabs], "device_ms": the sum over this rank's slabs,
    "plane_bytes": what this rank's slabs sent through the host}; the fields equal VoxelCarver.DistanceField of the
    whole grid."""
    ms = [0.0] * len(carvers)

    def finish(i, c, below, above):
        d2 = c.DistanceFieldSlab(below, above)
        ms[i] = c.last_distance_ms()
        return d2

    fields, begin_ms, nbytes = _distance_slabs(carvers, rank, world, iso_level, radius, each, finish)
    return {"fields": fields, "device_ms": begin_ms + float(sum(ms)), "plane_bytes": nbytes}


def redistance_slabs(carvers, rank=0, world=1, iso_level=0.0, radius=8, each=_each):
    """Redistance of a grid cut into z-slabs, by the steps of distance_field_slabs: every slab's state ends as the whole
    grid's context would leave its slices.  The halos below the slabs are stale afterwards, as after a carve.  Returns
    {"rewritten": [per slab of this rank], "device_ms": the sum over this rank's slabs, "begin_ms" / "finish_ms": its two
    parts, "plane_bytes"}."""
    parts, begin_ms, nbytes = _distance_slabs(carvers, rank, world, iso_level, radius, each,
                                              lambda i, c, below, above: c.RedistanceSlab(below, above))
    finish_ms = float(sum(p["device_ms"] for p in parts))
    return {"rewritten": [p["rewritten"] for p in parts], "device_ms": begin_ms + finish_ms, "begin_ms": begin_ms,
            "finish_ms": finish_ms, "plane_bytes": nbytes}


def close_hull_slabs(carvers, rank=0, world=1, iso_level=0.0, radius_voxels=1.3, each=_each):
    """CloseHull of a grid cut into z-slabs: the three steps of VoxelCarver.CloseHull, each a redistance_slabs, with the
    plan and the tie rule of vcy_close_hull_plan through vacancy_amd.carver.close_hull_plan (ValueError, state untouched,
    for a radius on which the closing ties).  Returns the three redistance_slabs dicts."""
    from . import carver as _vc
    r, big_r = _vc.close_hull_plan(radius_voxels, carvers[0].option.resolution)
    return [redistance_slabs(carvers, rank, world, level, big_r, each) for level in (iso_level, r, -r)]
