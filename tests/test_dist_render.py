"""world_size-2 gloo test of the ray-cast over z-slabs on CPU: vacancy_amd.dist.render_hull_slabs' and
hull_agreement_slabs' gather and host merge, with every slab's device render replaced by the numpy restatement on the
slab's slices (tests/slab_render_cases.py).  Rank 0 must end with the restatement's whole-grid images and counts."""
import os
import socket

import numpy as np

import render_ref as RR
import slab_render_cases as S
from vacancy_amd import dist as vdist

DIMS = (24, 20, 17)
STATE = "random"
BOUNDS = [0, 3, 9, 11, 17]   # four slabs: rank r of 2 holds slabs r and r + 2
NAMES = ["pinhole_outside", "pinhole_inside", "ortho_oblique", "roi_shrunk"]


class RestatedSlab:
    def __init__(self, z0, z1):
        self.z0, self.z1 = z0, z1


def _render(i, slab, views):
    out = []
    for vn, v in zip(NAMES, views):
        d, vox, a = S.slab_image(DIMS, STATE, vn, slab.z0, slab.z1)
        out.append({"depth": d, "voxel": vox, "axis": a, "hits": S.pack_hits(vox, v)})
    return out


def _worker(rank, world, port, ret):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        c = S.case(DIMS)
        views = [c["views"][vn] for vn in NAMES]
        ranges = S.slabs_of(BOUNDS)
        mine = [RestatedSlab(*ranges[s]) for s in range(rank, len(ranges), world)]
        got = vdist.render_hull_slabs(mine, rank, world, views, c["states"][STATE][2], voxel_ids=True, axes=True, render=_render)
        rng = np.random.RandomState(5)
        masks = [(rng.rand(S.H, S.W) < 0.5).astype(np.uint8) for _ in views]
        counts = vdist.hull_agreement_slabs(mine, rank, world, views, masks, render=_render)
        if rank != 0:
            ret["other"] = got is None and counts is None
            return
        ok = len(got) == len(views)
        for vn, g in zip(NAMES, got):
            d, vox, a = c["want"][STATE, vn]
            ok = ok and np.array_equal(S.bits(g["depth"]), S.bits(d)) and np.array_equal(g["voxel"], vox) and np.array_equal(g["axis"], a)
        ret["images"] = bool(ok)
        ret["counts"] = counts.tolist() == [RR.agreement(v, c["want"][STATE, vn][1], m) for vn, v, m in zip(NAMES, views, masks)]
        ret["hits"] = int(sum((c["want"][STATE, vn][1] >= 0).sum() for vn in NAMES))
    finally:
        dist.destroy_process_group()


def test_gather_and_merge_over_two_ranks():
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    with mp.Manager() as mgr:
        ret = mgr.dict()
        mp.spawn(_worker, args=(2, port, ret), nprocs=2, join=True)
        assert ret.get("images") is True and ret.get("counts") is True and ret.get("other") is True
        assert ret["hits"] > 100
