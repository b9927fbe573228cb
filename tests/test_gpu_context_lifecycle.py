"""What a context takes from the device goes back when it is destroyed, and a refused vcy_create leaves nothing behind.

Every resource of a context -- device buffers, page-locked staging, events, its two streams -- is a member of an owning
type (vcy_resources.h) and is released with the context; nothing is freed by name.  The first test creates, uses and
destroys contexts in a loop, touching every lazily allocated group of buffers once per cycle, and watches the device's
free memory: a buffer that a cycle leaves behind makes it fall from cycle to cycle.  The second pins the early exit of
vcy_create.  Only the public Python mirror is used."""
import ctypes as C

import numpy as np
import pytest
import torch

from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import synth

pytestmark = pytest.mark.gpu

N = 64            # the grid of a cycle: 64^3
SMALL = 16        # ... and of the context that widens its counters inside the same cycle
W, H = 96, 72
CYCLES = 5

# Free memory after the cycles 2 .. 5 may lie below the value after cycle 1 by at most SLACK_BYTES: the drift the same
# loop shows where everything is freed by name, plus the smallest per-voxel array of a cycle, the one-byte counters of
# 64^3 voxels (256 KiB) -- so one per-voxel buffer left behind per cycle always fails.
# Measured drift (largest fall of the values after cycles 2 .. 5 below the value after cycle 1, MI355X, both in one
# visit; all five readings were equal in both): the commit before the owning types 0 bytes, with them 0 bytes.
DRIFT_BYTES = 0
SLACK_BYTES = DRIFT_BYTES + N ** 3


def _use_everything(views, masks, sdfs, photo):
    """One context of 64^3 and one of 16^3, every lazily allocated group touched once, both destroyed."""
    dev = vc.VoxelCarver(synth.sphere_option(N))
    assert dev.Init(), vc.last_error()
    # per-view carves: the pending queue and the image pool (host image, device image, silhouette)
    assert dev.Carve(views[0], sdfs[0]), vc.last_error()
    img = dev.upload_sdf(sdfs[1])
    assert dev.CarveDevice(views[1], img), vc.last_error()
    assert dev.CarveSilhouette(views[2], masks[2]), vc.last_error()
    dev.sync()
    dev.free_device(img)
    # the streamed batch (stream pool, page-locked staging, producer stream and its events), timed and counted
    dev.set_param("carvetimer", 1)
    dev.set_param("paircount", 1)
    assert dev.CarveBatchSilhouettes(views[3:5], masks[3:5]), vc.last_error()
    dev.last_carve_ms()
    dev.last_carve_pairs()
    dev.last_stream_ms()
    dev.set_param("carvetimer", 0)
    dev.set_param("paircount", 0)
    mesh = dev.ExtractIsoSurface(0.0, True, normals=True)
    assert len(mesh["faces"]) > 0
    assert len(dev.ExtractVoxel()["faces"]) > 0
    assert len(dev.LabelComponents()["label"]) >= 1
    dev.KeepComponents()
    depth = dev.RenderHull(views[0])["depth"]
    assert np.isfinite(depth).any()
    rgb = dev.ColorVertices(mesh["vertices"], [views[0]], [photo], mesh["normals"])["rgb"]
    assert rgb.shape == (len(mesh["vertices"]), 3)
    dev.close()

    # the spare counter array: views across the 255 -> 256 widening, a reset (one byte again, the wide array kept), and
    # single-view carves across it once more
    small = vc.VoxelCarver(synth.sphere_option(SMALL))
    assert small.Init(), vc.last_error()
    cams, small_masks = synth.sphere_views(SMALL, 4, 32, 24)
    imgs = [small.upload_sdf(vc.make_sdf(m)) for m in small_masks]
    assert small.CarveBatchDevice([cams[i % 4] for i in range(260)], [imgs[i % 4] for i in range(260)]), vc.last_error()
    assert small.get_param("count_bytes") == 2
    small.reset()
    assert small.get_param("count_bytes") == 1
    for i in range(260):
        assert small.CarveDevice(cams[i % 4], imgs[i % 4]), vc.last_error()
    small.sync()
    assert small.get_param("count_bytes") == 2
    for p in imgs:
        small.free_device(p)
    small.close()


def test_destroy_returns_device_memory():
    views, masks = synth.sphere_views(N, 5, W, H)
    sdfs = [vc.make_sdf(m) for m in masks[:2]]
    photo = np.full((H, W, 3), 200, np.uint8)
    free = []
    for cycle in range(CYCLES):
        _use_everything(views, masks, sdfs, photo)
        torch.cuda.synchronize(0)
        free.append(torch.cuda.mem_get_info(0)[0])
    # (what the first cycle takes -- code objects, the runtime's own pools -- is in every reading, free[0] included:
    # the value after cycle 1 is the baseline, the values after cycles 2 .. 5 are compared with it)
    falls = [free[0] - f for f in free[1:]]
    print("free device memory after each cycle: %s; fall below cycle 1: %s bytes (slack %d)" % (free, falls, SLACK_BYTES))
    assert max(falls) <= SLACK_BYTES, (free, falls)


def test_create_failure_releases():
    lib = capi.load()
    opt = synth.sphere_option(N)
    ctx = C.c_void_p()
    # z_begin = 1: refused after the checks that allocate nothing, with the context already made
    rc = lib.vcy_create(C.byref(opt), 0, 1, N, C.byref(ctx))
    assert rc == capi.VCY_ERR_INVALID_ARG
    assert not ctx
    assert vc.last_error() == "a non-first slab must start at z >= 2"
    dev = vc.VoxelCarver(opt)
    assert dev.Init(), vc.last_error()
    assert dev.selftest()
    dev.close()
