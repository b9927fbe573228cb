"""The process-wide owners behind the halo all-gathers and the sharded silhouette producer: cached communicator groups
(halo_exchange.hip), cached producer groups (carve_stream.hip) and the vcy_comm of the one-process-per-GPU form.  Their
streams, staging buffers, page-locked memory, events and communicators are members of owning types (vcy_resources.h,
rccl_api.h) and go with their holder; nothing is freed by name.  Three properties, on one device, through the Python
mirror only: what the owners take goes back (free device memory over create / use / shutdown cycles), a cached group
whose buffers must grow keeps giving right results, and a call that fails half-way leaves the owners usable."""
import ctypes as C

import numpy as np
import pytest
import torch

from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist
from vacancy_amd import synth

pytestmark = pytest.mark.gpu

N = 24            # 24^3 in three slabs of 8 slices
W, H = 64, 48
NV = 70           # chunks of 32, 32 and 6: both image sets are reused
CYCLES = 5

# Free memory after the cycles 2 .. 5 may lie below the value after cycle 1 by at most SLACK_BYTES: the fall the same
# loop shows where the owners free their members by name (the commit before the owning types), plus the smallest single
# device allocation the owners make in a cycle -- the send staging of the vcy_comm: the halo packs of its two slabs, two
# slices of 24 x 24 voxels at 4 + 2 bytes each (float sdf, counters at their 2-byte wire width), 2 * 6912 = 13 824 bytes
# -- so one buffer of any owner left behind per cycle always fails.  (The contexts' own buffers:
# test_gpu_context_lifecycle.py.)
# Measured fall (largest fall of the values after cycles 2 .. 5 below the value after cycle 1; MI355X, both builds in one
# visit; all five readings were equal in both): the commit before the owning types 0 bytes, with them 0 bytes.
HALO_PACK_BYTES = 2 * N * N * (4 + 2)
SMALLEST_ALLOCATION = 2 * HALO_PACK_BYTES
PARENT_FALL_BYTES = 0
SLACK_BYTES = PARENT_FALL_BYTES + SMALLEST_ALLOCATION


def slabs_of(n, count=3, **kw):
    out = []
    for r in range(count):
        c = vc.VoxelCarver(synth.sphere_option(n, capi.UpdateOption(**kw)), z_range=vdist.slab_range(n, r, count))
        assert c.Init(), vc.last_error()
        out.append(c)
    return out


def distinct_views(n, nv, w, h, seed):
    views, masks = synth.sphere_views(n, nv, w, h)
    rng = np.random.RandomState(seed)
    for i in range(0, nv, 7):  # distinct silhouettes: an image in a wrong slot would show
        masks[i] = (rng.rand(h, w) < 0.5).astype(np.uint8) * 255
    return views, masks


def _cycle(lib, views, masks, monkeypatch):
    slabs = slabs_of(N)
    assert int(lib.vcy_halo_bytes(slabs[0].ctx)) == HALO_PACK_BYTES
    rec = vc.halo_exchange(slabs)  # one rank, three packs
    assert rec["backend"].startswith("rccl") and rec["ranks"] == 1 and rec["bytes_per_rank"] == 3 * HALO_PACK_BYTES
    for split in (0, 1):  # two different producer groups: one rank for the device, one rank per slab
        monkeypatch.setenv("VCY_TEST_SPLIT_PRODUCERS", str(split))
        assert vc.carve_batch_silhouettes_sharded(slabs, views, masks)
    comm = C.c_void_p()
    assert lib.vcy_comm_create(0, 1, 0, None, 1000, C.byref(comm)) == 0, vc.last_error()
    two = (C.c_void_p * 2)(slabs[0].ctx, slabs[1].ctx)
    assert lib.vcy_halo_allgather_ranks(comm, two, 2) == 0, vc.last_error()
    assert "bytes_per_rank=%d " % SMALLEST_ALLOCATION in lib.vcy_last_collective().decode()
    lib.vcy_comm_destroy(comm)
    for c in slabs:
        c.close()
    lib.vcy_halo_shutdown()


def test_process_wide_owners_return_device_memory(monkeypatch):
    lib = capi.load()
    views, masks = synth.sphere_views(N, NV, W, H)
    free = []
    for cycle in range(CYCLES):
        _cycle(lib, views, masks, monkeypatch)
        torch.cuda.synchronize(0)
        free.append(torch.cuda.mem_get_info(0)[0])
    # (what the first cycle takes for good -- code objects, the pools of the runtime and of RCCL -- is in every reading:
    # the value after cycle 1 is the baseline, the values after cycles 2 .. 5 are compared with it)
    falls = [free[0] - f for f in free[1:]]
    print("free device memory after each cycle: %s; fall below cycle 1: %s bytes (slack %d)" % (free, falls, SLACK_BYTES))
    assert max(falls) <= SLACK_BYTES, (free, falls)


# ---- growing under a cached group ------------------------------------------------------------------------------------

GROW_BATCHES = [(5, 64, 48), (40, 160, 120)]  # the 40-view batch makes every producer buffer and both image sets grow


@pytest.fixture(scope="module")
def grow_reference():
    """The batches of the growth test -- small, large, the small one again -- and, per batch, slabs that ran
    CarveBatchSilhouettes on their own up to and including it.  Built once, left unchanged, closed with the module."""
    batches = [distinct_views(N, nv, w, h, 11 + i) for i, (nv, w, h) in enumerate(GROW_BATCHES)]
    batches.append(batches[0])
    after = []
    for upto in range(len(batches)):
        ref = slabs_of(N)
        for views, masks in batches[:upto + 1]:
            for c in ref:
                assert c.CarveBatchSilhouettes(views, masks), vc.last_error()
        after.append(ref)
    yield batches, after
    for ref in after:
        for c in ref:
            c.close()


@pytest.mark.parametrize("split", [0, 1])
def test_producer_buffers_grow_under_a_cached_group(split, grow_reference, monkeypatch):
    """5 views of 64 x 48, then 40 of 160 x 120, then the first again, on live contexts without a shutdown in between: the
    second batch replaces the pool, the page-locked staging and both gathered image sets of every cached producer rank
    (and adds a second chunk), the third runs in the grown buffers with the first one's layout."""
    batches, after = grow_reference
    monkeypatch.setenv("VCY_TEST_SPLIT_PRODUCERS", str(split))
    capi.load().vcy_halo_shutdown()  # no producer group of an earlier test: the first batch sizes the buffers
    slabs = slabs_of(N)
    try:
        for i, (views, masks) in enumerate(batches):
            assert vc.carve_batch_silhouettes_sharded(slabs, views, masks)
            for s, (got, want) in enumerate(zip(slabs, after[i])):
                assert got.state_diff(want) == 0, "split %d, batch %d, slab %d" % (split, i, s)
    finally:
        capi.load().vcy_halo_shutdown()


def assert_mesh_equal(a, b, ctx):
    for k in ("vertices", "faces", "keys"):
        assert a[k].shape == b[k].shape, "%s %s: %s against %s" % (ctx, k, a[k].shape, b[k].shape)
    assert np.array_equal(a["keys"], b["keys"]) and np.array_equal(a["faces"], b["faces"]), ctx + " faces / keys"
    assert np.array_equal(a["vertices"].view(np.uint32), b["vertices"].view(np.uint32)), ctx + " vertex bits"


def test_halo_staging_grows_under_a_cached_group():
    """halo_exchange between the slabs of a 24^3 grid and then of a 48^3 grid on the same device, no shutdown in between:
    the second exchange finds the device's cached group and needs four times the staging.  The merged extraction of
    either set equals the single-context mesh."""
    lib = capi.load()
    lib.vcy_halo_shutdown()
    sets = []
    try:
        for n in (24, 48):
            views, masks = synth.sphere_views(n, 5, W, H)
            slabs = slabs_of(n)
            whole = vc.VoxelCarver(synth.sphere_option(n))
            assert whole.Init(), vc.last_error()
            for c in slabs + [whole]:
                assert c.CarveBatchSilhouettes(views, masks), vc.last_error()
            rec = vc.halo_exchange(slabs)
            assert rec["backend"].startswith("rccl") and rec["bytes_per_rank"] == 3 * 2 * n * n * 6
            sets.append((n, slabs, whole))
        for n, slabs, whole in sets:
            merged = vdist.merge_meshes([c.ExtractIsoSurface(0.0, True) for c in slabs])
            assert_mesh_equal(merged, whole.ExtractIsoSurface(0.0, True), "%d^3, merged against single context" % n)
            assert len(merged["faces"]) > 0
    finally:
        lib.vcy_halo_shutdown()


# ---- a failed chunk ----------------------------------------------------------------------------------------------------

def test_failed_chunk_leaves_the_owners_usable(monkeypatch):
    """One producer rank per slab (split 1), three chunks; the middle slab's first carve fails through the host-side hook
    "inject_carve_failure" (launch_carve returns VCY_ERR_INTERNAL before it launches anything).  Chunk 0 fails after
    chunk 1 has been produced, so chunk 2 is produced with the call already failed: its rank threads must still meet at
    the barriers of the gather, or the call never returns.  The cached producer group then serves a clean repeat."""
    monkeypatch.setenv("VCY_TEST_SPLIT_PRODUCERS", "1")
    lib = capi.load()
    lib.vcy_halo_shutdown()
    views, masks = distinct_views(N, NV, W, H, 3)
    slabs, ref = slabs_of(N), slabs_of(N)
    try:
        slabs[1].set_param("inject_carve_failure", 1)
        with pytest.raises(RuntimeError, match="injected failure") as info:
            vc.carve_batch_silhouettes_sharded(slabs, views, masks)
        assert info.value.rc == capi.VCY_ERR_INTERNAL
        for c in slabs:
            c.reset()
        assert vc.carve_batch_silhouettes_sharded(slabs, views, masks)
        for c in ref:
            assert c.CarveBatchSilhouettes(views, masks), vc.last_error()
        for s, (got, want) in enumerate(zip(slabs, ref)):
            assert got.state_diff(want) == 0, "slab %d after the failed call" % s
    finally:
        lib.vcy_halo_shutdown()
