"""bench.py --dump-outputs: the carved state after the last timed step, for a fixed sample of voxels, and the plain run
that measures the headline only (everything else is --full)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


class _Slab:
    """Stand-in for a slab context: the state of voxel i is (i / 2, i % 7); refuses ids outside its slab."""

    def __init__(self, n, z0, z1):
        self.dims, self.z_range = (n, n, n), (z0, z1)
        self.slab_voxels = n * n * (z1 - z0)

    def download_voxels(self, ids):
        plane = self.dims[0] * self.dims[1]
        assert ((ids >= self.z_range[0] * plane) & (ids < self.z_range[1] * plane)).all()
        return (ids * 0.5).astype(np.float32), (ids % 7).astype(np.int32)


@pytest.mark.parametrize("n", [16, 1024])
def test_dump_outputs_samples_every_slab_the_same_way(tmp_path, n):
    for out in ("a", "b"):
        bench.dump_outputs(str(tmp_path / out), [_Slab(n, 0, n // 3), _Slab(n, n // 3, n - 5), _Slab(n, n - 5, n)])
    files = sorted(os.listdir(str(tmp_path / "a")))
    assert files == ["sdf.npy", "update_num.npy", "voxel_ids.npy"]
    got = {f: np.load(str(tmp_path / "a" / f)) for f in files}
    for f in files:
        assert got[f].tobytes() == np.load(str(tmp_path / "b" / f)).tobytes()  # same sample every run
    ids = got["voxel_ids.npy"].astype(np.int64)
    assert got["sdf.npy"].dtype == np.float32 and got["update_num.npy"].dtype == np.float32
    if n ** 3 <= bench.DUMP_VOXELS:
        assert len(ids) == n ** 3
    else:  # drawn with replacement, duplicates dropped
        assert 0.99 * bench.DUMP_VOXELS < len(ids) <= bench.DUMP_VOXELS
    assert (np.diff(ids) > 0).all() and ids[0] >= 0 and ids[-1] < n ** 3
    assert np.array_equal(got["sdf.npy"], (ids * 0.5).astype(np.float32))
    assert np.array_equal(got["update_num.npy"], (ids % 7).astype(np.float32))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in files) <= 64e6


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["default", "tsdf"])
def test_plain_run_dumps_what_the_timed_steps_carved(tmp_path, mode):
    """A plain run at 64^3 (every voxel dumped): the JSON line has the headline fields and none of --full's blocks, and
    the dumped state is bit for bit the CPU oracle's carve of the same inputs."""
    import oracle_lib as O
    from vacancy_amd import carver as vc
    from vacancy_amd import synth
    from vacancy_amd.capi import UpdateOption

    n, nv, w, h = 64, 4, 160, 120
    out = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--grid", str(n), "--views", str(nv),
                        "--width", str(w), "--height", str(h), "--mode", mode, "--steps", "3", "--warmup", "1",
                        "--settle-ms", "0", "--dump-outputs", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in line
    assert line["steps"] == 3 and line["ms_per_step"] > 0 and line["mc"] is None
    assert not {"cpu_baseline", "variants", "configs"} & set(line)

    uo = UpdateOption(voxel_update=1, use_truncation=True, truncation_band=0.1) if mode == "tsdf" else UpdateOption()
    views, masks = synth.sphere_views(n, nv, w, h)
    sdf = vc.make_sdf(masks[0], use_truncation=bool(uo.use_truncation), band=uo.truncation_band)
    orc = O.OracleGrid(synth.sphere_option(n, uo))
    for v in views:
        orc.carve(v, sdf)
    os_, ou = orc.download()
    ids = np.load(os.path.join(out, "voxel_ids.npy"))
    assert np.array_equal(ids, np.arange(n ** 3, dtype=np.float64))
    assert np.array_equal(np.load(os.path.join(out, "sdf.npy")).view(np.uint32), os_.view(np.uint32))
    assert np.array_equal(np.load(os.path.join(out, "update_num.npy")), ou.astype(np.float32))
