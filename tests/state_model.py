"""Every writer of the voxel state against every reader that keeps something derived from it, in sequences.

A vcy_ctx holds flags and counters beside the state (fresh, cnt_implied, the brick minima, halo_valid, the queue of deferred
views, the epoch of the state and the ray-cast's bit planes, the marching-cubes size hints, the component labels); every reader is right
only if every writer cleared exactly the right ones.  This module has

  Model   (sdf, update_num) of the WHOLE grid on the CPU, every writer applied with the restatement the suite already trusts
          (the oracle's carve, depth_ref, robust_ref, components_ref), every reader answered from it; results are memoised by
          the tuple of writers applied so far, so cases that share a prefix pay for it once and get it read-only;
  Device  the same operations on one vacancy_amd.carver.VoxelCarver, or on two z-slab contexts in lock-step whose halos are
          exchanged through halo_pack_host / halo_unpack_host only where an operation says so; every reader is compared with
          the model bit for bit, and on slabs the halo contract is checked after every writer;
  script  the seeded generator of sequences (tests/test_gpu_state_sequences.py collects SEEDS, tests/fuzz/
          fuzz_state_sequences.py runs any range).

The base state of every case is CARVED, never uploaded: a fused carve of two silhouette views on a fresh context, after which
cnt_implied is true and the brick minima are valid -- an uploaded base would switch the minima off for good."""
import time

import numpy as np

import color_cases as CC
import components_ref as CR
import depth_ref as DR
import normals_ref as NR
import oracle_lib as O
import render_ref as RR
import robust_cases as RC
import robust_ref as R
import test_gpu_render as TR
from test_gpu_components import assert_mesh_equal
from vacancy_amd import capi
from vacancy_amd import carver as vc
from vacancy_amd import dist as vdist
from vacancy_amd.capi import UpdateOption

F = np.float32
LOWEST = np.finfo(np.float32).min
W, H = TR.W, TR.H  # 48 x 40

# ---- what a case is made of ------------------------------------------------------------------------------------------------

# "max_update_4": the fused carve's checkmax and the depth kernel's gate then hinge on views_carved staying right across writers
OPTION_SETS = {
    "max": dict(),
    "tsdf": dict(voxel_update=1, use_truncation=True, truncation_band=0.2),
    "max_update_4": dict(voxel_max_update_num=4),
}
# (24, 20, 17): nx no multiple of 8 -- no cooperative write-back; (64, 16, 18): a row is one whole 64-voxel word -- the
# brick-row pass of marching cubes, the cooperative write-back and the row kernel are possible; nz no multiple of 8
SHAPES = [(24, 20, 17), (64, 16, 18)]
# the smallest legal lower and upper slab, a cut on a brick layer and one off it
CUTS = {(24, 20, 17): [2, 15, 8, 9], (64, 16, 18): [2, 16, 8, 9]}
PAIR_CUT = {(24, 20, 17): 8, (64, 16, 18): 9}

WRITERS = ["fused", "perview", "queued", "streamed", "depth", "robust", "filter", "upload", "reset"]
READERS = ["download", "mc", "xv", "render", "labels", "color"]
SLAB_READERS = ["download", "mc", "xv", "render", "labels"]  # (the internal ray-cast of ColorVertices needs the whole grid)
NEW_WRITERS = ("depth", "robust", "filter", "upload", "reset")
CLOSE = "close"  # one more fused carve at "cull" 1: where stale brick minima would show

ROBUST_TOLERATE = 1
DEPTH_BAND = 2.0
# The ray-casts of a case -- RenderHull and the internal one of ColorVertices -- walk through this pattern, so that the iso
# level of the kept bit planes moves between some casts and stays between others: with two casts per round of readers every
# FIRST cast after a writer asks for the level the planes were last built for, where only the epoch of the state makes them stale.  (At
# -0.3 the hull is smaller with truncation and EMPTY without: test_state_model_cpu.py says why; kept planes show either way.)
RENDER_ISOS = (0.0, -0.3)
ISO_PATTERN = (0.0, -0.3, -0.3, 0.0)
HALO_ERROR = "halo slices not installed"


def writers_of(option_set):
    """The robust carve is defined for kMax only (include/vacancy_hip.h; weighted average is refused).  It runs under
    max_update_4 as well: by its definition voxel_max_update_num is not applied, and robust_ref samples every view on a fresh
    grid, where the limit cannot bind -- update_num = 5 = the limit + 1 is what the counters' cap admits."""
    return [w for w in WRITERS if not (w == "robust" and OPTION_SETS[option_set].get("voxel_update", 0) == 1)]


def option_for(option_set, dims):
    opt = RC.option_for(dims)
    opt.update_option = UpdateOption(**OPTION_SETS[option_set])
    return opt


# ---- the scene of a shape: an object with a floater, ten views of it, their silhouettes and depth images ---------------------

_DIRECTIONS = [(0.3, -1.6, 1.1), (-0.4, 1.7, -0.5), (1.3, 0.9, -1.7), (-1.2, 0.8, 1.5), (-0.9, -1.1, -1.4), (1.5, 0.2, 0.6),
               (0.8, -0.7, -1.6), (-1.6, 0.3, -0.2), (0.2, 1.1, 1.8), (1.1, -1.3, 0.4), (-0.6, -1.5, 0.9), (0.5, 1.4, -1.2)]
# A fused launch takes ONE projection model (a mixed batch goes to the per-view kernel, which leaves the brick minima invalid):
# every silhouette batch is all pinhole (even indices) or all orthographic (odd).  The depth and the robust carve may mix.
VIEWS_OF = {"base": [0, 2], "fused": [4, 6, 8], "perview": [4, 6, 8], "queued": [5, 7], "streamed": [1, 3, 9],
            CLOSE: [10, 4], "depth": [0, 3], "robust": [0, 1, 2, 4, 11], "render": [2, 1]}


def scene_views(dims):
    """Pinhole views (even indices) and orthographic ones (odd) around the grid, 3 and 4 with a shrunk ROI, made by
    test_gpu_render.look like the views of the render, robust and depth cases."""
    e = float(max(dims))
    out = []
    for i, d in enumerate(_DIRECTIONS):
        pos = np.array(d) * e
        if i % 2 == 0:
            out.append(TR.look(pos, (0.02 * e, -0.01 * e, 0.03 * e), 34.0 * float(np.linalg.norm(pos)) / e,
                               roi=((5, 4), (40, 33)) if i == 4 else None))
        else:
            out.append(TR.look(pos, (0.0, 0.0, 0.0), ortho=True, roi=((3, 2), (44, 37)) if i == 3 else None))
    return out


def object_mask(dims):
    """The object the silhouettes and depth images show: an ellipsoid and a small blob beside it along x (bool per voxel)."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")

    def ball(c, r):
        return ((x - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((z - c[2]) / r[2]) ** 2 <= 1.0

    main = ball((0.38 * nx, 0.5 * ny, 0.5 * nz), (0.20 * nx, 0.32 * ny, 0.32 * nz))
    blob = ball((0.86 * nx, 0.5 * ny, 0.45 * nz), (max(2.0, 0.06 * nx), 0.16 * ny, 0.16 * nz))
    return (main | blob).reshape(-1)


def depth_only_mask(dims):
    """A part of the object that only the depth images show, in a corner no silhouette leaves solid: with weighted averaging the
    depth carve LOWERS voxels there below the iso level, in bricks whose minimum the fused carve left above it -- the one way
    in which brick minima kept across a depth carve would be wrong and not merely cautious (under kMax a depth sample can only
    raise a voxel, so stale minima stay lower bounds)."""
    nx, ny, nz = dims
    z, y, x = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    return (((x - 0.12 * nx) / max(2.5, 0.08 * nx)) ** 2 + ((y - 0.8 * ny) / (0.14 * ny)) ** 2
            + ((z - 0.8 * nz) / (0.14 * nz)) ** 2 <= 1.0).reshape(-1)


class Scene:
    """Everything of a shape that does not depend on the option set."""

    def __init__(self, dims):
        self.dims = tuple(dims)
        self.n = dims[0] * dims[1] * dims[2]
        opt = RC.option_for(dims)
        self.planes = RR.option_planes(opt)
        self.views = scene_views(dims)
        self.solid = object_mask(dims)
        seen_by_depth = self.solid | depth_only_mask(dims)
        px, py, pz = DR.positions(opt)
        self.masks, self.depths = [], []
        for v in self.views:
            ok, xi, yi, _ = DR.project(v, px[self.solid], py[self.solid], pz[self.solid])
            m = np.zeros((H, W), bool)
            m[yi[ok], xi[ok]] = True
            grown = m.copy()  # a voxel may span more than a pixel: close the holes between the projected centres
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    grown[max(0, dy):H + min(0, dy), max(0, dx):W + min(0, dx)] |= m[max(0, -dy):H - max(0, dy), max(0, -dx):W - max(0, dx)]
            self.masks.append((grown * 255).astype(np.uint8))
            self.depths.append(RR.render(v, self.planes, self.dims, seen_by_depth)[0])  # (RenderHull's meaning: +inf on a miss)
        rng = np.random.RandomState(5)
        half = np.array([d + 0.3 for d in dims]) / 2.0 * 1.1
        self.points = ((rng.rand(400, 3) * 2.0 - 1.0) * half).astype(F)
        nr = rng.randn(400, 3)
        self.normals = (nr / np.linalg.norm(nr, axis=1, keepdims=True)).astype(F)
        self.render_views = [self.views[i] for i in VIEWS_OF["render"]]
        self.photos = CC.photos(self.render_views, 41)
        # the two-voxel floater of the upload, in a corner the object does not reach
        self.floater = np.array([(dims[2] - 2) * dims[0] * dims[1] + dims[0] + 1, (dims[2] - 2) * dims[0] * dims[1] + dims[0] + 2])


_scenes = {}


def scene(dims):
    if tuple(dims) not in _scenes:
        _scenes[tuple(dims)] = Scene(tuple(dims))
    return _scenes[tuple(dims)]


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


# ---- the model -------------------------------------------------------------------------------------------------------------------

class Model:
    """The state of the whole grid after a tuple of writers (readers in the tuple are ignored), and what every reader has to
    return for it.  One instance per (option set, shape); see model()."""

    def __init__(self, option_set, dims):
        self.option_set, self.dims = option_set, tuple(dims)
        self.scene = scene(dims)
        self.opt = option_for(option_set, dims)
        self.n = self.scene.n
        self.slice = dims[0] * dims[1]
        self._states, self._answers, self._sdfs, self._robust = {}, {}, None, None
        self.seconds = 0.0

    # -- inputs
    def sdf_images(self):
        """The silhouette SDF of every view, as the device's builder makes it for this option set."""
        if self._sdfs is None:
            u = self.opt.update_option
            self._sdfs = [O.make_sdf(m, tuple(v.roi_min), tuple(v.roi_max), True, bool(u.use_truncation), u.truncation_band)
                          for v, m in zip(self.scene.views, self.scene.masks)]
        return self._sdfs

    def inputs(self, name):
        """(views, images) of a writer: SDF images for the silhouette carves and the robust carve, depth images for "depth"."""
        ids = VIEWS_OF[name]
        images = self.scene.depths if name == "depth" else self.sdf_images()
        return [self.scene.views[i] for i in ids], [images[i] for i in ids]

    # -- writers
    @staticmethod
    def writers(ops):
        return tuple(o for o in ops if o in WRITERS or o == CLOSE)

    def _carve(self, state, name):
        views, sdfs = self.inputs(name)
        prev = O.set_num_threads(1)  # (a few thousand voxels: the OpenMP barriers would cost more than the work)
        try:
            g = O.OracleGrid(self.opt)
            g.upload(*state)
            for v, s in zip(views, sdfs):
                g.carve(v, s)
            out = g.download()
            g.close()
        finally:
            O.set_num_threads(prev)
        return out

    def overruled(self):
        return self._robust_result()[2]

    def _robust_result(self):
        if self._robust is None:
            views, sdfs = self.inputs("robust")
            self._robust = R.robust(self.opt, views, sdfs, ROBUST_TOLERATE, 0.0)
        return self._robust

    def upload_arrays(self, state):
        """What the "upload" writer hands to vcy_upload on top of `state`: + 0.125 on every third voxel (NaN -> 0 first) and a
        floater of two solid voxels."""
        s, c = state
        s2 = (np.where(np.isnan(s), F(0), s) + F(0.125) * (np.arange(s.size) % 3 == 0)).astype(F)
        c2 = c.copy()
        s2[self.scene.floater], c2[self.scene.floater] = F(-0.5), 1
        return s2, c2

    def apply(self, state, name):
        """The state after writer `name` on `state` (new arrays)."""
        s, c = state
        if name in ("fused", "perview", "queued", "streamed", CLOSE, "base"):
            return self._carve(state, name)
        if name == "depth":
            views, depths = self.inputs("depth")
            return DR.carve_depth(self.opt, views, depths, DEPTH_BAND, s, c)
        if name == "robust":
            rs, rc, _ = self._robust_result()
            return rs.copy(), rc.copy()
        if name == "filter":
            comps, lab = CR.reference(s, c, self.dims, 0.0)
            return CR.filter_state(s, lab, comps, largest=1)[0], c.copy()
        if name == "upload":
            return self.upload_arrays(state)
        if name == "reset":
            return np.full(self.n, LOWEST, F), np.zeros(self.n, np.int32)
        raise KeyError(name)

    def state(self, ops=()):
        """(sdf, update_num) after the base carve and the writers of `ops`, read-only."""
        key = self.writers(ops)
        if key not in self._states:
            t0 = time.perf_counter()
            if not key:
                fill = (np.full(self.n, LOWEST, F), np.zeros(self.n, np.int32))
                out = self.apply(fill, "base")
            else:
                out = self.apply(self.state(key[:-1]), key[-1])
            self._states[key] = _frozen(np.ascontiguousarray(out[0], F), np.ascontiguousarray(out[1], np.int32))
            self.seconds += time.perf_counter() - t0
        return self._states[key]

    # -- readers
    def _answer(self, ops, what, make):
        key = (self.writers(ops), what)
        if key not in self._answers:
            t0 = time.perf_counter()
            self._answers[key] = make()
            self.seconds += time.perf_counter() - t0
        return self._answers[key]

    def _grid(self, ops):
        g = O.OracleGrid(self.opt)
        g.upload(*self.state(ops))
        return g

    def mesh(self, ops, iso=0.0):
        """The oracle's marching cubes with the restated normals (normals_ref) of its mesh."""
        def make():
            g = self._grid(ops)
            m = g.marching_cubes(iso, True)
            g.close()
            m.pop("ms")
            m["normals"], m["face_normals"] = NR.mesh_normals(m["vertices"], m["faces"])
            return m
        return self._answer(ops, ("mesh", iso), make)

    def slab_mesh(self, ops, z0, z1, iso=0.0):
        def make():
            g = self._grid(ops)
            m = O.marching_cubes_slab(g, z0, z1, iso, True)
            g.close()
            return m
        return self._answer(ops, ("slab mesh", z0, z1, iso), make)

    def voxel_mesh(self, ops, inside_empty):
        def make():
            g = self._grid(ops)
            m = g.extract_voxel(inside_empty)
            g.close()
            return m
        return self._answer(ops, ("voxel mesh", bool(inside_empty)), make)

    def kept_voxels(self, ops):
        """ExtractVoxel's keep predicate without the on-surface test (extract_voxel.cc:283-286), in numpy."""
        s, c = self.state(ops)
        return np.nonzero(~((s > 0) | (c < 1)))[0].astype(np.int64)

    def render(self, ops, iso):
        """[(depth, voxel, axis)] of the two render views."""
        def make():
            solid = RR.solid_mask(*self.state(ops), iso)
            return [RR.render(v, self.scene.planes, self.dims, solid) for v in self.scene.render_views]
        return self._answer(ops, ("render", iso), make)

    def components(self, ops, iso=0.0):
        """(component list, label per voxel)."""
        return self._answer(ops, ("components", iso), lambda: CR.reference(*self.state(ops), self.dims, iso))

    def color(self, ops, iso):
        """(rgb, n_used, best_view) of the scene's points: the host function on the model's depth images."""
        def make():
            sc = self.scene
            depth = [r[0] for r in self.render(ops, iso)]
            got = vc.color_vertices_host(sc.points, sc.render_views, sc.photos, depth, sc.normals, capi.VCY_COLOR_WEIGHTED,
                                         capi.VCY_INTERP_BILINEAR, 0.6, 0.05, (9.0, 8.0, 7.0))
            return got["rgb"], got["n_used"], got["best_view"]
        return self._answer(ops, ("color", iso), make)

    def slab(self, state, z0, z1):
        return state[0][z0 * self.slice:z1 * self.slice], state[1][z0 * self.slice:z1 * self.slice]


_models = {}


def model(option_set, dims):
    key = (option_set, tuple(dims))
    if key not in _models:
        _models[key] = Model(option_set, dims)
    return _models[key]


# ---- the device ------------------------------------------------------------------------------------------------------------------

class Device:
    """One whole-grid context (cut None) or the two z-slab contexts [0, cut) and [cut, nz) of the model's grid.  apply() runs
    a writer, read() a reader and compares it with the model; `ops` is always the tuple of operations applied so far, the
    current one included."""

    def __init__(self, mdl, cut=None, params=None):
        self.m, self.cut = mdl, cut
        nz = mdl.dims[2]
        self.ranges = [(0, nz)] if cut is None else [(0, cut), (cut, nz)]
        self.ctxs = []
        self.params = dict(params or {})
        for zr in self.ranges:
            c = vc.VoxelCarver(mdl.opt, z_range=None if cut is None else zr)
            assert c.Init(), vc.last_error()
            assert c.dims == mdl.dims, (c.dims, mdl.dims)
            c.set_param("mcskip", 2)
            c.set_param("cull", 1)
            for k, v in self.params.items():
                c.set_param(k, v)
            self.ctxs.append(c)
        self._images = [dict() for _ in self.ctxs]
        self.halo_current = cut is None  # whether the upper slab holds the lower slab's last two slices as they are now
        self.casts = 0
        self.cnt_implied = True  # no vcy_upload since the fill (or since a robust carve, which starts the state over)
        self.slab_labelled = False  # whether vcy_label_components_slab has run on the slab contexts since the last filter
        self.voxel_mesh_done = False

    def close(self):
        for c, held in zip(self.ctxs, self._images):
            for p in held.values():
                c.free_device(p)
            c.close()
        self.ctxs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def _device_images(self, k, name):
        """The writer's images resident on context k's device, uploaded once."""
        views, images = self.m.inputs(name)
        held = self._images[k]
        for i, img in zip(VIEWS_OF[name], images):
            if (name == "depth", i) not in held:
                held[name == "depth", i] = self.ctxs[k].upload_sdf(img)
        return views, [held[name == "depth", i] for i in VIEWS_OF[name]]

    # -- writers
    def base(self):
        self._batch("base", 1)
        self.check_brick_minima("base")

    def check_brick_minima(self, ops):
        """The premise of a case: a fused carve went through the fused kernel, and left the brick minima valid unless an
        uploaded state has switched them off."""
        for c in self.ctxs:
            assert c.get_param("brick_min_valid") == int(self.cnt_implied), "%s: brick minima %d" % (ops, 1 - int(self.cnt_implied))

    def _batch(self, name, fused):
        for k, c in enumerate(self.ctxs):
            views, ptrs = self._device_images(k, name)
            c.set_param("fused", fused)
            assert c.CarveBatchDevice(views, ptrs), vc.last_error()
            c.set_param("fused", 1)

    def apply(self, name, ops):
        m = self.m
        if name in ("fused", CLOSE):
            self._batch(name, 1)
            self.check_brick_minima(ops)
        elif name == "perview":
            self._batch(name, 0)
        elif name == "queued":  # left in the queue: the next operation has to flush them
            views, sdfs = m.inputs(name)
            for c in self.ctxs:
                before = c.get_param("defer")
                c.set_param("defer", 1)
                for v, s in zip(views, sdfs):
                    assert c.Carve(v, s), vc.last_error()
                c.set_param("defer", before)
        elif name == "streamed":
            views = [m.scene.views[i] for i in VIEWS_OF[name]]
            masks = [m.scene.masks[i] for i in VIEWS_OF[name]]
            for c in self.ctxs:
                assert c.CarveBatchSilhouettes(views, masks), vc.last_error()
        elif name == "depth":
            views, depths = m.inputs(name)
            for c in self.ctxs:
                c.CarveDepth(views, depths, DEPTH_BAND)
        elif name == "robust":
            total = 0
            for k, c in enumerate(self.ctxs):
                views, ptrs = self._device_images(k, name)
                total = total + c.CarveRobustDevice(views, ptrs, ROBUST_TOLERATE, 0.0)["overruled"]
            self.cnt_implied = True
            assert np.array_equal(total, m.overruled()), "%s: overruled %s, the restatement %s" % (ops, total, m.overruled())
        elif name == "filter":
            self._filter(ops)
        elif name == "upload":
            state = m.state(ops)
            for c, (z0, z1) in zip(self.ctxs, self.ranges):
                c.upload(*m.slab(state, z0, z1))
            self.cnt_implied = False
        elif name == "reset":
            for c in self.ctxs:
                c.reset()
            self.cnt_implied = True
        else:
            raise KeyError(name)
        if self.cut is not None:
            self.halo_current = False
            self.check_halo_refused(ops)
            if name == "filter":
                self.slab_labelled = False  # (a slab that lost nothing keeps its labelling, and may)
            elif self.slab_labelled:
                self.check_labels_refused(ops)

    def _filter(self, ops):
        before = self.m.components(ops[:-1])[0]
        gone_want = int(before["n_voxels"][1:].sum())
        if self.cut is None:
            r = self.ctxs[0].KeepComponents(0.0, largest=1)
            assert (r["removed_components"], r["removed_voxels"]) == (max(0, len(before["label"]) - 1), gone_want), (ops, r)
            return
        # the five steps of include/vacancy_hip.h; the last one on EVERY slab, also one that loses nothing
        r = vdist.label_components_slabs(self.ctxs, 0, 1, 0.0)
        self.slab_labelled = True
        CR.assert_components_equal(r["merged"], before, "%s: merged list before the filter" % (ops,))
        gone = r["merged"]["label"][1:]
        removed = 0
        for k, c in enumerate(self.ctxs):
            mine = r["lists"][k]["label"][np.isin(r["maps"][k], gone)]
            removed += c.KeepComponentsSlab(mine, 1.0)["removed_voxels"]
        assert removed == gone_want, (ops, removed, gone_want)

    # -- the halo contract of an upper slab (include/vacancy_hip.h: after ANY writer, extraction refuses until the exchange)
    def check_halo_refused(self, ops):
        upper = self.ctxs[1]
        for what, call in (("ExtractIsoSurface", lambda: upper.ExtractIsoSurface(0.0, True)),
                           ("extract_voxel_ids(True)", lambda: upper.extract_voxel_ids(True))):
            try:
                call()
            except RuntimeError as e:
                assert HALO_ERROR in str(e), "%s: %s on the upper slab failed with %r" % (ops, what, str(e))
            else:
                raise AssertionError("%s: %s on the upper slab answered from a halo that was not exchanged after the last writer"
                                     % (ops, what))

    # -- the seam calls speak about the state that was labelled: after a writer they refuse until the slab is labelled again
    def check_labels_refused(self, ops):
        for c, (z0, z1) in zip(self.ctxs, self.ranges):
            try:
                c.component_top_plane()
            except RuntimeError as e:
                assert "vcy_label_components_slab" in str(e), "%s z %d..%d: %r" % (ops, z0, z1, str(e))
            else:
                raise AssertionError("%s z %d..%d: vcy_component_top_plane answered from the labels of the state before the "
                                     "last writer" % (ops, z0, z1))

    def exchange(self):
        if self.cut is None or self.halo_current:
            return
        gathered = np.concatenate([c.halo_pack_host() for c in self.ctxs])
        for r, c in enumerate(self.ctxs):
            c.halo_unpack_host(gathered, r, len(self.ctxs))
        self.halo_current = True

    # -- readers
    def read(self, name, ops):
        getattr(self, "read_" + name)(ops)

    def read_all(self, ops):
        """Every reader; on slabs the ones that need no halo first, then the exchange, then the extractions."""
        names = READERS if self.cut is None else ["download", "render", "labels", "render", "mc", "xv"]
        for name in names:
            self.read(name, ops)

    def read_download(self, ops):
        want = self.m.state(ops)
        for c, (z0, z1) in zip(self.ctxs, self.ranges):
            ds, du = c.download()
            ws, wu = self.m.slab(want, z0, z1)
            assert np.array_equal(du, wu), "%s z %d..%d: %d update_num differ" % (ops, z0, z1, int((du != wu).sum()))
            R.assert_sdf_equal(ds, ws, "%s z %d..%d" % (ops, z0, z1))

    def read_mc(self, ops):
        if self.cut is not None:
            self.exchange()
        for skip in (2, 0):
            for c, (z0, z1) in zip(self.ctxs, self.ranges):
                c.set_param("mcskip", skip)
                ctx = "%s z %d..%d mcskip %d" % (ops, z0, z1, skip)
                if self.cut is None:
                    want = self.m.mesh(ops)
                    assert_mesh_equal(c.ExtractIsoSurface(0.0, True), {k: want[k] for k in ("vertices", "faces", "keys")}, ctx)
                    assert_mesh_equal(c.ExtractIsoSurface(0.0, True, normals=True), want, ctx + " normals")
                else:
                    want = self.m.slab_mesh(ops, z0, z1)
                    got = c.ExtractIsoSurface(0.0, True)
                    assert got["n_foreign"] == want["n_foreign"], ctx
                    assert_mesh_equal(got, want, ctx)
        for c in self.ctxs:
            c.set_param("mcskip", 2)

    def read_xv(self, ops):
        if self.cut is not None:
            self.exchange()
        for inside_empty in (True, False):
            ids = np.concatenate([c.extract_voxel_ids(inside_empty) for c in self.ctxs])
            if not inside_empty:
                assert np.array_equal(ids, self.m.kept_voxels(ops)), "%s: kept voxel ids" % (ops,)
            want = self.m.voxel_mesh(ops, inside_empty)
            got = vc.voxel_cubes(self.m.opt, ids)
            assert np.array_equal(got["faces"], want["faces"]), "%s: cubes of the kept voxels, inside_empty %s" % (ops, inside_empty)
            assert np.array_equal(TR.bits(got["vertices"]), TR.bits(want["vertices"])), (ops, inside_empty)
        if self.cut is None and not self.voxel_mesh_done:  # ExtractVoxel itself, once per case
            self.voxel_mesh_done = True
            got, want = self.ctxs[0].ExtractVoxel(True), self.m.voxel_mesh(ops, True)
            assert np.array_equal(got["faces"], want["faces"]) and np.array_equal(TR.bits(got["vertices"]), TR.bits(want["vertices"])), ops

    def next_iso(self):
        iso = ISO_PATTERN[self.casts % len(ISO_PATTERN)]
        self.casts += 1
        return iso

    def read_render(self, ops):
        iso = self.next_iso()
        views = self.m.scene.render_views
        want = self.m.render(ops, iso)
        if self.cut is None:
            got = self.ctxs[0].RenderHull(views, iso, voxel_ids=True, axes=True)
        else:
            parts = [c.RenderHullSlab(views, iso, voxel_ids=True, axes=True) for c in self.ctxs]
            got = [vc.render_merge_host(v, [p[j] for p in parts]) for j, v in enumerate(views)]
        for j, (g, w) in enumerate(zip(got, want)):
            TR.assert_images_equal(g, w, "%s iso %g view %d" % (ops, iso, j))

    def read_labels(self, ops):
        want, lab = self.m.components(ops)
        if self.cut is None:
            got = self.ctxs[0].LabelComponents(0.0, labels=True)
            labels = got["labels"]
        else:
            got = vdist.label_components_slabs(self.ctxs, 0, 1, 0.0)["merged"]
            self.slab_labelled = True
            labels = np.concatenate([c.download_labels() for c in self.ctxs])
        CR.assert_components_equal(got, want, "%s" % (ops,))
        assert np.array_equal(labels, lab), "%s: the labels of %d voxels differ" % (ops, int((labels != lab).sum()))

    def read_color(self, ops):
        assert self.cut is None
        iso = self.next_iso()
        sc = self.m.scene
        got = self.ctxs[0].ColorVertices(sc.points, sc.render_views, sc.photos, sc.normals, None, capi.VCY_COLOR_WEIGHTED,
                                         capi.VCY_INTERP_BILINEAR, 0.6, 0.05, (9.0, 8.0, 7.0), iso_level=iso)
        CC.assert_equal(got, self.m.color(ops, iso), "%s colour at iso %g" % (ops, iso))


def run_pair(option_set, dims, cut, a, b):
    """The pair matrix' case: base, all readers (every cache populated), A, all readers, B, all readers, one more fused carve
    at "cull" 1, then download and marching cubes with brick skipping."""
    m = model(option_set, dims)
    with Device(m, cut) as dev:
        dev.base()
        dev.read_all(())
        for ops in ((a,), (a, b)):
            dev.apply(ops[-1], ops)
            dev.read_all(ops)
        ops = (a, b, CLOSE)
        dev.apply(CLOSE, ops)
        dev.read_download(ops)
        dev.read_mc(ops)


# ---- seeded sequences ------------------------------------------------------------------------------------------------------------

SEEDS = list(range(54))  # one (writer, reader) adjacency forced per seed: 9 x 6
SCRIPT_STREAM = 72000  # (chosen so that SEEDS meet the coverage test_state_model_cpu.py asserts)


def script(seed):
    """dict(option_set, dims, cut (None: whole grid), params, ops) of a seed.  Seed s places writer s % 9 directly before reader
    (s // 9) % 6 somewhere in its 8 - 12 operations, so that 54 consecutive seeds hold every such pair; everything else is drawn."""
    rng = np.random.RandomState(SCRIPT_STREAM + seed)
    w, r = WRITERS[seed % len(WRITERS)], READERS[(seed // len(WRITERS)) % len(READERS)]
    sets = [s for s in OPTION_SETS if w in writers_of(s)]
    option_set = sets[int(rng.randint(0, len(sets)))]
    dims = SHAPES[int(rng.randint(0, len(SHAPES)))]
    slabs = r in SLAB_READERS and bool((seed + seed // len(WRITERS)) % 2)
    cut = CUTS[dims][int(rng.randint(0, 4))] if slabs else None
    params = dict(defer=int(rng.randint(0, 2)), livelist=int(rng.randint(0, 2)), coopstore=int(rng.choice([-1, 0, 1, 1])),
                  rowkernel=int(rng.choice([-1, 0, 0, 2])), oneview=int(rng.choice([1, 1, 0])))
    writers, readers = writers_of(option_set), (SLAB_READERS if slabs else READERS)
    n = int(rng.randint(8, 13))
    ops = [writers[int(rng.randint(0, len(writers)))] if rng.rand() < 0.5 else readers[int(rng.randint(0, len(readers)))]
           for _ in range(n)]
    at = int(rng.randint(0, n - 1))
    ops[at], ops[at + 1] = w, r
    return dict(option_set=option_set, dims=dims, cut=cut, params=params, ops=ops)


def run_script(s):
    """Runs a script: `download` is compared after every writer, every reader after the last operation."""
    m = model(s["option_set"], s["dims"])
    with Device(m, s["cut"], s["params"]) as dev:
        dev.base()
        done = ()
        for op in s["ops"]:
            done = done + (op,)
            if op in WRITERS:
                dev.apply(op, done)
                dev.read_download(done)
            else:
                dev.read(op, done)
        dev.read_all(done)
