"""vcy_extract_iso_chain on the GPU: bit equality with the separate route (ExtractIsoSurface -> SmoothMesh ->
DecimateMesh[Quadric] -> normals) over the states and the option matrix of chain_cases.py; the chain as a reader of the
voxel state; the refusals; the timers; the "mcdirect" default."""
import ctypes as C

import numpy as np
import pytest

import chain_cases as CH
import color_cases as CC
from vacancy_amd import capi
from vacancy_amd import carver as vc

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=CH.ROWS, ids=["rows_from_faces", "rows_from_cells"])
def chainrows(request):
    """Every test runs with "chainrows" 0 and 1: the contexts of CH.make_dev take the value."""
    CH.use_rows(request.param)
    yield request.param
    CH.use_rows(1)   # (the library's default)


def random_dev(state=CH.finite_random_state):
    sdf, cnt, iso = state()
    dev = CH.make_dev(CC.option(), CC.DIMS)
    dev.upload(sdf, cnt)
    return dev, iso


# ---- 1. bit equality --------------------------------------------------------------------------------------------------

def test_full_matrix_on_the_random_state():
    """Vertices on all three edge axes, dense faces, rows of every length; every smoothing against every decimation."""
    dev, iso = random_dev(CC.random_state)
    for smooth, decimate in CH.full_matrix():
        # (the state has NaN voxels, so NaN vertices: the decimation refuses them, and the chain refuses as it does)
        got = CH.check(dev, iso, smooth, decimate, "random state")
        assert (got is None) == (decimate is not None), CH.name_of(smooth, decimate)
    assert np.isnan(dev.ExtractIsoSurface(iso)["vertices"]).any()


def test_full_matrix_on_the_random_state_without_its_nan_voxels():
    """The same state with every vertex finite: every smoothing against every decimation, to the bit."""
    dev, iso = random_dev()
    n = 0
    for smooth, decimate in CH.full_matrix():
        got = CH.check(dev, iso, smooth, decimate, "finite random state")
        n += len(got["faces"])
    assert n > 0 and got["extracted"][1] > 1000
    CH.check(dev, iso, CH.SMOOTHS[1], CH.DECIMATES[1], "finite random state, nearest-voxel vertices", linear_interp=False)


def test_long_rows_of_three_cell_words():
    sdf, cnt, iso = CH.long_state()
    dev = CH.make_dev(CH.long_option(), CH.LONG_DIMS)
    dev.upload(sdf, cnt)
    for smooth, decimate in CH.stage_pairs():
        got = CH.check(dev, iso, smooth, decimate, "130 x 6 x 5")
    assert got["extracted"][1] > 500


def test_carved_sphere_with_empty_bricks():
    dev = CH.sphere_dev()
    for smooth, decimate in CH.stage_pairs():
        got = CH.check(dev, 0.0, smooth, decimate, "sphere")
    assert got["extracted"][1] > 1000 and 0 < len(got["faces"]) < got["extracted"][1]


def test_iso_on_a_voxel_value_gives_coincident_vertices_and_the_same_bits():
    dev = CH.sphere_dev()
    iso = CH.voxel_value_iso(dev)
    for smooth, decimate in CH.stage_pairs():
        CH.check(dev, iso, smooth, decimate, "sphere, iso %r" % iso)
    v = dev.ExtractIsoSurface(iso)["vertices"]
    assert len(np.unique(v, axis=0)) < len(v)   # (the snaps: distinct ids at one position)


def test_fresh_context_gives_the_empty_mesh():
    dev = CH.make_dev(CC.option(), CC.DIMS)
    for smooth, decimate in CH.stage_pairs():
        got = CH.check(dev, 0.0, smooth, decimate, "fresh")
        assert got["extracted"] == (0, 0) and len(got["vertices"]) == 0 and len(got["faces"]) == 0


def test_second_mesh_on_one_context_pooled_buffers_and_the_capacity_rerun():
    """A small mesh first, then a larger one on the same context: the capacity guesses of the first extraction are too
    small for the second (the chain takes the re-run's counts), and every pool holds rows left over."""
    sdf, cnt, iso = CH.finite_random_state()
    small = sdf.copy()
    small.reshape(CC.DIMS[::-1])[:, :, 3:] = 1.0   # (solid voxels at x < 3 only: a fraction of the mesh)
    dev = CH.make_dev(CC.option(), CC.DIMS)
    dev.upload(small, cnt)
    first = CH.check(dev, iso, CH.SMOOTHS[3], CH.DECIMATES[8], "small state")
    dev.upload(sdf, cnt)
    for smooth, decimate in CH.stage_pairs():
        got = CH.check(dev, iso, smooth, decimate, "large state behind the small one")
    assert got["extracted"][1] > first["extracted"][1] * 5 // 4 + 4096   # (beyond the guess's headroom: a quarter and 4096)
    dev.upload(small, cnt)
    CH.check(dev, iso, CH.SMOOTHS[3], CH.DECIMATES[8], "small state again")
    dev.reset()                                     # ... and a carved sphere behind the random states, on the same context
    for view, mask in zip(*CH.small_sphere_inputs()):
        assert dev.CarveSilhouette(view, mask)
    for smooth, decimate in CH.stage_pairs():
        got = CH.check(dev, 0.0, smooth, decimate, "sphere behind the random states")
    assert got["extracted"][1] > 100


# ---- 2. a reader of the state -------------------------------------------------------------------------------------------

def test_chain_reads_the_state_as_an_extraction_does():
    dev, twin = CH.make_dev(CH.sphere_inputs()[0]), CH.make_dev(CH.sphere_inputs()[0])
    smooth, decimate = CH.SMOOTHS[2], CH.DECIMATES[8]
    for step, write in (("carve", CH.carve_sphere), ("keep", lambda d: d.KeepComponents(0.0, largest=1)),
                        ("redistance", lambda d: d.Redistance(0.0, 4))):
        write(dev)
        write(twin)
        CH.check(dev, 0.0, smooth, decimate, step, ref_dev=twin)
    a, b = dev.ExtractIsoSurface(0.0, True, normals=True), twin.ExtractIsoSurface(0.0, True, normals=True)
    for key in ("vertices", "faces", "normals", "face_normals"):
        assert np.array_equal(CH.bits(a[key]), CH.bits(b[key])), key
    sa, sb = dev.download(), twin.download()
    assert np.array_equal(CH.bits(sa[0]), CH.bits(sb[0])) and np.array_equal(sa[1], sb[1])


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------

BAD_SMOOTH = {"iterations -1": dict(iterations=-1), "iterations 10001": dict(iterations=10001), "lambda nan": dict(lam=float("nan")),
              "lambda inf": dict(lam=float("inf")), "mu nan": dict(mu=float("nan")), "mu -inf": dict(mu=float("-inf")),
              "pin 2": dict(pin_boundary=2), "pin -1": dict(pin_boundary=-1)}
BAD_DECIMATE = {"cell 0": dict(cell=0.0), "cell -1": dict(cell=-1.0), "cell nan": dict(cell=float("nan")), "cell inf": dict(cell=float("inf")),
                "origin nan": dict(origin=(float("nan"), 0.0, 0.0)), "origin inf": dict(origin=(0.0, 0.0, float("inf"))),
                "mode -1": dict(mode=-1), "mode 3": dict(mode=3)}
BAD_QUADRIC = {"regularize nan": dict(regularize=float("nan")), "regularize -1": dict(regularize=-1.0), "regularize 2": dict(regularize=2.0),
               "quadric from NEAREST": dict(regularize=1e-3, mode=capi.VCY_DECIMATE_NEAREST)}


def refused(dev, iso, smooth, decimate):
    with pytest.raises(RuntimeError) as e:
        dev.ExtractIsoChain(iso, True, smooth, decimate)
    return e.value.rc


def separate_rc(dev, smooth, decimate):
    """The code the separate calls give for the same options, on a mesh they would otherwise accept."""
    v, f = np.zeros((3, 3), np.float32), np.array([[0, 1, 2]], np.int32)
    with pytest.raises(RuntimeError) as e:
        if smooth is not None:
            dev.SmoothMesh(v, f, smooth["iterations"], smooth["lam"], smooth["mu"], smooth["pin_boundary"])
        if decimate is not None and "regularize" in decimate:
            o = capi.DecimateOption(decimate["cell"], decimate.get("origin", (0.0, 0.0, 0.0)), decimate.get("mode", 0))
            keep, args, out = vc._quadric_args(v, f, 1.0, (0.0, 0.0, 0.0), decimate["regularize"], False)
            args = args[:4] + (C.byref(o),) + args[5:]
            vc._quadric_result(capi.load().vcy_decimate_mesh_quadric(dev.ctx, *args), keep, out)
        elif decimate is not None:
            dev.DecimateMesh(v, f, decimate["cell"], decimate.get("origin"), decimate["mode"])
    return e.value.rc


def test_refusals_carry_the_separate_calls_codes_and_leave_the_context_usable():
    dev, iso = random_dev()
    good_s, good_d, good_q = CH.SMOOTHS[1], CH.DECIMATES[1], CH.DECIMATES[8]
    n = 0
    for name, change in BAD_SMOOTH.items():
        bad = dict(good_s, **change)
        assert refused(dev, iso, bad, good_d) == separate_rc(dev, bad, None) == capi.VCY_ERR_INVALID_ARG, name
        n += 1
    for name, change in BAD_DECIMATE.items():
        bad = dict(good_d, **change)
        assert refused(dev, iso, good_s, bad) == separate_rc(dev, None, bad) == capi.VCY_ERR_INVALID_ARG, name
        n += 1
    for name, change in BAD_QUADRIC.items():
        bad = dict(good_q, **change)
        assert refused(dev, iso, None, bad) == separate_rc(dev, None, bad) == capi.VCY_ERR_INVALID_ARG, name
        n += 1
    assert n == 20
    lib = capi.load()
    o = dev.chain_option(good_s, good_d)
    m, mn, rep = capi.Mesh(), capi.MeshNormals(), capi.ChainReport()
    for field, value in (("smooth", 2), ("decimate", 3), ("decimate", -1), ("which", 4), ("maps", 2)):
        o2 = dev.chain_option(good_s, good_d)
        setattr(o2, field, value)
        assert lib.vcy_extract_iso_chain(dev.ctx, iso, 1, C.byref(o2), C.byref(m), C.byref(mn), C.byref(rep)) == capi.VCY_ERR_INVALID_ARG, field
    assert lib.vcy_extract_iso_chain(dev.ctx, iso, 1, None, C.byref(m), C.byref(mn), C.byref(rep)) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_extract_iso_chain(dev.ctx, iso, 1, C.byref(o), None, C.byref(mn), C.byref(rep)) == capi.VCY_ERR_INVALID_ARG
    assert lib.vcy_extract_iso_chain(dev.ctx, iso, 1, C.byref(o), C.byref(m), None, C.byref(rep)) == capi.VCY_ERR_INVALID_ARG
    CH.check(dev, iso, good_s, good_d, "right after the refusals")
    CH.check(dev, iso, good_s, good_q, "right after the refusals")


def test_slab_and_edge_key_contexts_are_refused():
    sdf, cnt, iso = CC.random_state()
    slab = CH.make_dev(CC.option(), CC.DIMS, z_range=(5, 11))
    assert refused(slab, iso, CH.SMOOTHS[1], None) == capi.VCY_ERR_UNSUPPORTED
    assert "z [5, 11)" in vc.last_error()
    dev, iso = random_dev()
    assert dev.ExtractIsoChain(iso, True, CH.SMOOTHS[1], CH.DECIMATES[8])["passes_ms"] > 0.0
    dev.set_param("meshkeys", 1)
    for smooth, decimate in ((None, None), (CH.SMOOTHS[1], CH.DECIMATES[1])):
        assert refused(dev, iso, smooth, decimate) == capi.VCY_ERR_UNSUPPORTED
        assert "meshkeys" in vc.last_error()
        ms = [C.c_float(-1.0) for _ in dev.CHAIN_MS]      # (a call refused for its context reports no times, not the last call's)
        assert capi.load().vcy_last_chain_ms(dev.ctx, *[C.byref(x) for x in ms]) == 0
        assert [x.value for x in ms] == [0.0] * 8
    dev.set_param("meshkeys", 0)
    CH.check(dev, iso, CH.SMOOTHS[1], CH.DECIMATES[1], "keys off again")


# ---- 4. timers, outputs that are not asked for --------------------------------------------------------------------------------

def test_timers_are_positive_for_the_stages_that_ran_and_zero_for_the_others():
    dev, iso = random_dev()
    S, D, Q = CH.SMOOTHS[1], CH.DECIMATES[1], CH.DECIMATES[8]
    for smooth, decimate, normals, ran in (
            (None, None, True, {"extract_ms", "normals_ms"}),
            (None, None, False, {"extract_ms"}),
            (S, None, True, {"extract_ms", "table_ms", "passes_ms", "normals_ms"}),
            (S, None, False, {"extract_ms", "table_ms", "passes_ms"}),
            (None, D, True, {"extract_ms", "cluster_ms", "faces_emit_ms", "normals_ms"}),
            (None, Q, False, {"extract_ms", "table_ms", "cluster_ms", "quadric_ms", "faces_emit_ms"}),
            (S, Q, True, {"extract_ms", "table_ms", "passes_ms", "cluster_ms", "quadric_ms", "faces_emit_ms", "normals_ms"})):
        got = dev.ExtractIsoChain(iso, True, smooth, decimate, normals=normals)
        assert ("normals" in got) == normals
        for key in dev.CHAIN_MS[:-1]:
            assert (got[key] > 0.0) if key in ran else (got[key] == 0.0), (CH.name_of(smooth, decimate), normals, key, got[key])
        assert got["wall_ms"] > 0.0
        if decimate is not None and "regularize" in decimate:
            assert got["quadric_ms"] < got["cluster_ms"]
    fresh = CH.make_dev(CC.option(), CC.DIMS).ExtractIsoChain(0.0, True, S, Q)
    assert all(fresh[key] == 0.0 for key in dev.CHAIN_MS[1:-1])


def test_one_kind_of_normals_and_no_maps():
    lib = capi.load()
    dev, iso = random_dev()
    want = CH.separate(dev, iso, CH.SMOOTHS[1], CH.DECIMATES[8])
    for which, key in ((capi.VCY_NORMALS_VERTEX, "normals"), (capi.VCY_NORMALS_FACE, "face_normals")):
        o = dev.chain_option(CH.SMOOTHS[1], CH.DECIMATES[8], maps=False)
        o.which = which
        m, mn, rep = capi.Mesh(), capi.MeshNormals(), capi.ChainReport()
        assert lib.vcy_extract_iso_chain(dev.ctx, iso, 1, C.byref(o), C.byref(m), C.byref(mn), C.byref(rep)) == 0, vc.last_error()
        assert (m.n_vertices, m.n_faces) == (len(want["vertices"]), len(want["faces"])) and not m.edge_keys
        assert bool(mn.vertex_normals) == (key == "normals") and bool(mn.face_normals) == (key == "face_normals")
        assert not rep.vertex_map and not rep.face_source and rep.n_fallback == want["n_fallback"]
        n = m.n_vertices if key == "normals" else m.n_faces
        got = vc._mesh_array(mn.vertex_normals if key == "normals" else mn.face_normals, n, 3, np.float32)
        assert np.array_equal(CH.bits(got), CH.bits(want[key])), key
        lib.vcy_mesh_free(C.byref(m))
        lib.vcy_mesh_normals_free(C.byref(mn))
        lib.vcy_chain_report_free(C.byref(rep))
    # no report, no normals
    o = dev.chain_option(CH.SMOOTHS[1], CH.DECIMATES[8], normals=False, maps=True)
    m = capi.Mesh()
    assert lib.vcy_extract_iso_chain(dev.ctx, iso, 1, C.byref(o), C.byref(m), None, None) == 0, vc.last_error()
    assert np.array_equal(CH.bits(vc._mesh_array(m.vertices, m.n_vertices, 3, np.float32)), CH.bits(want["vertices"]))
    lib.vcy_mesh_free(C.byref(m))


# ---- 5. the "mcdirect" default ---------------------------------------------------------------------------------------------

def test_a_mesh_small_enough_for_direct_emit_is_staged_all_the_same():
    dev, iso = random_dev()
    assert dev.get_param("mcdirect") > 0   # (the default: ExtractIsoSurface writes this mesh straight into host memory)
    CH.check(dev, iso, CH.SMOOTHS[1], None, "direct, chain first")
    plain = dev.ExtractIsoSurface(iso)
    CH.check(dev, iso, None, CH.DECIMATES[3], "direct, behind a direct extraction")
    again = dev.ExtractIsoSurface(iso)
    assert np.array_equal(CH.bits(plain["vertices"]), CH.bits(again["vertices"])) and np.array_equal(plain["faces"], again["faces"])
    dev.set_param("mcdirect", 0)
    CH.check(dev, iso, CH.SMOOTHS[1], CH.DECIMATES[8], "mcdirect 0")
