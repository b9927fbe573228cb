"""The states, the option matrix and the separate route of the extraction chain's tests (vcy_extract_iso_chain; definition:
include/vacancy_hip.h, "extraction chain").  The chain is by definition the bits of the separate calls in a row, so the
reference of every test is `separate` on the same context or on a twin."""
import numpy as np

import color_cases as CC
import test_gpu_render as TR
from vacancy_amd import capi, synth
from vacancy_amd import carver as vc
from vacancy_amd.capi import CarverOption

F = np.float32
TAUBIN = dict(lam=0.5, mu=-0.53)
LONG_DIMS = (130, 6, 5)   # rows of three 64-bit cell words; cells at x = 1 and x = nx - 1

# the stages: None, or the keywords of ExtractIsoChain's `smooth` / `decimate`
SMOOTHS = [None] + [dict(iterations=it, pin_boundary=pin, **TAUBIN) for it in (1, 7) for pin in (0, 1)]
DECIMATES = [None] + [dict(cell=cell, mode=mode) for cell in (2.0, 3.7)
                      for mode in (capi.VCY_DECIMATE_MEAN, capi.VCY_DECIMATE_NEAREST, capi.VCY_DECIMATE_FIRST)] + \
            [dict(cell=cell, regularize=reg) for cell in (2.0, 3.7) for reg in (0.0, 1e-3)]


def full_matrix():
    return [(s, d) for s in SMOOTHS for d in DECIMATES]


def stage_pairs():
    """Every kind of stage pair once: smoothing off / on with either pin, against no decimation, each clustering mode and
    quadric representatives with either regularisation; both cell sizes and both iteration counts occur."""
    s1, s7 = SMOOTHS[2], SMOOTHS[3]   # (1 iteration pinned, 7 iterations unpinned)
    mean2, near37, first2, q0, q1 = DECIMATES[1], DECIMATES[5], DECIMATES[3], DECIMATES[9], DECIMATES[8]
    return [(None, None), (s1, None), (s7, None), (None, mean2), (None, q1), (s1, mean2), (s7, near37), (s1, first2), (s7, q0), (s1, q1)]


def name_of(smooth, decimate):
    s = "s-" if smooth is None else "s%d%s" % (smooth["iterations"], "p" if smooth["pin_boundary"] else "")
    if decimate is None:
        return s + " d-"
    kind = "q%g" % decimate["regularize"] if "regularize" in decimate else "m%d" % decimate["mode"]
    return "%s d%s@%g" % (s, kind, decimate["cell"])


# ---- contexts and states ---------------------------------------------------------------------------------------------

ROWS = (0, 1)   # "chainrows": the corner table from the faces (mesh_rows.h) / from the cells (mc_corner_rows)
_rows = [1]


def use_rows(value):
    """The "chainrows" every context of make_dev gets from here on (the fixture of test_gpu_chain.py sets it per test)."""
    _rows[0] = int(value)


def make_dev(opt, dims=None, z_range=None):
    dev = TR.make_dev(opt, dims, z_range)
    dev.set_param("meshkeys", 0)   # (the chain's mesh has no edge keys)
    dev.set_param("chainrows", _rows[0])
    assert dev.get_param("chainrows") == _rows[0]
    return dev


def finite_random_state():
    """color_cases.random_state() with its NaN voxels made empty space: every vertex is finite, so the decimation accepts
    the mesh (the random state itself has NaN vertices, which vcy_decimate_mesh refuses -- and the chain with it)."""
    def make():
        sdf, cnt, iso = CC.random_state()
        return np.where(np.isnan(sdf), F(0.5), sdf).astype(F), cnt, iso
    return CC.memo("chain_finite_state", make)


def small_sphere_inputs():
    """Views of a sphere of radius 5.6 that fits the grid of color_cases.DIMS."""
    return CC.memo("chain_small_sphere", lambda: synth.sphere_views(16, 4, 160, 120))


def long_option():
    h = [e / 2.0 for e in LONG_DIMS]
    return CarverOption(bb_min=[-x for x in h], bb_max=h, resolution=1.0)


def long_state():
    """A seeded random state on LONG_DIMS: (sdf, cnt, iso)."""
    def make():
        n = int(np.prod(LONG_DIMS))
        rng = np.random.RandomState(71)
        sdf = (rng.rand(n) - 0.35).astype(F)
        return sdf, np.ones(n, np.int32), 0.0
    return CC.memo("chain_long_state", make)


def sphere_inputs():
    return CC.memo("chain_sphere", lambda: (synth.sphere_option(32),) + tuple(synth.sphere_views(32, 4, 160, 120)))


def carve_sphere(dev):
    _, views, masks = sphere_inputs()
    for view, mask in zip(views, masks):
        assert dev.CarveSilhouette(view, mask)


def sphere_dev():
    dev = make_dev(sphere_inputs()[0])
    carve_sphere(dev)
    return dev


def voxel_value_iso(dev):
    """An iso level that IS a voxel value of the carved sphere, near the surface: the 1e-5 snaps of VertexInterp."""
    sdf = dev.download()[0]
    inside = np.sort(sdf[(sdf > -3.0e38) & (sdf < 0.0)])
    assert len(inside) >= 8
    return float(inside[-(len(inside) // 8)])


# ---- the separate route ----------------------------------------------------------------------------------------------

def separate(dev, iso, smooth, decimate, linear_interp=True):
    """Today's route on `dev`: ExtractIsoSurface -> SmoothMesh -> DecimateMesh[Quadric], the last one with normals=True.
    The keys the chain returns."""
    both_off = smooth is None and decimate is None
    m = dev.ExtractIsoSurface(iso, linear_interp, normals=both_off)
    out = {"vertices": m["vertices"], "faces": m["faces"], "extracted": (len(m["vertices"]), len(m["faces"]))}
    if both_off:
        out["normals"], out["face_normals"] = m["normals"], m["face_normals"]
    if smooth is not None:
        s = dev.SmoothMesh(out["vertices"], out["faces"], smooth["iterations"], smooth["lam"], smooth["mu"], smooth["pin_boundary"],
                           normals=decimate is None)
        out.update({k: s[k] for k in ("vertices", "normals", "face_normals") if k in s})
    if decimate is not None:
        if "regularize" in decimate:
            d = dev.DecimateMeshQuadric(out["vertices"], out["faces"], decimate["cell"], None, decimate["regularize"], normals=True)
            out["n_fallback"] = d["n_fallback"]
        else:
            d = dev.DecimateMesh(out["vertices"], out["faces"], decimate["cell"], None, decimate["mode"], normals=True)
        out.update({k: d[k] for k in ("vertices", "faces", "normals", "face_normals", "vertex_map", "face_source")})
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def assert_equal(got, want, ctx):
    """Bit equality of vertices, faces, both normals, the maps, the counts and n_fallback."""
    assert got["extracted"] == want["extracted"], ctx
    for key in ("vertices", "faces", "normals", "face_normals", "vertex_map", "face_source"):
        assert (key in got) == (key in want), (ctx, key)
        if key in want:
            assert got[key].shape == want[key].shape, (ctx, key, got[key].shape, want[key].shape)
            same = bits(got[key]) == bits(want[key])
            assert same.all(), "%s: %s differs at %d of %d entries" % (ctx, key, same.size - int(same.sum()), same.size)
    assert got.get("n_fallback") == want.get("n_fallback"), ctx


def check(dev, iso, smooth, decimate, ctx, ref_dev=None, linear_interp=True):
    """The chain against the separate route: the same bits, or -- where a separate call refuses the mesh it is given, as the
    decimation does for a vertex that is not finite -- the same refusal.  Returns the chain's dict, or None after a refusal."""
    ctx = "%s %s" % (ctx, name_of(smooth, decimate))
    try:
        want = separate(ref_dev or dev, iso, smooth, decimate, linear_interp)
    except RuntimeError as e:
        want = e.rc
    try:
        got = dev.ExtractIsoChain(iso, linear_interp, smooth, decimate, normals=True, maps=True)
    except RuntimeError as e:
        assert e.rc == want, (ctx, e.rc, want, str(e))
        return None
    assert not isinstance(want, int), (ctx, "the separate route refuses with %r" % (want,))
    assert_equal(got, want, ctx)
    return got
