"""The conditions that keep tests/test_gpu_state_pairs.py and tests/test_gpu_state_sequences.py from passing vacuously, checked on
the model alone (tests/state_model.py; no GPU): every writer changes the base state, the states have something to extract, to
render and to label, the collected seeds cover what they are meant to cover, and the model agrees with itself."""
import os
import subprocess
import time

import numpy as np
import pytest

import depth_ref as DR
import state_model as SM

CASES = [(s, d) for s in SM.OPTION_SETS for d in SM.SHAPES]
case_id = lambda c: "%s-%dx%dx%d" % ((c[0],) + c[1])  # noqa: E731


def differs(a, b):
    return bool((a[0].view(np.uint32) != b[0].view(np.uint32)).any() or (a[1] != b[1]).any())


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_every_writer_changes_the_base_state(case):
    m = SM.model(*case)
    base = m.state(())
    assert len(m.components(())[0]["label"]) >= 2, "the base state has no second component for the filter to remove"
    for w in SM.writers_of(case[0]):
        after = m.state((w,))
        assert differs(after, base), "%s leaves the base state as it is" % w
        if w == "filter":
            gone = (after[0] != base[0]) & (base[0] < 0)
            assert gone.sum() >= 1 and (after[0][gone] == 1.0).all()
        for second in SM.writers_of(case[0]):  # B after A: only a reset that follows a reset may change nothing
            if second == "reset" and (w, second) != ("reset", "reset"):
                assert differs(m.state((w, second)), after), (w, second)
    assert not differs(m.state(("reset", "reset")), m.state(("reset",)))


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_states_are_not_empty(case):
    m = SM.model(*case)
    for ops in [()] + [(w,) for w in SM.writers_of(case[0])]:
        faces = len(m.mesh(ops)["faces"])
        pixels = sum(int(np.isfinite(d).sum()) for iso in SM.RENDER_ISOS for d, _, _ in m.render(ops, iso))
        comps = len(m.components(ops)[0]["label"])
        kept = len(m.kept_voxels(ops))
        if ops == ("reset",):  # the fill state: nothing to extract, to hit or to label -- said here, not passed over
            assert (faces, pixels, comps) == (0, 0, 0)
            assert len(m.voxel_mesh(ops, True)["faces"]) == 0
        else:
            assert faces > 0 and comps >= 1 and kept > 0, (ops, faces, comps, kept)
            assert all(np.isfinite(d).any() for d, _, _ in m.render(ops, 0.0)), ops
            assert (m.color(ops, 0.0)[1] > 0).any(), "%s: no view colours any point" % (ops,)
    # the two iso levels of the render give different images of every view: the kept bit planes have to follow the level.  (The
    # normalised silhouette SDF of a 48 x 40 image does not go below -0.33, so at -0.3 the hull of the kMax sets is EMPTY, or
    # the upload's floater alone: planes kept from level 0 show as hits where there are none, and the other way round.  With
    # truncation it is a smaller hull.)
    for ops in [()] + [(w,) for w in SM.writers_of(case[0]) if w != "reset"]:
        assert all(not np.array_equal(a[1], b[1]) for a, b in zip(m.render(ops, 0.0), m.render(ops, -0.3))), ops
    if case[0] == "tsdf":
        assert all(np.isfinite(d).any() for d, _, _ in m.render((), -0.3))


def test_depth_lowers_a_brick_minimum_below_the_iso_level():
    """What makes brick minima kept across a depth carve WRONG: a brick that the base state leaves entirely above the iso level
    (marching cubes with brick skipping would not read it) and in which the depth carve puts a voxel below it.  Only weighted
    averaging can do that -- under kMax a sample only ever raises a voxel, so there the minima would merely be cautious."""
    dims = (64, 16, 18)
    nx, ny, nz = dims

    def crossing(option_set):
        m = SM.model(option_set, dims)
        b, a = m.state(())[0].reshape(nz, ny, nx), m.state(("depth",))[0].reshape(nz, ny, nx)
        return sum(b[z:z + 8, y:y + 8, x:x + 8].min() > 0.0 > a[z:z + 8, y:y + 8, x:x + 8].min()
                   for z in range(0, nz, 8) for y in range(0, ny, 8) for x in range(0, nx, 8))

    assert crossing("tsdf") >= 1
    assert crossing("max") == 0 and crossing("max_update_4") == 0


def test_collected_seeds_cover_writers_readers_options_and_layouts():
    scripts = [SM.script(s) for s in SM.SEEDS]
    n = len(scripts)
    for w in SM.WRITERS:
        assert sum(w in s["ops"] for s in scripts) >= 3, w
    follows = {(a, b) for s in scripts for a, b in zip(s["ops"][:-1], s["ops"][1:])}
    missing = [(w, r) for w in SM.WRITERS for r in SM.READERS if (w, r) not in follows]
    assert not missing, missing
    for name in SM.OPTION_SETS:
        assert sum(s["option_set"] == name for s in scripts) * 5 >= n, name
    for dims in SM.SHAPES:
        assert sum(s["dims"] == dims for s in scripts) * 5 >= n, dims
    assert sum(s["cut"] is None for s in scripts) * 5 >= n and sum(s["cut"] is not None for s in scripts) * 5 >= n
    for dims in SM.SHAPES:
        assert {s["cut"] for s in scripts if s["dims"] == dims and s["cut"] is not None} == set(SM.CUTS[dims]), dims
    for s in scripts:
        assert 8 <= len(s["ops"]) <= 12
        assert set(s["ops"]) <= set(SM.writers_of(s["option_set"])) | set(SM.READERS if s["cut"] is None else SM.SLAB_READERS)
        assert s["cut"] is None or 2 <= s["cut"] <= s["dims"][2] - 2
    assert SM.script(7) == SM.script(7)
    # every parameter the scripts draw takes every value it can
    for key, values in (("defer", {0, 1}), ("livelist", {0, 1}), ("coopstore", {-1, 0, 1}), ("rowkernel", {-1, 0, 2}),
                        ("oneview", {0, 1})):
        assert {s["params"][key] for s in scripts} == values, key


def test_pair_cuts_are_legal_slabs():
    for dims in SM.SHAPES:
        for cut in SM.CUTS[dims] + [SM.PAIR_CUT[dims]]:
            assert 2 <= cut <= dims[2] - 2, (dims, cut)   # a slab above the first starts at z >= 2 and every slab has 2 slices
        assert min(SM.CUTS[dims]) == 2 and max(SM.CUTS[dims]) == dims[2] - 2
        assert any(c % 8 == 0 for c in SM.CUTS[dims]) and any(c % 8 for c in SM.CUTS[dims])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_slices_of_a_writer_equal_the_writer_on_slices(case):
    m = SM.model(*case)
    base = m.state(())
    views, depths = m.inputs("depth")
    whole = m.state(("depth",))
    up = m.state(("upload",))
    for cut in SM.CUTS[case[1]]:
        for z0, z1 in ((0, cut), (cut, case[1][2])):
            s, c = m.slab(base, z0, z1)
            part = DR.carve_depth(m.opt, views, depths, SM.DEPTH_BAND, s, c, z_range=(z0, z1))
            assert not differs(part, m.slab(whole, z0, z1)), ("depth", cut, z0)
            # the upload's pattern is a function of the GLOBAL voxel id: a slab is handed the slices of the whole array
            sl = m.slab(m.upload_arrays(base), z0, z1)
            assert not differs(sl, m.slab(up, z0, z1)), ("upload", cut, z0)


def test_memoised_results_are_read_only_and_unchanged_by_later_operations():
    m = SM.model("max", SM.SHAPES[0])
    base = m.state(())
    copy = (base[0].copy(), base[1].copy())
    mesh = {k: v.copy() for k, v in m.mesh(()).items()}
    for w in SM.writers_of("max"):
        m.state((w, "filter"))
        m.state((w, "upload", SM.CLOSE))
    assert m.state(()) is base and not differs(base, copy)
    assert m.state(("render", "mc")) is base, "readers in a tuple of operations do not change the key"
    for a in base:
        with pytest.raises(ValueError):
            a[0] = 1
    assert all(np.array_equal(v, m.mesh(())[k]) for k, v in mesh.items())


def test_model_time_per_pair_case():
    """The CPU share of a case of the pair matrix, with the prefixes memoised as the GPU module has them: printed, and held
    to the few seconds a case of the suite may take."""
    dims, name = SM.SHAPES[1], "max"
    m = SM.Model(name, dims)  # (a model of its own: nothing memoised yet)
    t0 = time.perf_counter()
    pairs = [("depth", b) for b in SM.writers_of(name)]
    for a, b in pairs:
        for ops in ((), (a,), (a, b)):
            m.mesh(ops), m.voxel_mesh(ops, True), m.voxel_mesh(ops, False), m.components(ops)
            for iso in SM.RENDER_ISOS:
                m.render(ops, iso), m.color(ops, iso)
        m.mesh((a, b, SM.CLOSE))
    per_case = (time.perf_counter() - t0) / len(pairs)
    print("model time per pair case at %s: %.2f s" % (dims, per_case))
    assert per_case < 3.0


def test_state_flags_follow_the_transition_table_under_host_sanitizers():
    """The stand-alone program of tests/state_flags_host_check.cpp: every writer's declaration from every reachable combination
    of what a context keeps beside its state (vacancy_amd/csrc/state_flags.h), against the table written out there as data,
    under AddressSanitizer and UBSan, on the CPU."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    run = subprocess.run(["make", "-C", os.path.join(root, "vacancy_amd", "csrc"), "-s", "state_flags_host_check"],
                         capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "state_flags_host_check: ok" in run.stdout
