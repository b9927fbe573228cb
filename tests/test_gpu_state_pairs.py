"""The pair matrix of tests/state_model.py: for every option set and every ordered pair (A, B) of the writers of the voxel state
it admits -- the fused carve, the per-view kernel, queued per-view calls, the streamed silhouette batch, the depth carve, the
robust carve, the component filter, vcy_upload, vcy_reset -- on a context whose state was CARVED and whose every cache is
populated: A, every reader against the model, B, every reader against the model, one more fused carve with view dropping,
download and marching cubes with brick skipping.  Bit for bit; a stale flag shows as a skipped brick, a dropped view, last
call's hull or last state's mesh.  The pairs that hold a writer which does not go through the fused kernel run on two z-slab
contexts as well, where after EVERY writer the upper slab must refuse to extract until the halos are exchanged, and must still
download, render and label correctly before that."""
import pytest

import state_model as SM

pytestmark = pytest.mark.gpu

WHOLE = [(s, d, None, a, b) for s in SM.OPTION_SETS for d in SM.SHAPES for a in SM.writers_of(s) for b in SM.writers_of(s)]
SLABS = [(s, d, SM.PAIR_CUT[d], a, b) for s, d, _, a, b in WHOLE if a in SM.NEW_WRITERS or b in SM.NEW_WRITERS]


def case_id(c):
    return "%s-%dx%dx%d-%s-%s-%s" % (c[0], c[1][0], c[1][1], c[1][2], "whole" if c[2] is None else "cut%d" % c[2], c[3], c[4])


@pytest.mark.parametrize("case", WHOLE, ids=case_id)
def test_pair_on_the_whole_grid(case):
    SM.run_pair(*case)


@pytest.mark.parametrize("case", SLABS, ids=case_id)
def test_pair_on_two_slabs(case):
    SM.run_pair(*case)
