"""Seeded sequences of writers AND readers of the voxel state (tests/state_model.py: script): an option set, a shape, the whole
grid or two z-slabs at one of the cuts, a random setting of "defer", "livelist", "coopstore", "rowkernel" and "oneview", and
8 - 12 operations, so that a cache is sometimes warm and sometimes not when a writer runs.  The state is compared with the
model after every writer, every reader after the last operation; on slabs the halo contract is checked after every writer.
tests/fuzz/fuzz_state_sequences.py runs any range of seeds of the same generator."""
import pytest

import state_model as SM

pytestmark = pytest.mark.gpu


def seed_id(seed):
    s = SM.script(seed)
    return "%d-%s-%dx%dx%d-%s" % ((seed, s["option_set"]) + s["dims"] + ("whole" if s["cut"] is None else "cut%d" % s["cut"],))


@pytest.mark.parametrize("seed", SM.SEEDS, ids=seed_id)
def test_sequence(seed):
    SM.run_script(SM.script(seed))
