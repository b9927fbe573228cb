"""Long-running form (not collected by pytest) of tests/test_gpu_state_sequences.py: the sequences of writers and readers of
tests/state_model.py for any range of seeds -- every writer of the voxel state (fused and per-view carves, queued views, the
streamed batch, the depth and the robust carve, the component filter, vcy_upload, vcy_reset) against every reader that keeps
something derived from it, on one context and on two z-slabs, compared with the CPU model bit for bit.
usage: python tests/fuzz/fuzz_state_sequences.py FIRST_SEED LAST_SEED"""
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import state_model as SM  # noqa: E402

lo, hi = int(sys.argv[1]), int(sys.argv[2])
bad = 0
t0 = time.time()
for seed in range(lo, hi):
    s = SM.script(seed)
    try:
        SM.run_script(s)
    except AssertionError as e:
        bad += 1
        print("MISMATCH seed %d %s %s cut %s params %s\n  ops %s\n  %s" % (seed, s["option_set"], s["dims"], s["cut"], s["params"],
                                                                          s["ops"], e), flush=True)
    if (seed - lo) % 10 == 9:
        print("  ... seed %d, %d mismatches so far, %.0f s" % (seed, bad, time.time() - t0), flush=True)
print("state sequences, seeds %d..%d done, %d mismatches, %.0f s" % (lo, hi, bad, time.time() - t0))
sys.exit(1 if bad else 0)
