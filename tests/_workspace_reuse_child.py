"""Child of tests/test_workspace_reuse_cpu.py: tests/workspace_reuse.py's case lists on the CPU stand-in of the HIP runtime.  Run with
MODGPU_LIB naming the stand-in build of the library (`make standin-lib`), MODGPU_REQUIRE_GPU=0 and MODGPU_SHIM_DEVICES=1; prints one line
per list and, last, "workspace reuse on the stand-in: ok"."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import modulate_amd as M  # noqa: E402
from oracle import oracle as O  # noqa: E402
import workspace_reuse as R  # noqa: E402


def main():
    assert os.environ.get("MODGPU_LIB"), "runs only against the stand-in build"
    O.build(ref=False)
    K = R.Keystreams(O)
    S = R.Standin(M)
    t0 = time.time()
    with R.rig(S, K, R.all_cases()) as r:
        for fill, kind in R.FILL_CASES:
            R.run_fill(r, fill, kind)
        print(f"fills: {len(R.FILL_CASES)} ({time.time() - t0:.1f} s)", flush=True)
        for prev in R.KINDS:
            R.run_pairs(r, prev)
        print(f"pairs: {len(R.PAIR_CASES)} ({time.time() - t0:.1f} s)", flush=True)
        for prev in R.REFUSAL_PREVIOUS:
            R.run_refusals(r, prev)
        R.run_verify_summaries(r)
        R.run_move_statuses(r)
        R.run_checks(r)
        for kind in R.ALIGN_CASES:
            R.run_aligned(r, kind)
        print(f"refusals, readers, alignment ({time.time() - t0:.1f} s)", flush=True)
    assert R.PASSED == set(R.FILL_CASES)
    print("workspace reuse on the stand-in: ok")


if __name__ == "__main__":
    main()
