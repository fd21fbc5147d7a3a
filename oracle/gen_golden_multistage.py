"""Record tests/golden/multistage_answers.npz -- TEST INFRASTRUCTURE ONLY.

Counts and SHA-256 of the sparse list, the range table and the pass-2 list that tests/multistage_oracle.py's
restatement of multi-stage matching gives on fixed synthetic frames.  The answers are the restatement's own as of the
commit that records them, not the reference's (it has nothing behind use_prior): the file only makes a later edit of
the restatement visible.  Run from the repository root: python oracle/gen_golden_multistage.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import __graft_entry__ as entry  # noqa: E402
import multistage_oracle as mo  # noqa: E402
from test_multistage_scale import answer_cases  # noqa: E402


def main():
    pkg, ob = entry.load_package(), entry.load_oracle()
    ans = mo.recorded_answers(ob, ob.Oracle(), answer_cases(pkg))
    names = sorted(ans)
    path = os.path.join(ROOT, "tests", "golden", "multistage_answers.npz")
    np.savez(path, names=np.array(names), counts=np.array([ans[n][0] for n in names], np.int32),
             sha256=np.array([ans[n][1] for n in names]))
    for n in names:
        print(n, ans[n][0])
    print("wrote", path)


if __name__ == "__main__":
    main()
