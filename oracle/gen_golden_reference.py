#!/usr/bin/env python3
"""TEST INFRASTRUCTURE: tests/golden/reference_answers.npz -- the answers of the reference's own code (oracle/_ref) to
every call the CPU tests put to it through the `reference` fixture (tests/conftest.py), recorded by running those tests
against the live build.  The tests then replay them (binding.RecordedReference), so that they compare the oracle with
the reference where the reference tree is absent.  Run in the build container (needs the reference tree):

    python oracle/gen_golden_reference.py
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import pytest  # noqa: E402

from oracle import binding as ob  # noqa: E402

ob.build(ref=True)
rec = ob.ReferenceRecorder(ob.Reference())
ob.RecordedReference = lambda path=None: rec  # the `reference` fixture hands the tests the live, recording reference
rc = pytest.main([os.path.join(ROOT, "tests", f) for f in ("test_egomotion.py", "test_mono.py", "test_oracle.py", "test_outliers.py",
                                                                "test_egomotion_edges.py", "test_mono_edges.py")]
                 + ["-q", "-m", "not gpu", "-p", "no:cacheprovider"])
assert rc == 0, "the tests must pass against the live reference before its answers are recorded"
rec.save(ob.REFERENCE_ANSWERS)
print(len(rec.answers), "calls recorded:", ob.REFERENCE_ANSWERS + "_*.npz")
