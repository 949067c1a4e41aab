"""CPU: the five plan queries of lr_gemm_conv_f16 (host code) answer exactly what tests/golden/gemm_plans.npz recorded
(tools/make_golden_gemm_plans.py: the keys of tile_table.json and a grid over tiles, epilogues, split-K, the phase form, the 16-channel
source and the skip extension).  The front end sizes its statistics buffers and the workspace from these answers."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gemm_plan_queries_match_the_recorded_answers():
    from leftrefill_amd import _lib, build
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_golden_gemm_plans as gen
    finally:
        sys.path.pop(0)
    build.build(verbose=False)
    lib = _lib.load()
    gold = np.load(os.path.join(ROOT, "tests", "golden", "gemm_plans.npz"))
    cases = gen.cases()
    assert np.array_equal(np.asarray(cases, dtype=np.int32), gold["cases"]), "the case generator and the fixture disagree: record again"
    assert len(cases) >= 15000 and gold["answers"].dtype == np.int32
    got = np.asarray([gen.answers(lib, c) for c in cases], dtype=np.int64)
    bad = np.nonzero((got != gold["answers"]).any(axis=1))[0]
    assert bad.size == 0, [(dict(zip(gen.FIELDS, cases[i])), dict(zip(gen.ANSWERS, got[i])), dict(zip(gen.ANSWERS, gold["answers"][i])))
                           for i in bad[:5]]
    gen.check_coverage(cases, got)
