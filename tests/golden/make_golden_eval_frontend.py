#!/usr/bin/env python
"""Generate tests/golden/eval_frontend.json: what evaluate() and predict wrote for the runs of tests/eval_frontend_cases.py - write_json's
file, write_csv's rows, predict's rows and CSV - and how often each stage was called per batch.

Recorded on the commit BEFORE the evaluation front end was rearranged (the probability stage moved to uda_clr_amd/inference.py, the packed
tables got one layout each); tests/test_eval_frontend_cpu.py holds every later commit to it.  Needs no GPU: every device stage is
replaced by its host restatement.  To record from another checkout of the package, name its root in UDA_CLR_PACKAGE_ROOT:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_eval_frontend.py
"""
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.environ.get("UDA_CLR_PACKAGE_ROOT", os.path.dirname(os.path.dirname(HERE))))


def main():
    import pytest
    import eval_frontend_cases as cases
    import uda_clr_amd
    patch = pytest.MonkeyPatch()
    try:
        with tempfile.TemporaryDirectory() as tmp:
            runs = cases.run_all(patch, tmp)
    finally:
        patch.undo()
    with open(os.path.join(HERE, "eval_frontend.json"), "w") as f:
        json.dump(runs, f, indent=1)
        f.write("\n")
    print("eval_frontend: recorded from %s" % os.path.dirname(uda_clr_amd.__file__))
    for name, run in runs.items():
        print("  %-13s calls per batch %s" % (name, run["calls"]))


if __name__ == "__main__":
    main()
