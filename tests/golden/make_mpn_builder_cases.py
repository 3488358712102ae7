"""Generates tests/golden/mpn_builder_cases.json: per case of tests/mpn_builder_cases.py and per builder call, the sha256 of the work bytes
(withdraw_signed: of the instance's z) and the root the call leaves, AS THE HOST BUILDER OF THE LIBRARY IN THE TREE computes them.  Recorded
results only: the file pins the host builder's output across a rewrite of the builders, so it is made on the commit BEFORE such a rewrite and
must not be regenerated with it.

    python tests/golden/make_mpn_builder_cases.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mpn_builder_cases as M  # noqa: E402

if __name__ == "__main__":
    out = {}
    for name in M.CASES:
        out[name] = M.digest(M.run(name))
        print(name, len(out[name]), "calls", flush=True)
    json.dump(out, open(M.GOLDEN, "w"), indent=1, sort_keys=True)
