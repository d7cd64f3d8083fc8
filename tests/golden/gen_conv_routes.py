#!/usr/bin/env python
"""tests/golden/conv_routes.json: the answers of the public convolution queries of flairhip.ops that
tests/test_conv_route_cpu.py compares.  Run in a checkout of the commit whose rules are the reference (its own library
built; no GPU needed: the queries launch nothing), with that commit's short hash as the first argument and optionally
the output path as the second.  Not run for a change of the call path: the point of the file is that it stays."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "flair-for-aigle_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_conv_route_cpu as T  # noqa: E402

commit = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
answers = T.answers()
with open(path, "w") as f:
    json.dump({"recorded": f"tests/golden/gen_conv_routes.py at commit {commit}", "answers": answers}, f, indent=1,
              sort_keys=True)
    f.write("\n")
print(len(answers["operands"]), "operands ->", path)
