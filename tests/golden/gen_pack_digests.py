#!/usr/bin/env python
"""tests/golden/pack_digests.json: sha256 of every operand tests/test_pack_layouts_gpu.py packs, with the bco the planner
returned.  Run on an MI355X in a checkout of the commit whose packers are the reference (its own library built), with
that commit's short hash as the first argument and optionally the output path as the second; the one-off and the batched
pack must already agree there.  Not run for a change of the packing code: the point of the file is that it stays."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "flair-for-aigle_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_pack_layouts_gpu as T  # noqa: E402

commit = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
dev = torch.device("cuda:0")
digests = {}
for layout in sorted(T.GROUPS):
    for name in T.SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(T.GROUPS[layout][1])
    for key, (bco, one, batched) in T.pack_group(layout, dev).items():
        assert batched in (None, one), key
        digests[key] = {"bco": bco, "sha256": one}
with open(path, "w") as f:
    json.dump({"recorded": f"tests/golden/gen_pack_digests.py at commit {commit} on {torch.cuda.get_device_name(0)}",
               "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
print(len(digests), "digests ->", path)
