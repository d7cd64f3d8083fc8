#!/usr/bin/env python
"""tests/golden/conv_call_digests.json: sha256 of every tensor tests/test_conv_call_gpu.py hashes.  Run on an MI355X in a
checkout of the commit whose convolution entries are the reference (its own library built), with that commit's short
hash as the first argument and optionally the output path as the second.  Run it twice and compare the two files before
trusting them: a difference means a call leaves bytes unwritten.  Not run for a change of the call path: the point of
the file is that it stays."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "flair-for-aigle_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import test_conv_call_gpu as T  # noqa: E402

commit = sys.argv[1]
path = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
dev = torch.device("cuda:0")
digests = {}
for group in sorted(T.GROUPS):
    for name in T.SWITCHES:
        os.environ.pop(name, None)
    os.environ.update(T.GROUPS[group][0])
    digests.update(T.run_group(group, dev))
with open(path, "w") as f:
    json.dump({"recorded": f"tests/golden/gen_conv_call_digests.py at commit {commit} on {torch.cuda.get_device_name(0)}",
               "digests": digests}, f, indent=1, sort_keys=True)
    f.write("\n")
print(len(digests), "digests ->", path)
