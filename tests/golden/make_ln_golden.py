"""Records tests/golden/ln_row_sha1.json: the sha1 of the output bytes of every case of tests/test_gpu_ln_pins.py, on the MI355X.

The record is what the normalising kernels must keep computing, so it is made with a library built from a commit whose kernels are trusted -- the
parent of the change under test -- and never from the change itself: check that commit out into a worktree, copy tests/test_gpu_ln_pins.py and
this file into it, build, and run there, from the worktree's root:

    python tests/golden/make_ln_golden.py [--commit SHA] [--out FILE]

The package imported is the one beside this file's tests/ directory.  The JSON states the recording commit: `git rev-parse HEAD` of that tree,
or --commit where the tree is not a git checkout."""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]
import _pkg  # noqa: E402
import test_gpu_ln_pins as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", default=None)
ap.add_argument("--out", default=T.GOLDEN)
a = ap.parse_args()
commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
import torch  # noqa: E402
if not torch.cuda.is_available():
    sys.exit("make_ln_golden.py needs the GPU: the record is what the kernels compute")
pkg = _pkg.load()
from vitcpp_amd import binding  # noqa: E402
out = {"commit": commit, "sha1": {}}
for name in T.CASES:
    out["sha1"][name] = T.sha1_of(pkg, binding, torch, name)
with open(a.out, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(f"wrote {a.out}: {len(out['sha1'])} cases, recorded on {commit}")
