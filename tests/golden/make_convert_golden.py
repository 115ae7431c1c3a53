"""Records tests/golden/convert_sha1.json: the sha1 of the file vit.cpp_amd/convert.py writes for every case of tests/test_cpu_convert_pins.py.

The record is what the converter must keep writing, so it is made on a commit whose converter is trusted -- the parent of the change under test --
and never on the change itself: check that commit out into a worktree, copy tests/test_cpu_convert_pins.py and this file into it, and run there,
from the worktree's root:

    python tests/golden/make_convert_golden.py [--commit SHA]

The package imported is the one beside this file's tests/ directory.  The JSON states the recording commit: `git rev-parse HEAD` of that tree,
or --commit where the tree is not a git checkout."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path[:0] = [ROOT, TESTS]
import _pkg  # noqa: E402
import test_cpu_convert_pins as T  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--commit", default=None)
a = ap.parse_args()
commit = a.commit or subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
pkg = _pkg.load()
out = {"commit": commit, "sha1": {}}
with tempfile.TemporaryDirectory() as tmp:
    for name in T.CASES:
        out["sha1"][name] = T.sha1_of(pkg, name, os.path.join(tmp, "out.gguf"))
with open(T.GOLDEN, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(f"wrote {T.GOLDEN}: {len(out['sha1'])} cases, recorded on {commit}")
