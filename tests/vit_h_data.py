"""Helpers of tests/test_gpu_vit_h.py and tests/test_cpu_vit_h.py: build tests/cpp/vit_h_driver.cpp, write its raw input arrays, run a script of steps
in a fresh child process and read back what every step returned.

The driver runs vit.h's entry points (csrc/vit_api.cpp) on ONE vit_model / vit_state pair; the tests compare its outputs bit for bit with the C ABI
called through `binding` in the test process.  A child that ends by a signal or at its time limit sets FAULT: every later run() in the session skips."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, "vit.cpp_amd")
SOURCE = os.path.join(ROOT, "tests", "cpp", "vit_h_driver.cpp")
FAULT = []                     # the reason, once a driver run ended by a signal or at its time limit: nothing more is started after a fault
PAIR = np.dtype([("v", "<f4"), ("i", "<i4")])


def build_driver(out_dir):
    """g++ the driver against vit.cpp_amd/vit.h and libvitx.so (the command line of the examples' test).  Returns the executable's path."""
    exe = os.path.join(str(out_dir), "vit_h_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", SOURCE, "-I" + PKGDIR, "-L" + PKGDIR, "-lvitx", "-L/opt/rocm/lib",
                        "-Wl,-rpath," + PKGDIR, "-Wl,-rpath,/opt/rocm/lib", "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return exe


def fhex(x):
    """A float32 as the C hex float that strtof reads back to the same bits."""
    return float(np.float32(x)).hex()


def step(op, **kv):
    """One script line.  Lists become a,b,c; None and empty lists become '-'; floats must already be strings (fhex)."""
    parts = [op]
    for k, v in kv.items():
        if v is None or (isinstance(v, (list, tuple)) and not len(v)):
            v = "-"
        elif isinstance(v, (list, tuple)):
            v = ",".join(str(int(e)) for e in v)
        elif isinstance(v, (bool, np.bool_)):
            v = int(v)
        assert not isinstance(v, float), (k, "pass floats through fhex()")
        parts.append(f"{k}={v}")
    return " ".join(parts)


class Data:
    """The driver's DATA_DIR: the images (a list of [h, w, 3] f32 arrays, any shapes) and named arrays."""

    def __init__(self, path, images):
        self.path = str(path)
        os.makedirs(self.path, exist_ok=True)
        imgs = [np.ascontiguousarray(a, "<f4") for a in images]
        assert all(a.ndim == 3 and a.shape[2] == 3 for a in imgs)
        self.put("pixels", np.concatenate([a.ravel() for a in imgs]), "<f4")
        self.put("hw", np.asarray([a.shape[:2] for a in imgs]), "<i4")

    def put(self, name, array, dtype):
        np.ascontiguousarray(array, dtype).tofile(os.path.join(self.path, name + ".bin"))
        return name


class Step:
    def __init__(self, out_dir, index, status):
        self.out_dir, self.index, self.status = out_dir, index, status
        self.op = status["op"]
        self.rc = int(self.arr("rc", "<i4")[0])
        assert self.rc == status["rc"]

    def arr(self, name, dtype):
        return np.fromfile(os.path.join(self.out_dir, f"out_{self.index}_{name}.bin"), dtype)

    def rows(self, name, dtype, counts="counts"):
        """The per-image pieces of a flat output, split by its counts file."""
        c = self.arr(counts, "<i4")
        flat = self.arr(name, dtype)
        assert flat.size == int(c.sum()), (name, flat.size, c)
        return np.split(flat, np.cumsum(c)[:-1]) if c.size else []

    def heads_off(self):
        s = self.status
        return s["dense_classes"] == 0 and s["depth_bins"] == 0 and s["zeroshot_classes"] == 0 and s["nn_k"] == 0 and s["feat_floats"] == 0


def run(exe, model_path, data, lines, out_dir):
    """Run the script `lines` in a fresh child process.  Returns (steps, stderr).  A non-zero exit fails the test with the child's stderr; a child killed
    by a signal or by the time limit sets FAULT first."""
    if FAULT:
        pytest.skip(f"an earlier driver run faulted: {FAULT[0]}")
    out_dir = str(out_dir)
    os.makedirs(out_dir, exist_ok=True)
    script = os.path.join(out_dir, "script.txt")
    with open(script, "w") as f:
        f.write("\n".join(lines) + "\n")
    try:
        r = subprocess.run([exe, model_path, data.path, script, out_dir], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        FAULT.append(f"the driver ran into its time limit on {lines}")
        pytest.fail(f"{FAULT[0]}\n{str(e.stderr or '')[-4000:]}")
    if r.returncode < 0:
        FAULT.append(f"the driver ended by signal {-r.returncode} on {lines}")
        pytest.fail(f"{FAULT[0]}\n{r.stderr[-4000:]}")
    assert r.returncode == 0, f"exit status {r.returncode}\n{r.stderr[-4000:]}"
    steps = []
    for ln in r.stdout.splitlines():
        if not ln.startswith("STEP "):
            continue
        tok = ln.split()
        status = {"op": tok[2]}
        status.update({k: int(v) for k, v in (t.split("=") for t in tok[3:])})
        assert int(tok[1]) == len(steps)
        steps.append(Step(out_dir, len(steps), status))
    assert len(steps) == len(lines), (len(steps), len(lines), r.stdout[-2000:], r.stderr[-2000:])
    return steps, r.stderr


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    """Equal shapes and equal bits."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool((bits(a) == bits(b)).all())


def check_sorted_pairs(pairs, probs_row):
    """`pairs` (PAIR records) is a permutation of (probability, class) of probs_row with non-increasing probabilities; the order among ties is free."""
    p = np.asarray(probs_row, np.float32)
    assert pairs.size == p.size
    assert sorted(pairs["i"].tolist()) == list(range(p.size)), "the classes are not a permutation"
    assert (bits(pairs["v"]) == bits(p[pairs["i"]])).all(), "a pair's probability is not its class's"
    assert (pairs["v"][:-1] >= pairs["v"][1:]).all(), "the probabilities are not in non-increasing order"
