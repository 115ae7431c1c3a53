"""The segment-table layout of a packed context (vit.cpp_amd/csrc/packed_context.h PackLayout): tests/cpp/pack_layout_main.cpp, a stand-alone program
with no device call, prints every accessor and ints() for cap in {1, 3, 16} and each of the 16 subsets of the parts; the output equals
tests/golden/pack_layout.json, which the same program printed from the hand-written chain of conditional offsets the layout was before it was computed
from one table list.  ints() sizes the table buffer, so vitx_pack_scratch_bytes follows it for every sequence of sets and un-sets."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "pack_layout_main.cpp")
GOLDEN = os.path.join(ROOT, "tests", "golden", "pack_layout.json")
ACCESSORS = ("row0", "qb0", "toff", "tile0", "seg", "ftile0", "otile0", "dseg", "ptile0", "pseg", "rblk0", "sq0", "ints")


def test_every_accessor_of_every_subset_of_parts_is_where_the_hand_written_chain_put_it(tmp_path):
    exe = str(tmp_path / "pack_layout_main")
    r = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-I" + os.path.join(ROOT, "vit.cpp_amd"),
                        "-I" + os.path.join(ROOT, "include"), SOURCE, "-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-4000:]
    got = json.loads(r.stdout)
    with open(GOLDEN) as f:
        want = json.load(f)
    assert [(e["cap"], e["parts"]) for e in want] == [(cap, parts) for cap in (1, 3, 16) for parts in range(16)]
    assert all(set(e) == {"cap", "parts", *ACCESSORS} for e in want)
    for g, w in zip(got, want):
        assert g == w, (w["cap"], w["parts"], {k: (g.get(k), w[k]) for k in ACCESSORS if g.get(k) != w[k]})
    assert len(got) == len(want)
