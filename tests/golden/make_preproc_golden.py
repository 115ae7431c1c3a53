"""Records tests/golden/preproc_pil.json: the sha1 of Pillow's u8 result for every case of tests/preproc_data.py -- Image.resize((W, H)) with
BILINEAR and BICUBIC on each pattern of each geometry, then the centre crop of side min(W, H) the case takes.  Run from the repo root:

    python tests/golden/make_preproc_golden.py

The committed record was made with Pillow 12.2.0 (the file states the version that wrote it).  The tests compare the library with this record
and with the installed Pillow: a Pillow whose resize arithmetic changed shows up as a disagreement between the two."""
import json
import os
import sys

import PIL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import preproc_data as PD  # noqa: E402

out = {"pillow": PIL.__version__, "sha1": {}}
for g in PD.GEOMETRIES:
    for pattern in PD.PATTERNS:
        a = PD.image(pattern, g[0], g[1])
        for fname, f in PD.FILTERS.items():
            window, _ = PD.pillow_window(a, PD.geometry_spec(g, f))
            out["sha1"][PD.golden_key(g, pattern, fname)] = PD.sha1(window)
with open(PD.GOLDEN, "w") as fh:
    json.dump(out, fh, indent=1, sort_keys=True)
    fh.write("\n")
print(f"wrote {PD.GOLDEN}: {len(out['sha1'])} cases, Pillow {PIL.__version__}")
