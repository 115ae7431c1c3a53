"""Records what the reference-compiled code (oracle/_ref, built by oracle/build_ref.sh where the reference sources exist) returns on
the inputs of tests/test_cpu_ref_pin.py and tests/test_cpu_vitstr.py, so that those pins hold on machines without the reference.
Run from the repo root after __graft_entry__.build():

    python tests/golden/make_ref_golden.py

  * ref_vit.json     vit_image_preprocess of the bundled images and edge shapes (sha1 of the -ffp-contract=off build's f32 output,
                     plus the values the FMA-contracting build returns differently), the rejected "nearest" mode, the prediction
                     sort, the quantize tensor selection, the hparams defaults
  * ref_vitstr.json  the ViTSTR grey preprocess (sha1 of the strict build's output, largest distance of the FMA-contracting build's)
                     and the greedy decode (text, score)

Every test that reads these also compares them with oracle/_ref where that library exists, so a stale recording fails there.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
import _pkg  # noqa: E402

pkg = _pkg.load()
from vitcpp_amd import binding  # noqa: E402
import test_cpu_ref_pin as P  # noqa: E402
import test_cpu_vitstr as V  # noqa: E402


def _need(L, build):
    if L is None:
        raise SystemExit(f"oracle/_ref/{build} is missing: run __graft_entry__.build() where the reference sources exist")
    return L


def vit():
    Lf, Ls = (_need(P._ref(b), b) for b in P.BUILDS)
    rec = {"preprocess": {}, "edge": {}}
    for a in P.ASSETS:
        img = P._decode(a)
        for mode in ("bicubic", "bilinear"):
            for S in (224, 384):
                rec["preprocess"][f"{a}|{mode}|{S}"] = P.preprocess_record(Ls, Lf, img, S, mode)
    for shape in P.EDGE_SHAPES:
        img = P.edge_image(shape)
        for mode in ("bicubic", "bilinear"):
            for S in (32, 224):
                rec["edge"][f"{shape[0]}x{shape[1]}|{mode}|{S}"] = P.preprocess_record(Ls, None, img, S, mode)
    rec["nearest_rc"] = P._ref_preprocess(Lf, P._decode(P.ASSETS[0]), 224, "nearest")[0]
    rec["sort"] = [P.sort_record(Ls, p) for p in P.sort_inputs()]
    src = pkg.synth.cached_synthetic("vit_micro_patch16_64", head_scale=4.0)
    names = sorted(t[0] for t in binding.Model(src).tensors())
    rec["quantize_file"] = P.quantize_record(Ls, [(n, P.n_dims_in_file(n)) for n in names])
    rec["quantize_probes"] = P.quantize_record(Ls, P.QUANT_PROBES)
    rec["hparams"] = P.hparams_record(Ls)
    return rec


def vitstr():
    strict, fma = (_need(V._ref(b), b) for b in ("libvitstr_ref_strict.so", "libvitstr_ref_fma.so"))
    rec = {"preprocess": {f"{i}|{S}": V.preprocess_record(strict, fma, img, S) for i, img in enumerate(V.images(binding)) for S in (224, 64)}}
    rec["decode"] = [V.decode_record(strict, pkg.synth.VITSTR_LABELS, p) for p in V.decode_cases()]
    return rec


def main():
    for name, rec in (("ref_vit.json", vit()), ("ref_vitstr.json", vitstr())):
        with open(os.path.join(HERE, name), "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
    print("reference recordings written to", HERE)


if __name__ == "__main__":
    main()
