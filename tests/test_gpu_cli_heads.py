"""vit_cli.py's gallery, dense-head and depth-head modes on a fixed-shape context, run as a subprocess on tests/golden/assets and compared bit for bit
with the C ABI called through `binding` here on the same decoded and preprocessed pixels."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import dense_data as DD
import depth_data as PD
import zs_data as ZD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "tests", "golden", "assets")
GEOMETRIES = {"square": [], "shape": ["--img-shape", "28x70"], "fit": ["--img-fit", "28"]}
DTYPES = {"f16": 0, "bf16": 1}


def _cli(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "vit_cli.py"), *argv], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    return r.stdout.split("\n"), r.stderr


def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def _square(binding, model, img):
    """The CLI's default preprocessing at the file's size: the file's own where it carries one, the reference's bicubic stretch otherwise."""
    if model.has_preproc:
        return binding.preprocess_ex(img, model.preproc())
    return binding.preprocess(img, model.img_size, binding.BICUBIC)


def _geometry(binding, model, img, geometry):
    """(preprocessed image [h, w, 3], the Context keywords) of one of GEOMETRIES for the decoded image."""
    if geometry == "square":
        return _square(binding, model, img), {}
    if geometry == "shape":
        h, w = 28, 70
    else:
        w, h = binding.rect_shape(img.shape[1], img.shape[0], model.hparams.patch_size, 28)
    pp = model.preproc()
    if pp.filter not in (binding.PP_PIL_BILINEAR, binding.PP_PIL_BICUBIC):
        pp.filter = binding.PP_PIL_BICUBIC
    return binding.preprocess_rect(img, pp, w, h), dict(img_shape=(h, w), pos_interp=binding.POS_BICUBIC)


@pytest.fixture(scope="module")
def backbone(pkg):
    return pkg.synth.cached_synthetic("vit_micro_patch14_56", ftype=1, head_scale=4.0, registers=4, head_pool=0)


# ------------------------------------------------------------------------------------------------ --dense-head, --depth-head
@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_dense_head_writes_the_label_map_of_dense_read(pkg, binding, torch_gpu, backbone, tmp_path, geometry):
    """The PGM's header is `img_w img_h`, its bytes are dense_read's labels, the printed shares are the map's."""
    model = binding.Model(backbone)
    K, names = 5, ["sky", "road", "tree", "grass", "water"]
    _, W, b = DD.exact_head(1, K, 2 * model.hparams.hidden_size, seed=8)
    head, out, asset = str(tmp_path / "head.npz"), str(tmp_path / "map.pgm"), os.path.join(ASSETS, "tench.jpg")
    pkg.convert.write_dense_head(head, {"weight": W, "bias": b, "layers": [0, 1], "names": names})
    printed, err = _cli("-m", backbone, "--dtype", "bf16", "-i", asset, "--dense-head", head, "--dense-out", out, "-k", "3", *GEOMETRIES[geometry])
    img1, kw = _geometry(binding, model, _decode(asset), geometry)
    h, w = img1.shape[:2]
    assert (geometry == "square") == (h == w) and (geometry != "shape" or (h, w) == (28, 70))
    ctx = binding.Context(model, device=0, max_batch=1, dtype=DTYPES["bf16"], **kw)
    ctx.dense_set(W, b, [0, 1])
    ctx.forward(img1[None])
    lab = ctx.dense_read(1)[0][0]
    ctx.close(); model.close()
    assert lab.shape == (h, w) and len(np.unique(lab)) > 1
    blob = open(out, "rb").read()
    hdr = f"P5\n{w} {h}\n255\n".encode()
    assert blob.startswith(hdr), blob[:20]
    assert blob[len(hdr):] == lab.tobytes()
    assert f"wrote the {w} x {h} label map" in err
    share = np.bincount(lab.reshape(-1), minlength=K) / lab.size
    want = [f" > {names[k]} : {share[k]:.2f}" for k in np.argsort(-share, kind="stable")[:3] if share[k] > 0]
    assert printed == want + [""], printed


@pytest.mark.parametrize("geometry", list(GEOMETRIES))
def test_depth_head_writes_the_depth_map_of_depth_read(pkg, binding, torch_gpu, backbone, tmp_path, geometry):
    """The .npy array is depth_read's, bit for bit, of shape [img_h, img_w]; the printed line summarises it."""
    model = binding.Model(backbone)
    K = 8
    _, _, wp, wc, bias = PD.exact_head(1, 1, K, model.hparams.hidden_size, seed=9)
    bins = PD.bins_ud(K)
    head, out, asset = str(tmp_path / "head.npz"), str(tmp_path / "d.npy"), os.path.join(ASSETS, "tench.jpg")
    pkg.convert.write_depth_head(head, {"wp": wp, "wc": wc, "bias": bias, "bins": bins, "layers": [1], "upsample": 2, "min_depth": 1.5, "max_depth": 8.0, "norm": True})
    printed, err = _cli("-m", backbone, "-i", asset, "--depth-head", head, "--depth-out", out, *GEOMETRIES[geometry])
    img1, kw = _geometry(binding, model, _decode(asset), geometry)
    h, w = img1.shape[:2]
    assert (geometry == "square") == (h == w)
    ctx = binding.Context(model, device=0, max_batch=1, dtype=DTYPES["f16"], **kw)
    ctx.depth_set(wp, wc, bias, bins, [1], 2, 1.5, 8.0, norm=True)
    ctx.forward(img1[None])
    dm = ctx.depth_read(1)[0][0]
    ctx.close(); model.close()
    got = np.load(out)
    assert got.dtype == np.float32 and got.shape == (h, w) == dm.shape
    assert (got.view(np.uint32) == dm.view(np.uint32)).all()
    assert len(np.unique(dm)) > 1
    assert f"wrote the {w} x {h} depth map" in err
    assert printed == [f" > depth : min {float(dm.min()):.3f} median {float(np.median(dm)):.3f} max {float(dm.max()):.3f}", ""], printed


# ------------------------------------------------------------------------------------------------ --gallery-build, --gallery
FOLDERS = {"ant": ["apple.jpg", "cheetah.jpg"], "bee": ["giraffe.jpg", "kiwi.jpg", "tench.jpg"], "cat": ["image.png", "polars.jpeg"]}


def _gallery_dir(tmp_path):
    root = tmp_path / "gallery"
    for d, fs in FOLDERS.items():
        os.makedirs(root / d)
        for f in fs:
            shutil.copy(os.path.join(ASSETS, f), root / d / f)
    paths = [str(root / d / f) for d in sorted(FOLDERS) for f in sorted(FOLDERS[d])]
    labels = [li for li, d in enumerate(sorted(FOLDERS)) for _ in FOLDERS[d]]
    return str(root), paths, labels


def _rows(binding, ctx, paths, source, batch):
    """binding.nn_gallery on the preprocessed files, in the chunks of `batch`."""
    imgs = np.stack([_square(binding, ctx.model, _decode(p)) for p in paths])
    return np.concatenate([binding.nn_gallery(ctx, imgs[lo:lo + batch], source) for lo in range(0, len(paths), batch)])


@pytest.mark.parametrize("source", ["embed", "logits"])
def test_gallery_build_writes_the_rows_of_nn_gallery(pkg, binding, torch_gpu, tmp_path, source):
    """Seven files in three label folders with --batch 3 (three chunks): embeds are nn_gallery's rows of the chosen source bit for bit, labels follow the
    sorted folder names, paths the sorted files."""
    src = ZD.model_file(pkg, "clip")
    root, paths, labels = _gallery_dir(tmp_path)
    out = str(tmp_path / "g.npz")
    _, err = _cli("-m", src, "--gallery-build", root, "--gallery-out", out, "--nn-source", source, "--batch", "3")
    model = binding.Model(src)
    ctx = binding.Context(model, device=0, max_batch=3, dtype=DTYPES["f16"])
    code = binding.NN_EMBED if source == "embed" else binding.NN_LOGITS
    want = _rows(binding, ctx, paths, code, 3)
    other = _rows(binding, ctx, paths, binding.NN_LOGITS if source == "embed" else binding.NN_EMBED, 3)
    ctx.close(); model.close()
    assert want.shape[0] == 7 and want.shape[1] != other.shape[1], "the two sources must differ for the test to see --nn-source ignored"
    with np.load(out) as z:
        assert sorted(z.files) == ["embeds", "label_names", "labels", "paths", "source"]
        assert z["embeds"].dtype == np.float32 and z["embeds"].shape == want.shape
        assert (z["embeds"].view(np.uint32) == want.view(np.uint32)).all()
        assert z["labels"].dtype == np.int32 and z["labels"].tolist() == labels
        assert z["label_names"].tolist() == sorted(FOLDERS)
        assert z["paths"].tolist() == paths
        assert int(z["source"]) == code
    assert f"wrote 7 {source} rows of 3 labels" in err


@pytest.mark.parametrize("labelled", [True, False], ids=["labels", "no-labels"])
def test_gallery_query_prints_the_neighbours_and_the_vote_of_nn_read(pkg, binding, torch_gpu, tmp_path, labelled):
    """--gallery g.npz -i asset -k 3: the ' ~ path : score' lines are nn_read's neighbours, the ' > label : weight' lines vitx_topk's order over its vote;
    a gallery saved without labels prints no vote."""
    src = ZD.model_file(pkg, "clip")
    root, paths, labels = _gallery_dir(tmp_path)
    model = binding.Model(src)
    ctx = binding.Context(model, device=0, max_batch=1, dtype=DTYPES["f16"])
    embeds = _rows(binding, ctx, paths, binding.NN_LOGITS, 1)
    gal = str(tmp_path / "g.npz")
    arrays = dict(embeds=embeds, paths=np.asarray(paths), source=np.int32(binding.NN_LOGITS))
    if labelled:
        arrays.update(labels=np.asarray(labels, np.int32), label_names=np.asarray(sorted(FOLDERS)))
    np.savez(gal, **arrays)
    asset = os.path.join(ASSETS, "magpie.jpeg")                     # not in the gallery
    printed, _ = _cli("-m", src, "-i", asset, "--gallery", gal, "-k", "3", "--nn-temperature", "0.5")
    ctx.nn_set(embeds, 3, binding.NN_LOGITS, labels if labelled else None, 3 if labelled else 0, 0.5)
    ctx.forward(_square(binding, model, _decode(asset))[None])
    idx, score, vote = ctx.nn_read(1)
    want = [f" ~ {paths[g]} : {s:.4f}" for g, s in zip(idx[0], score[0])]
    assert len(set(idx[0].tolist())) == 3
    if labelled:
        want += [f" > {sorted(FOLDERS)[i]} : {p:.2f}" for i, p in zip(*binding.topk(vote[0], 3))]
    else:
        assert vote is None
    ctx.close(); model.close()
    assert printed == want + [""], printed
