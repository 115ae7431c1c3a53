"""Command-line front end equivalent to the reference's `vit` binary (/root/reference/main.cpp:25-112) and its
directory-walk accuracy harness:

    python vit_cli.py -m model.gguf -i image.jpg [-k 5] [--dtype f16|bf16|mxfp8] [--interp bicubic|bilinear]
    python vit_cli.py -m model.gguf --dir imagenet_val/ [--batch 256]       # top-1 over <dir>/<label>/*.jpg
    python vit_cli.py -m model.gguf -i image.jpg --attn-map map.pgm [--attn-kind rollout|last]   # + where the model looked (P5 picture)
    python vit_cli.py -m model.gguf (-i image.jpg | --dir DIR) --embed out.npy [--embed-kind cls|mean|tokens] [--embed-l2]   # + the embeddings
    python vit_cli.py -m model.gguf ... --img-size 384 [--pos-interp bicubic|bicubic-aa]   # run at another input size than the file's
    python vit_cli.py -m model.gguf ... --img-shape 224x448 | --img-fit 224   # a rectangular context: HxW, or the aspect-preserving shape of the input image
    python vit_cli.py -m model.gguf -i a.jpg,b.jpg,c.jpg --pack --img-fit 224   # several images, each at its own aspect-preserving shape, in one packed forward
    python vit_cli.py -m model.gguf -i a.jpg,b.jpg,c.jpg --pack --img-fit 224 --attn-map PREFIX [--attn-kind rollout|last]   # + PREFIX.<i>.pgm per image, on its own grid
    python vit_cli.py -m model.gguf -i a.jpg,b.jpg,c.jpg --pack --img-fit 224 --pack-u8   # the same, resized on the device from the u8 originals in one launch
    python vit_cli.py -m model.gguf ... [--preprocess model|reference]   # the file's own preprocessing (default) or the reference's for any file
    python vit_cli.py -m clip.gguf -i image.jpg -k 5 --zero-shot bank.npz   # zero-shot classes of a CLIP / SigLIP file (bank: convert.py --zero-shot-out)
    python vit_cli.py -m clip.gguf -i image.jpg --text-model text.gguf --zero-shot-ids ids.npy [--zero-shot-labels labels.txt]   # the bank made by the engine, same run
    python vit_cli.py --text-model text.gguf --zero-shot-ids ids.npy --text-embed out.npy   # the text embeddings of tokenised prompts (no image, no -m)
    python vit_cli.py -m model.gguf --gallery-build DIR --gallery-out g.npz [--nn-source embed|logits]   # embed DIR/<label>/* into a gallery
    python vit_cli.py -m model.gguf -i image.jpg --gallery g.npz -k 5 [--nn-temperature 0.07]   # the k nearest gallery images and the k-NN vote of their labels
    python vit_cli.py -m backbone.gguf -i image.jpg --dense-head head.npz --dense-out labels.pgm [--img-shape HxW | --img-fit SHORT]   # a label per pixel (P5 picture of class bytes)
    python vit_cli.py -m backbone.gguf -i a.jpg,b.jpg --pack --img-fit SHORT --dense-head head.npz --dense-out PREFIX   # PREFIX.<i>.pgm per image, at each ORIGINAL's size
    python vit_cli.py -m backbone.gguf -i image.jpg --depth-head head.npz --depth-out depth.npy [--img-shape HxW | --img-fit SHORT]   # a depth per pixel (float32 .npy)
    python vit_cli.py -m backbone.gguf -i a.jpg,b.jpg --pack --img-fit SHORT --depth-head head.npz --depth-out PREFIX   # PREFIX.<i>.npy per image, at each ORIGINAL's size

--preprocess model follows the file's `preproc` tensor (include/vitx.h "each model's own preprocessing": what convert.py reads from a
HuggingFace preprocessor_config.json -- CLIP: Pillow-bicubic shortest edge 224, centre crop 224, CLIP's mean / std; DINOv2: shortest edge 256,
crop 224; HuggingFace ViT: Pillow-bilinear stretch, mean = std = 0.5); with --img-size it is rescaled by vitx_preproc_at_size.  A file without
the tensor -- every file of the reference's converter -- is preprocessed by the reference's vit_image_preprocess with --interp, as always.

Same flags as vit_params_parse (vit.cpp:955-1002: -m -i -t -k -s -e; -t, -s and -e are accepted and ignored exactly
as the reference's forward ignores seed and eps), same stdout lines (" > label : 0.xx", vit.cpp:1062-1067) and the
same stderr timing block.  Decoding is PIL here (the reference uses stb_image inside the absent ggml tree); everything
after the decoded u8 RGB array -- preprocess, forward, top-k -- runs through the C ABI of libvitx.so on the GPU.
"""
from __future__ import annotations

import argparse
import os
import sys
import time
from typing import List

import numpy as np


def _decode(path: str) -> np.ndarray:
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def attn_pgm(grid: np.ndarray, img_size) -> bytes:
    """[gh, gw] patch map -> binary PGM (P5) of img_w x img_h bytes (img_size: a side, or (img_h, img_w)): nearest-neighbour upsampling, scaled to
    0..255 (the maximum is 255)."""
    gh, gw = grid.shape
    ih, iw = (int(img_size), int(img_size)) if np.isscalar(img_size) else (int(img_size[0]), int(img_size[1]))
    m = np.asarray(grid, np.float64)
    lo, hi = float(m.min()), float(m.max())
    u8 = np.zeros_like(m, np.uint8) if hi <= lo else np.rint((m - lo) / (hi - lo) * 255.0).astype(np.uint8)
    iy, ix = np.arange(ih) * gh // ih, np.arange(iw) * gw // iw      # source patch of every output pixel
    return f"P5\n{iw} {ih}\n255\n".encode() + u8[iy][:, ix].tobytes()


def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="vit", description="ViT inference on MI355X (drop-in for staghado/vit.cpp's CLI)")
    ap.add_argument("-m", "--model", default="../ggml-model-f16.gguf")
    ap.add_argument("-i", "--inp", default="../assets/tench.jpg")
    ap.add_argument("-t", "--threads", type=int, default=4, help="accepted for compatibility; the GPU path has no thread count")
    ap.add_argument("-k", "--topk", type=int, default=5)
    ap.add_argument("-s", "--seed", type=int, default=-1, help="accepted for compatibility (unused by the forward, as in the reference)")
    ap.add_argument("-e", "--epsilon", type=float, default=1e-6, help="accepted for compatibility (the reference's forward uses hparams.eps = 1e-6)")
    ap.add_argument("--dtype", default="f16", choices=["f16", "bf16", "mxfp8"],
                    help="MFMA operand type; f16 reproduces the reference's rounding points; mxfp8 is EXPERIMENTAL (qkv, fc1, fc2 on block-scaled e4m3, "
                         "the rest bf16): slower than bf16 on MI355X and less accurate (DESIGN.md section 4)")
    ap.add_argument("--interp", default="bicubic", choices=["bicubic", "bilinear"])
    ap.add_argument("--preprocess", default="model", choices=["model", "reference"],
                    help="model (default): the file's own preprocessing where it carries one (resize, centre crop, mean / std as the model's publisher defines "
                         "them), the reference's otherwise; reference: the reference's stretch to img_size^2 with --interp and ImageNet mean / std for any file")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--dir", default=None, help="accuracy harness: walk DIR/<label>/* and report top-1 against the directory name")
    ap.add_argument("--batch", type=int, default=256, help="images per forward in --dir mode")
    ap.add_argument("--attn-map", default=None, metavar="PATH", help="with -i: write the image's attention map as a binary PGM (P5), img_size x img_size; with --pack: a prefix, "
                                                                                "PATH.<i>.pgm per image at its own packed shape")
    ap.add_argument("--attn-kind", default="rollout", choices=["rollout", "last"],
                    help="rollout: attention rollout through all layers; last: head mean of the last layer's class-token map")
    ap.add_argument("--embed", default=None, metavar="OUT.npy",
                    help="also write the last layer's final-norm features as an .npy array, one row per image (with --dir: in walk order, and the "
                         "file names to OUT.npy.txt); the classification output is unchanged")
    ap.add_argument("--embed-kind", default="cls", choices=["cls", "mean", "tokens"],
                    help="cls: the class-token embedding [D]; mean: the mean of the patch features [D]; tokens: the patch features [patches, D] (the class token and any register tokens excluded)")
    ap.add_argument("--embed-l2", action="store_true", help="divide the cls / mean embedding by its Euclidean norm")
    ap.add_argument("--img-size", type=int, default=0, metavar="N",
                    help="run at N x N instead of the file's img_size (a multiple of the patch size): the position table is resampled to the new grid; "
                         "the preprocess, the --attn-map picture and the --embed shapes follow")
    ap.add_argument("--img-shape", default=None, metavar="HxW",
                    help="run on H x W images (both multiples of the patch size) in a rectangular context: the image is STRETCHED to that shape by the "
                         "file's own filter, mean and std, without a crop (a file without a `preproc` tensor, or one with the reference's filter: Pillow "
                         "bicubic with the file's default mean / std); --attn-map then writes a W x H picture, --embed-kind tokens (H/P)(W/P) rows")
    ap.add_argument("--pack-u8", action="store_true",
                    help="with --pack: feed the decoded u8 originals and let ONE device launch stretch each to its own shape (vitx_pack_forward_u8), instead of "
                         "resizing on the host; the printed lines are the same")
    ap.add_argument("--img-fit", type=int, default=0, metavar="SHORT",
                    help="with -i: like --img-shape, with the shape taken from the input image: its short side becomes SHORT (a multiple of the patch size), "
                         "the long side the largest multiple of the patch size that keeps the aspect (vitx_rect_shape; 500 x 375 at 224, patch 16: 288 x 224)")
    ap.add_argument("--pack", action="store_true",
                    help="with --img-fit SHORT and -i A.jpg,B.jpg,...: every image at its own aspect-preserving shape in ONE forward of a packed context "
                         "(include/vitx.h \"packed batches\"); prints each image's ' > label : 0.xx' lines, image after image")
    ap.add_argument("--pos-interp", default="bicubic", choices=["bicubic", "bicubic-aa"],
                    help="with --img-size, --img-shape or --img-fit: bicubic = F.interpolate(mode='bicubic') (HuggingFace interpolate_pos_encoding, DINO); "
                         "bicubic-aa = the same with antialias=True (timm resample_abs_pos_embed)")
    ap.add_argument("--zero-shot", default=None, metavar="BANK.npz",
                    help="with -i, a CLIP or SigLIP file: classify against the bank of text embeddings in BANK.npz (convert.py --zero-shot-out) instead of the "
                         "file's own head; the ' > label : 0.xx' lines are the bank's labels and the zero-shot probabilities (softmax for CLIP, sigmoid for SigLIP)")
    ap.add_argument("--text-model", default=None, metavar="TEXT.gguf",
                    help="the checkpoint's text-tower file (convert.py --text-out): with --zero-shot-ids the zero-shot bank is made by the engine in this run")
    ap.add_argument("--zero-shot-ids", default=None, metavar="IDS.npy",
                    help="with --text-model: token ids, an integer array [prompts][tokens], one class per prompt (there is no tokenizer in the engine)")
    ap.add_argument("--zero-shot-labels", default=None, metavar="LABELS.txt", help="with --zero-shot-ids: one class name per line (default: class_<k>)")
    ap.add_argument("--text-embed", default=None, metavar="OUT.npy", help="with --text-model and --zero-shot-ids: write the prompts' text embeddings [prompts][E] and stop "
                                                                          "unless -m names an image model to classify with")
    ap.add_argument("--gallery-build", default=None, metavar="DIR",
                    help="embed every image under DIR/<label>/* and write the gallery to --gallery-out: unit rows `embeds`, `labels`, `label_names`, `paths` (and `source`)")
    ap.add_argument("--gallery-out", default=None, metavar="G.npz", help="with --gallery-build: the file to write")
    ap.add_argument("--nn-source", default="embed", choices=["embed", "logits"],
                    help="with --gallery-build: what a gallery row is: embed = the head's operand row (any backbone, also one converted without a head), "
                         "logits = the logits row (image_embeds of a CLIP file)")
    ap.add_argument("--gallery", default=None, metavar="G.npz",
                    help="with -i: print the -k nearest gallery images with their scores and, when the gallery has labels, the ' > label : 0.xx' lines of the "
                         "temperature-weighted k-NN vote (vitx_nn_set) instead of the file's own head")
    ap.add_argument("--nn-temperature", type=float, default=0.07, help="with --gallery: the vote's temperature (DINO: 0.07)")
    ap.add_argument("--dense-head", default=None, metavar="HEAD.npz",
                    help="with -i: a linear head over the patch tokens (convert.py --dense-head-out: weight, bias, layers, names): the label of every pixel of the "
                         "preprocessed image goes to --dense-out, the share of every class is printed as ' > name : 0.xx'")
    ap.add_argument("--dense-out", default=None, metavar="PATH", help="with --dense-head: the label map as a binary PGM (P5) of class bytes, img_w x img_h")
    ap.add_argument("--depth-head", default=None, metavar="HEAD.npz",
                    help="with -i: a binned linear depth head (convert.py --depth-head-out): the depth of every pixel of the preprocessed image goes to --depth-out")
    ap.add_argument("--depth-out", default=None, metavar="PATH.npy", help="with --depth-head: the depth map as a float32 .npy array [img_h, img_w]")
    return ap


def gallery_build(binding, a, model, ctx, preprocess):
    """--gallery-build: DIR/<label>/<image> -> G.npz.  The label of an image is its sub-directory's name."""
    names = [d for d in sorted(os.listdir(a.gallery_build)) if os.path.isdir(os.path.join(a.gallery_build, d))]
    paths, labels = [], []
    for li, d in enumerate(names):
        for f in sorted(os.listdir(os.path.join(a.gallery_build, d))):
            paths.append(os.path.join(a.gallery_build, d, f)); labels.append(li)
    if not paths:
        print(f"main: no <label>/<image> files under '{a.gallery_build}'", file=sys.stderr)
        return 1
    source = binding.NN_EMBED if a.nn_source == "embed" else binding.NN_LOGITS
    rows = []
    for lo in range(0, len(paths), ctx.max_batch):
        rows.append(binding.nn_gallery(ctx, np.stack([preprocess(_decode(f)) for f in paths[lo:lo + ctx.max_batch]]), source))
    np.savez(a.gallery_out, embeds=np.concatenate(rows), labels=np.asarray(labels, np.int32), label_names=np.asarray(names), paths=np.asarray(paths),
             source=np.int32(source))
    print(f"main: wrote {len(paths)} {a.nn_source} rows of {len(names)} labels to '{a.gallery_out}'", file=sys.stderr)
    return 0


def text_side(binding, a, dt):
    """--text-model: the embeddings and the bank of --zero-shot-ids made by the engine.  Returns the bank (load_bank's dict), or raises
    VitxError / OSError / ValueError."""
    ids = np.load(a.zero_shot_ids)
    tmodel = binding.Model(a.text_model)
    if tmodel.kind != binding.KIND_TEXT:
        raise ValueError(f"'{a.text_model}' is an image model, not a text-tower file")
    tctx = binding.TextContext(tmodel, max_prompts=max(1, min(int(np.shape(ids)[0]), 256)), dtype=dt, device=a.device)
    raw = tctx.embed(ids)                                                 # the tower runs once: the file and the bank are made of the same rows
    if a.text_embed:
        np.save(a.text_embed, raw)
        print(f"main: wrote {np.shape(ids)[0]} text embeddings to '{a.text_embed}'", file=sys.stderr)
    embeds, kind, scale, bias = binding.text_bank(tctx, ids, embeds=raw)
    tctx.close(); tmodel.close()
    labels = [f"class_{k}" for k in range(embeds.shape[0])]
    if a.zero_shot_labels:
        with open(a.zero_shot_labels) as f:
            labels = [l.rstrip("\n") for l in f if l.strip()]
        if len(labels) != embeds.shape[0]:
            raise ValueError(f"{len(labels)} labels in '{a.zero_shot_labels}' for {embeds.shape[0]} prompts")
    return dict(embeds=embeds.astype(np.float32), labels=labels, kind=kind, scale=scale, bias=bias)


def main(argv: List[str] | None = None) -> int:
    from . import binding
    ap = make_parser()
    a = ap.parse_args(argv)
    if a.zero_shot and a.dir is not None:
        ap.error("--zero-shot takes the single image of -i, not --dir")
    if (a.text_model is None) != (a.zero_shot_ids is None):
        ap.error("--text-model and --zero-shot-ids come together")
    if (a.zero_shot_labels or a.text_embed) and not a.text_model:
        ap.error("--zero-shot-labels and --text-embed need --text-model TEXT.gguf --zero-shot-ids IDS.npy")
    if a.text_model and a.zero_shot:
        ap.error("--zero-shot BANK.npz and --text-model are two sources of one bank: give one")
    if a.text_model and a.dir is not None:
        ap.error("--text-model takes the single image of -i, not --dir")
    if a.text_model and a.dtype == "mxfp8":
        ap.error("--text-model: a text context takes --dtype f16 or bf16")
    if a.attn_map and a.dir is not None:
        ap.error("--attn-map takes the single image of -i, not --dir")
    if a.embed is None and (a.embed_l2 or a.embed_kind != "cls"):
        ap.error("--embed-kind and --embed-l2 need --embed OUT.npy")
    if a.embed_l2 and a.embed_kind == "tokens":
        ap.error("--embed-l2 normalises the cls / mean embedding; token features are never normalised")
    if bool(a.gallery_build) != bool(a.gallery_out):
        ap.error("--gallery-build DIR and --gallery-out G.npz go together")
    if bool(a.dense_head) != bool(a.dense_out):
        ap.error("--dense-head HEAD.npz and --dense-out PATH go together")
    if a.dense_head and (a.dir is not None or a.gallery_build or a.gallery):
        ap.error("--dense-head labels the single image of -i (or, with --pack, each image of -i A.jpg,B.jpg,...)")
    if bool(a.depth_head) != bool(a.depth_out):
        ap.error("--depth-head HEAD.npz and --depth-out PATH.npy go together")
    if a.depth_head and (a.dir is not None or a.gallery_build or a.gallery or a.dense_head):
        ap.error("--depth-head measures the single image of -i (or, with --pack, each image of -i A.jpg,B.jpg,...), and not together with --dense-head")
    if a.gallery and (a.dir is not None or a.gallery_build):
        ap.error("--gallery searches for the single image of -i")
    if sum(bool(v) for v in (a.img_size, a.img_shape, a.img_fit)) > 1:
        ap.error("--img-size, --img-shape and --img-fit are three ways to say one thing: give one")
    if a.img_fit and a.dir is not None:
        ap.error("--img-fit takes its shape from the single image of -i, not --dir (use --img-shape HxW)")
    if a.img_fit and a.gallery_build:
        ap.error("--img-fit takes its shape from the single image of -i, not --gallery-build (use --img-shape HxW)")
    if a.pack_u8 and not a.pack:
        ap.error("--pack-u8 goes with --pack")
    if a.pack and (not a.img_fit or a.dir is not None or a.dtype == "mxfp8" or a.embed or a.zero_shot or a.text_model or a.gallery or a.gallery_build):
        ap.error("--pack takes --img-fit SHORT, the images of -i A.jpg,B.jpg,... and --dtype f16 or bf16; of the opt-in outputs a packed context has attention maps "
                 "(--attn-map PREFIX), the dense head (--dense-head HEAD.npz --dense-out PREFIX) and the depth head (--depth-head HEAD.npz --depth-out PREFIX) only")
    if (a.img_shape or a.img_fit) and a.preprocess == "reference":
        ap.error("--preprocess reference resizes to squares only: not with --img-shape / --img-fit")
    rect = None                                          # (img_h, img_w) of a rectangular context
    if a.img_shape:
        try:
            rect = tuple(int(v) for v in a.img_shape.lower().split("x"))
            assert len(rect) == 2
        except (ValueError, AssertionError):
            ap.error(f"--img-shape takes HxW, e.g. 224x448 (got '{a.img_shape}')")
    feat = dict(cls=a.embed_kind == "cls", mean=a.embed_kind == "mean", tokens=a.embed_kind == "tokens", l2=a.embed_l2)
    last = lambda ctx: ctx.feat_read()[model.hparams.num_hidden_layers - 1][a.embed_kind]

    t_main = time.perf_counter()
    print(f"main: seed = {a.seed if a.seed >= 0 else int(time.time())}", file=sys.stderr)
    text_bank = None
    if a.text_model:
        try:
            text_bank = text_side(binding, a, binding.F16 if a.dtype == "f16" else binding.BF16)
        except (binding.VitxError, OSError, ValueError) as e:
            print(f"main: the text tower of '{a.text_model}' failed: {e}", file=sys.stderr)
            return 1
        if a.text_embed and a.model == ap.get_default("model"):           # embeddings only: no image model was named
            return 0
    try:
        model = binding.Model(a.model)
    except binding.VitxError as e:
        print(f"main: failed to load model from '{a.model}': {e}", file=sys.stderr)
        return 1
    t_load = time.perf_counter() - t_main
    dt = {"f16": binding.F16, "bf16": binding.BF16, "mxfp8": binding.MXFP8}[a.dtype]
    interp = binding.BICUBIC if a.interp == "bicubic" else binding.BILINEAR
    if a.img_size < 0:
        print(f"main: --img-size {a.img_size} is not a positive multiple of the patch size {model.hparams.patch_size}", file=sys.stderr)
        return 1
    S = a.img_size or model.img_size                     # the context's size: preprocess, maps and features follow it
    if a.preprocess == "model" and model.has_preproc:
        pp = model.preproc()
        if S != model.img_size:
            try:
                pp = binding.preproc_at_size(pp, S)
            except binding.VitxError as e:
                print(f"main: the model's preprocessing has no form at --img-size {S}: {e}", file=sys.stderr)
                return 1
        preprocess = lambda img: binding.preprocess_ex(img, pp)
    else:
        preprocess = lambda img: binding.preprocess(img, S, interp)
    geometry = dict(img_size=a.img_size, pos_interp=binding.POS_BICUBIC_AA if a.pos_interp == "bicubic-aa" else binding.POS_BICUBIC) if a.img_size else {}
    if rect or a.img_fit:
        # a rectangular context: the whole image stretched to img_w x img_h by the file's PIL filter, mean and std (vitx_preprocess_rect); a file
        # without a description, or with the reference's filter, takes Pillow bicubic with its default mean / std
        pp_rect = model.preproc()
        if pp_rect.filter not in (binding.PP_PIL_BILINEAR, binding.PP_PIL_BICUBIC):
            pp_rect.filter = binding.PP_PIL_BICUBIC
        preprocess = lambda img: binding.preprocess_rect(img, pp_rect, rect[1], rect[0])
        geometry = dict(pos_interp=binding.POS_BICUBIC_AA if a.pos_interp == "bicubic-aa" else binding.POS_BICUBIC)

    bank = text_bank
    if a.zero_shot:
        from .convert import load_bank
        try:
            bank = load_bank(a.zero_shot)
        except (OSError, ValueError) as e:
            print(f"main: failed to load the zero-shot bank from '{a.zero_shot}': {e}", file=sys.stderr)
            return 1

    if a.gallery_build:
        n_files = sum(len(fs) for _, _, fs in os.walk(a.gallery_build))
        try:
            ctx = binding.Context(model, device=a.device, max_batch=max(1, min(a.batch, n_files)), dtype=dt, img_shape=rect, **geometry)
            return gallery_build(binding, a, model, ctx, preprocess)
        except (binding.VitxError, OSError, ValueError) as e:
            print(f"main: failed to build the gallery of '{a.gallery_build}': {e}", file=sys.stderr)
            return 1
    gallery = None
    if a.gallery:
        try:
            with np.load(a.gallery) as z:
                gallery = {k: z[k] for k in z.files}
        except (OSError, ValueError) as e:
            print(f"main: failed to load the gallery from '{a.gallery}': {e}", file=sys.stderr)
            return 1

    dense = None
    if a.dense_head:
        try:
            dense = binding.dense_head(a.dense_head)
        except (OSError, ValueError, KeyError) as e:
            print(f"main: failed to load the dense head from '{a.dense_head}': {e}", file=sys.stderr)
            return 1

    depth = None
    if a.depth_head:
        try:
            depth = binding.depth_head(a.depth_head)
        except (OSError, ValueError, KeyError) as e:
            print(f"main: failed to load the depth head from '{a.depth_head}': {e}", file=sys.stderr)
            return 1

    if a.pack:
        # several images, each at its own aspect-preserving shape, in ONE forward of a packed context; the lines of the per-image --img-fit path, image after image
        files = [f for f in a.inp.split(",") if f]
        try:
            imgs = [_decode(f) for f in files]
        except Exception as e:
            print(f"main: failed to load an image of '{a.inp}': {e}", file=sys.stderr)
            return 1
        try:
            if a.pack_u8:
                shapes = binding.pack_fit_shapes(model, [im.shape[:2] for im in imgs], a.img_fit)
            else:
                pixels, shapes = binding.pack_images(imgs, pp_rect, a.img_fit, patch=model.hparams.patch_size)
            tokens = int(binding.pack_check(model, shapes, 2 ** 31 - 1, len(files))[-1])
            ctx = binding.PackContext(model, device=a.device, max_tokens=tokens, max_images=len(files), dtype=dt, pos_interp=geometry["pos_interp"])
            if dense:
                # a label map per image at the ORIGINAL's size (never below the patch grid: a tiny original keeps the preprocessed shape's side)
                P = model.hparams.patch_size
                outs = [(max(im.shape[0], h // P), max(im.shape[1], w // P)) for im, (h, w) in zip(imgs, shapes)]
                ctx.dense_set(dense["weight"], dense["bias"], dense["layers"], max_pixels=sum(h * w for h, w in outs))
                ctx.dense_out(outs)
            if depth:
                # a depth map per image at the ORIGINAL's size (never below the fine plane: a tiny original keeps that side of the fine plane)
                P, u = model.hparams.patch_size, depth["upsample"]
                outs = [(max(im.shape[0], u * (h // P)), max(im.shape[1], u * (w // P))) for im, (h, w) in zip(imgs, shapes)]
                ctx.depth_set(depth["wp"], depth["wc"], depth["bias"], depth["bins"], depth["layers"], u, depth["min_depth"], depth["max_depth"],
                              max_pixels=sum(h * w for h, w in outs), norm=depth["norm"])
                ctx.depth_out(outs)
            if a.attn_map:
                # where the model looked, per image on its own grid: the rollout row, or the head mean of the last layer's class-token maps
                L, P, Tp = model.hparams.num_hidden_layers, model.hparams.patch_size, model.num_prefix
                ctx.attn_enable([] if a.attn_kind == "rollout" else [L - 1], rollout=a.attn_kind == "rollout",
                                max_sq_tokens=sum((Tp + (h // P) * (w // P)) ** 2 for h, w in shapes))
            if a.pack_u8:
                ctx.u8_set(pp_rect, max_src_bytes=sum(im.size for im in imgs))
                probs, _ = ctx.forward_u8(imgs, shapes)
            else:
                probs, _ = ctx.forward_flat(pixels, shapes)
            maps = ctx.dense_read()[0] if dense else None
            dmaps = ctx.depth_read()[0] if depth else None
            amaps = ctx.attn_read() if a.attn_map else None
        except binding.VitxError as e:
            print(f"main: the packed forward failed: {e}", file=sys.stderr)
            return 1
        for k, (f, (h, w), p) in enumerate(zip(files, shapes, probs)):
            print(f"main: '{f}' at ({w} x {h})", file=sys.stderr)
            if a.attn_map:
                cls, roll = amaps[k]
                m, path = roll if a.attn_kind == "rollout" else cls[0].mean(axis=0), f"{a.attn_map}.{k}.pgm"
                with open(path, "wb") as fo:
                    fo.write(attn_pgm(ctx.attn_grid(k, m), (int(h), int(w))))
                print(f"main: wrote the {a.attn_kind} attention map to '{path}'", file=sys.stderr)
            if depth:
                dm, path = dmaps[k], f"{a.depth_out}.{k}.npy"
                with open(path, "wb") as fo:
                    np.save(fo, dm)
                print(f"main: wrote the {dm.shape[1]} x {dm.shape[0]} depth map to '{path}'", file=sys.stderr)
                print(f" > depth : min {float(np.nanmin(dm)):.3f} median {float(np.nanmedian(dm)):.3f} max {float(np.nanmax(dm)):.3f}")
                continue
            if dense:
                lab, path = maps[k], f"{a.dense_out}.{k}.pgm"
                with open(path, "wb") as fo:
                    fo.write(f"P5\n{lab.shape[1]} {lab.shape[0]}\n255\n".encode() + lab.tobytes())
                print(f"main: wrote the {lab.shape[1]} x {lab.shape[0]} label map to '{path}'", file=sys.stderr)
                share = np.bincount(lab.reshape(-1), minlength=dense["weight"].shape[0]) / lab.size
                for c in np.argsort(-share, kind="stable")[:a.topk]:
                    if share[c] > 0:
                        print(f" > {dense['names'][c] if dense['names'] else f'class_{c}'} : {share[c]:.2f}")
                continue
            for i, v in zip(*binding.topk(p, a.topk)):
                print(f" > {model.label(i)} : {v:.2f}")
        return 0

    if a.dir is None:
        try:
            img0 = _decode(a.inp)
        except Exception as e:                                              # main.cpp:69-73
            print(f"main: failed to load image from '{a.inp}': {e}", file=sys.stderr)
            return 1
        print(f"main: loaded image '{a.inp}' ({img0.shape[1]} x {img0.shape[0]})", file=sys.stderr)
        try:
            if a.img_fit:
                w_fit, h_fit = binding.rect_shape(img0.shape[1], img0.shape[0], model.hparams.patch_size, a.img_fit)
                rect = (h_fit, w_fit)
            img1 = preprocess(img0)
        except binding.VitxError as e:
            print(f"main: failed to preprocess '{a.inp}': {e}", file=sys.stderr)
            return 1
        print(f"processed, out dims : ({rect[1]} x {rect[0]})" if rect else f"processed, out dims : ({S} x {S})", file=sys.stderr)
        try:
            ctx = binding.Context(model, device=a.device, max_batch=1, dtype=dt, img_shape=rect, **geometry)
        except binding.VitxError as e:
            print(f"main: failed to create the context: {e}", file=sys.stderr)
            return 1
        if a.attn_map:
            L = model.hparams.num_hidden_layers
            ctx.attn_enable([] if a.attn_kind == "rollout" else [L - 1], rollout=a.attn_kind == "rollout")
        if a.embed:
            ctx.feat_enable(**feat)
        if bank:
            try:
                ctx.zeroshot_set(bank["embeds"], bank["kind"], bank["scale"], bank["bias"])
            except binding.VitxError as e:
                print(f"main: the bank of '{a.zero_shot or a.text_model}' does not fit this model: {e}", file=sys.stderr)
                return 1
        if gallery:
            try:
                labels = gallery["labels"] if "labels" in gallery and len(gallery.get("label_names", ())) else None
                ctx.nn_set(gallery["embeds"], min(a.topk, len(gallery["embeds"])), int(gallery["source"]) if "source" in gallery else binding.NN_EMBED, labels,
                           len(gallery["label_names"]) if labels is not None else 0, a.nn_temperature)
            except binding.VitxError as e:
                print(f"main: the gallery of '{a.gallery}' does not fit this model: {e}", file=sys.stderr)
                return 1
        if dense:
            try:
                ctx.dense_set(dense["weight"], dense["bias"], dense["layers"])
            except binding.VitxError as e:
                print(f"main: the head of '{a.dense_head}' does not fit this model: {e}", file=sys.stderr)
                return 1
        if depth:
            try:
                ctx.depth_set(depth["wp"], depth["wc"], depth["bias"], depth["bins"], depth["layers"], depth["upsample"], depth["min_depth"], depth["max_depth"],
                              norm=depth["norm"])
            except binding.VitxError as e:
                print(f"main: the head of '{a.depth_head}' does not fit this model: {e}", file=sys.stderr)
                return 1
        probs = ctx.forward(img1[None])[0]
        if depth:
            dm = ctx.depth_read(1)[0][0]
            with open(a.depth_out, "wb") as f:
                np.save(f, dm)
            print(f"main: wrote the {dm.shape[1]} x {dm.shape[0]} depth map to '{a.depth_out}'", file=sys.stderr)
            print("", file=sys.stderr)
            print(f" > depth : min {float(np.nanmin(dm)):.3f} median {float(np.nanmedian(dm)):.3f} max {float(np.nanmax(dm)):.3f}")
            return 0
        if dense:
            lab = ctx.dense_read(1)[0][0]
            with open(a.dense_out, "wb") as f:
                f.write(f"P5\n{lab.shape[1]} {lab.shape[0]}\n255\n".encode() + lab.tobytes())
            print(f"main: wrote the {lab.shape[1]} x {lab.shape[0]} label map to '{a.dense_out}'", file=sys.stderr)
            print("", file=sys.stderr)
            share = np.bincount(lab.reshape(-1), minlength=dense["weight"].shape[0]) / lab.size
            for k in np.argsort(-share, kind="stable")[:a.topk]:
                if share[k] > 0:
                    print(f" > {dense['names'][k] if dense['names'] else f'class_{k}'} : {share[k]:.2f}")
            return 0
        if gallery:
            idx, score, vote = ctx.nn_read(1)
            print("", file=sys.stderr)
            for g, s in zip(idx[0], score[0]):
                print(f" ~ {gallery['paths'][g] if 'paths' in gallery else g} : {s:.4f}")
            if vote is not None:
                names = gallery["label_names"]
                for i, p in zip(*binding.topk(vote[0], min(a.topk, len(names)))):
                    print(f" > {names[i]} : {p:.2f}")
            return 0
        if a.embed:
            np.save(a.embed, last(ctx))
            print(f"main: wrote the {a.embed_kind} embedding to '{a.embed}'", file=sys.stderr)
        if a.attn_map:
            cls, roll = ctx.attn_read()
            m = roll[0] if a.attn_kind == "rollout" else cls[0, 0].mean(axis=0)
            with open(a.attn_map, "wb") as f:
                f.write(attn_pgm(ctx.attn_grid(m), rect or S))
            print(f"main: wrote the {a.attn_kind} attention map to '{a.attn_map}'", file=sys.stderr)
        label = model.label
        if bank:                                                            # the bank's classes in place of the file's own head
            probs, label = ctx.zeroshot_read(1)[0], lambda i: bank["labels"][i]
        idx, val = binding.topk(probs, a.topk)
        print("", file=sys.stderr)
        for i, p in zip(idx, val):                                          # vit.cpp:1062-1067
            print(f" > {label(i)} : {p:.2f}")
        t_all = time.perf_counter() - t_main
        print("\n", file=sys.stderr)
        print(f"main:    model load time = {t_load * 1e3:8.2f} ms", file=sys.stderr)
        print(f"main:    processing time = {(t_all - t_load) * 1e3:8.2f} ms", file=sys.stderr)
        print(f"main:    total time      = {t_all * 1e3:8.2f} ms", file=sys.stderr)
        return 0

    # ---- accuracy harness: DIR/<label>/<image>; the label must be one of the model's id2label strings
    label_id = {model.label(i): i for i in range(model.num_classes) if model.label(i) is not None}
    files, truth = [], []
    for d in sorted(os.listdir(a.dir)):
        sub = os.path.join(a.dir, d)
        if not os.path.isdir(sub) or d not in label_id:
            continue
        for f in sorted(os.listdir(sub)):
            files.append(os.path.join(sub, f)); truth.append(label_id[d])
    if not files:
        print(f"main: no <label>/<image> files under '{a.dir}' match the model's labels", file=sys.stderr)
        return 1
    try:
        ctx = binding.Context(model, device=a.device, max_batch=min(a.batch, len(files)), dtype=dt, img_shape=rect, **geometry)
    except binding.VitxError as e:
        print(f"main: failed to create the context: {e}", file=sys.stderr)
        return 1
    if a.embed:
        ctx.feat_enable(**feat)
    rows = []
    correct = 0
    t0 = time.perf_counter()
    for lo in range(0, len(files), ctx.max_batch):
        chunk = files[lo:lo + ctx.max_batch]
        batch = np.stack([preprocess(_decode(f)) for f in chunk])
        pred = ctx.forward(batch).argmax(1)
        if a.embed:
            rows.append(last(ctx).copy())
        correct += int((pred == np.asarray(truth[lo:lo + len(chunk)])).sum())
    el = time.perf_counter() - t0
    if a.embed:
        np.save(a.embed, np.concatenate(rows))
        with open(a.embed + ".txt", "w") as f:
            f.write("".join(p + "\n" for p in files))
        print(f"main: wrote {len(files)} {a.embed_kind} embeddings to '{a.embed}' and their file names to '{a.embed}.txt'", file=sys.stderr)
    print(f"top-1 accuracy: {correct / len(files):.4f} ({correct}/{len(files)})  {len(files) / el:.1f} images/s incl. decode + preprocess")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
