"""Converter: a HuggingFace `transformers` vision model or a timm state dict -> the legacy-ggml ".gguf" model file (ggml_file.write_model).

An offline tool, not on the compute path.  The file holds timm's VisionTransformer names in the order the loader reads them -- cls_token, pos_embed,
patch_embed.proj.*, per block norm1, the fused attn.qkv (q, k, v rows in that order), attn.proj, norm2, mlp.fc1, mlp.fc2, then norm.* and head.* --
plus the extensions of include/vitx.h: `arch`, `preproc`, `reg_token`, `pre_norm.*`, the [C][2 D] head and `attn_pool.*`.  A HuggingFace family
differs from it in its names and in a few tensors around the blocks: BlockNames states a family's block names as data and map_blocks is the one
place that renames, fuses and folds a block; the embeddings, the final norm and the head are each family's own few lines (its *_state_dict_to_timm
function documents them).  convert_hf_model writes every family through one path, chosen by the FAMILIES table.

What is converted
  ViT      ViTForImageClassification, both namings (`vit.encoder.layer.N` before transformers 5, `vit.layers.N` from 5 on); with --vitstr a
           one-channel ViTSTR scene-text recogniser, whose file carries the character set as labels.
  DINOv2   Dinov2ForImageClassification, Dinov2WithRegistersForImageClassification; with --no-head the backbones Dinov2Model /
           Dinov2WithRegistersModel.  Register tokens, folded LayerScale, the head over concat(cls, mean of the patch tokens).
  CLIP     CLIPVisionModelWithProjection, CLIPModel (its vision tower and visual_projection); with --no-head a CLIPVisionModel.
  SigLIP   SiglipVisionModel, SiglipModel (its vision tower): no class token, the attention-pooling head.
  DINOv3   DINOv3ViTModel (ViT-S/B/L): class token, register tokens, folded LayerScale, and rotary position embeddings -- the `rope` tensor,
           f32 [4] = {1, rope_theta, 0, 0}, beside an all-zero pos_embed (include/vitx.h "rotary position embeddings").  A backbone: the zero head.
  gated    DINOv2 ViT-g/14 (use_swiglu_ffn) and DINOv3 ViT-H+ (use_gated_mlp), OPT-IN: convert_hf_model(..., gated_mlp=True) / --gated-mlp.  The MLP is
           fc2(silu(gate(x)) . up(x)) with a hidden width F that is not 4 x hidden: the `glu` tensor, f32 [4] = {1, F, 0, 0}, directly after `arch` /
           `rope`; mlp.fc1 = [2 F][D], gate rows then up rows (DINOv2's weights_in as it is; DINOv3's cat(gate_proj, up_proj)), mlp.fc2 = [D][F]
           (include/vitx.h "gated MLP").  Without the switch such a model is refused: the file cannot be read by the reference or by an engine build
           before the `glu` tensor existed.
  timm     a VisionTransformer state_dict (--timm-state-dict model.pth, no `timm` import): convert_timm_state_dict.

Every model's settings travel with it.  The MLP activation (`hidden_act`: gelu -> erf-GELU, gelu_pytorch_tanh / gelu_new -> tanh-GELU, quick_gelu ->
QuickGELU) and `layer_norm_eps` become the `arch` tensor, f32 [4] = {activation, eps, 0, 0}, the first of the file -- written ONLY when they differ
from (tanh-GELU, 1e-6), the reference's arithmetic, so that such a file is byte for byte the reference converter's and stays readable by the
reference (with_arch).  The HuggingFace ViT default is erf-GELU with 1e-12; timm and DINOv2 use erf-GELU.  A timm state dict carries no config:
--act {tanh,erf,quick} and --eps state its settings (timm's VisionTransformer uses nn.GELU: --act erf); without them the file is the reference's.

Its preprocessing travels too (include/vitx.h "each model's own preprocessing"): the `preprocessor_config.json` beside a HuggingFace checkpoint
(hf_preproc: `do_resize` / `size` {"shortest_edge"} or {"height", "width"}, `resample` 2 = PIL bilinear or 3 = PIL bicubic, `do_center_crop` /
`crop_size`, `image_mean`, `image_std`, `do_rescale` with the usual 1/255) is written as the `preproc` tensor directly after `arch`, with mean255 =
f32(255.0 * mean).  --no-preproc writes the file without it: the reference's stretch and ImageNet mean / std then apply.  A timm checkpoint has no
processor: the --pp-* options state one (cli_preproc); with none of them no tensor is written and the file keeps the reference's bytes.

What is refused, by name: an activation the forward path does not evaluate; an MLP that is not 4 x hidden (SigLIP SO400M's 4304); a head_dim that
is no multiple of 8 up to 128; qkv_bias=False; SwiGLU (use_swiglu_ffn) and DINOv3's gated MLP (use_gated_mlp) unless gated_mlp=True / --gated-mlp opts in, a gate
activation other than silu and a gated width that is no multiple of 64; qk-norm, fc_norm and distillation tokens; a SigLIP tower without its pooling head
(vision_use_head = False), SiglipForImageClassification (a mean-pool classifier: no slot), Siglip2VisionModel (NaFlex: its patch embedding is a
Linear); --no-head on a ViT, and a model without classifier or projection converted without it; --vitstr on anything but a one-channel ViT; in a
preprocessor_config whatever the engine's preprocess cannot honour -- another resample code, do_resize off, padding, a channel flip, a final size
that is not the model's -- with the field's name.

Zero-shot banks (include/vitx.h "zero-shot classification"): the engine has no text encoder and no tokenizer, so the bank of a CLIPModel /
SiglipModel is computed here, once per set of prompts, by its TEXT tower (zeroshot_bank).  --zero-shot-ids ids.npy [--zero-shot-labels labels.txt]
--zero-shot-out bank.npz writes it as an .npz (save_bank / load_bank; vit_cli.py --zero-shot reads it); the model file is converted as usual.

At another input size (--img-size N) pos_embed is resampled; transformers 5.x resamples the DINOv2-with-registers table with antialias=True, which
`--pos-interp bicubic-aa` reproduces (plain Dinov2 and ViT: `bicubic`).

    python -m ... convert.py <hf_model_dir_or_name> <out.gguf> [--ftype 1] [--no-head] [--no-preproc] [--vitstr] [--img-size N]
    python -m ... convert.py <hf_clip_or_siglip_dir> <out.gguf> --zero-shot-ids ids.npy [--zero-shot-labels labels.txt] --zero-shot-out bank.npz
    python -m ... convert.py --timm-state-dict <checkpoint.pth> <out.gguf> [--ftype 1] [--heads H] [--labels labels.json] [--act erf] [--eps 1e-6] [--pp-*]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from collections import namedtuple
from typing import Dict

import numpy as np

from .ggml_file import (HParams, write_model, preproc_slots, preproc_fields, IMAGENET_MEAN, IMAGENET_STD,
                        PP_STRETCH, PP_SHORTEST_EDGE, PP_PIL_BILINEAR, PP_PIL_BICUBIC,
                        ACT_TANH, ACT_ERF, ACT_QUICK, ZS_SOFTMAX, ZS_SIGMOID)


_HF_ACTS = {"gelu": ACT_ERF, "gelu_pytorch_tanh": ACT_TANH, "gelu_new": ACT_TANH, "quick_gelu": ACT_QUICK}
_ACT_NAMES = {"tanh": ACT_TANH, "erf": ACT_ERF, "quick": ACT_QUICK}
NO_HEAD_LABELS = {0: "(no head)"}


def hf_activation(cfg) -> int:
    """enum vitx_activation of a HuggingFace config's hidden_act; an activation the forward path does not evaluate is refused by name."""
    act = getattr(cfg, "hidden_act", "gelu")
    if not isinstance(act, str) or act not in _HF_ACTS:
        raise ValueError(f"hidden_act {act!r} is not supported (the forward path evaluates {sorted(_HF_ACTS)})")
    return _HF_ACTS[act]


def with_arch(tensors: Dict[str, np.ndarray], activation: int, eps: float) -> Dict[str, np.ndarray]:
    """`tensors` with the `arch` tensor [activation, eps, 0, 0] in front -- only when it says something else than (tanh-GELU, 1e-6), so that a
    file of the reference's arithmetic stays byte for byte what it was."""
    eps32 = np.float32(eps)
    if activation not in (ACT_TANH, ACT_ERF, ACT_QUICK) or not np.isfinite(eps32) or not eps32 > 0:
        raise ValueError(f"activation {activation} / eps {eps}: the activation is 0, 1 or 2, eps a finite float32 > 0")
    if activation == ACT_TANH and eps32 == np.float32(1e-6):
        return tensors
    out = {"arch": np.array([activation, eps32, 0, 0], np.float32)}
    out.update(tensors)
    return out


def _square(v, field: str):
    """A processor's size entry -- {"height": h, "width": w}, [h, w] or an int -- as (width, height)."""
    if isinstance(v, dict) and "height" in v and "width" in v:
        return int(v["width"]), int(v["height"])
    if isinstance(v, (list, tuple)) and len(v) == 2:
        return int(v[1]), int(v[0])
    if isinstance(v, int) and not isinstance(v, bool):
        return v, v
    raise ValueError(f"preprocessor_config: {field} = {v!r} is not a height / width pair")


def hf_preproc(cfg: dict, img_size: int) -> np.ndarray:
    """The 16 slots of the `preproc` tensor from a HuggingFace preprocessor_config.json (a dict), for a model that takes img_size^2 images.
    Defaults are the image processors' own: do_resize, do_rescale and do_normalize on, do_center_crop off.  A legacy integer `size` is the
    shortest edge when the processor centre-crops (CLIP's) and a square otherwise (ViT's).  Whatever the engine cannot honour raises a
    ValueError that names the field."""
    for field in ("do_pad", "do_flip_channel_order", "do_color_quantize", "do_reduce_labels"):
        if cfg.get(field):
            raise ValueError(f"preprocessor_config: {field} = {cfg[field]!r} is not supported")
    if cfg.get("do_convert_rgb") is False and cfg.get("image_mode") not in (None, "RGB"):
        raise ValueError(f"preprocessor_config: do_convert_rgb is off for {cfg.get('image_mode')!r} images; the engine decodes every file to RGB")
    if not cfg.get("do_rescale", True):
        raise ValueError("preprocessor_config: do_rescale = False is not supported (pixels are scaled by 1/255 before mean / std)")
    rf = cfg.get("rescale_factor", 1.0 / 255.0)
    if abs(float(rf) * 255.0 - 1.0) > 1e-6:
        raise ValueError(f"preprocessor_config: rescale_factor = {rf!r} is not the usual 1/255")
    if not cfg.get("do_resize", True):
        raise ValueError("preprocessor_config: do_resize = False is not supported (the engine's preprocess always resizes)")
    if "resample" not in cfg or cfg["resample"] not in (2, 3):
        raise ValueError(f"preprocessor_config: resample = {cfg.get('resample')!r}: 2 (PIL bilinear) and 3 (PIL bicubic) are supported")
    filt = PP_PIL_BILINEAR if cfg["resample"] == 2 else PP_PIL_BICUBIC
    crop = 0
    if cfg.get("do_center_crop", False):
        if "crop_size" not in cfg:
            raise ValueError("preprocessor_config: do_center_crop without crop_size")
        cw, ch = _square(cfg["crop_size"], "crop_size")
        if cw != ch:
            raise ValueError(f"preprocessor_config: crop_size = {cfg['crop_size']!r} is not square")
        crop = cw
    size = cfg.get("size")
    if isinstance(size, dict) and "shortest_edge" in size and "height" not in size:
        if "longest_edge" in size:
            raise ValueError(f"preprocessor_config: size = {size!r}: a longest_edge bound is not supported")
        mode, a, b = PP_SHORTEST_EDGE, int(size["shortest_edge"]), 0
    elif isinstance(size, int) and not isinstance(size, bool) and crop:
        mode, a, b = PP_SHORTEST_EDGE, size, 0
    elif size is not None:
        mode = PP_STRETCH
        a, b = _square(size, "size")
    else:
        raise ValueError("preprocessor_config: size is missing")
    if mode == PP_SHORTEST_EDGE and not crop:
        raise ValueError(f"preprocessor_config: size = {size!r} without do_center_crop gives images of the source's aspect; the model takes {img_size} x {img_size}")
    if crop:
        if crop != img_size:
            raise ValueError(f"preprocessor_config: crop_size = {cfg['crop_size']!r}, the model takes {img_size} x {img_size}")
        if crop > a or (mode == PP_STRETCH and crop > b):
            raise ValueError(f"preprocessor_config: crop_size = {cfg['crop_size']!r} is larger than size = {size!r} (padding is not supported)")
    elif (a, b) != (img_size, img_size):
        raise ValueError(f"preprocessor_config: size = {size!r}, the model takes {img_size} x {img_size}")
    if cfg.get("do_normalize", True):
        mean, std = cfg.get("image_mean"), cfg.get("image_std")
        for field, v in (("image_mean", mean), ("image_std", std)):
            if not isinstance(v, (list, tuple)) or len(v) != 3:
                raise ValueError(f"preprocessor_config: {field} = {v!r} is not one value per RGB channel")
        if not all(np.isfinite(np.float32(255.0 * x)) and np.float32(255.0 * x) > 0 for x in std):
            raise ValueError(f"preprocessor_config: image_std = {std!r} is not finite and positive")
    else:
        mean, std = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)          # out = q / 255
    return preproc_slots(mode, a, b, filt, crop=crop, crop_round=0, mean=mean, std=std)


def cli_preproc(img_size: int, resize: int = 0, crop: int = 0, filt: str = "", mean=None, std=None, crop_round: str = ""):
    """The `preproc` slots of a timm checkpoint from the --pp-* options (torchvision's Resize(N) + CenterCrop(M) + Normalize on PIL images);
    None when none of them is given.  resize: the shortest edge (default: the crop); crop: the centre crop (default: the model's img_size)."""
    if not (resize or crop or filt or mean or std or crop_round):
        return None
    crop = crop or img_size
    if crop != img_size:
        raise ValueError(f"--pp-crop {crop}: the model takes {img_size} x {img_size}")
    resize = resize or crop
    if resize < crop:
        raise ValueError(f"--pp-resize {resize} is smaller than the crop {crop} (padding is not supported)")
    if (filt or "bicubic") not in ("bilinear", "bicubic"):
        raise ValueError(f"--pp-filter {filt!r}: bilinear or bicubic")
    if (crop_round or "floor") not in ("floor", "torchvision"):
        raise ValueError(f"--pp-crop-round {crop_round!r}: floor or torchvision")
    return preproc_slots(PP_SHORTEST_EDGE, resize, 0, PP_PIL_BILINEAR if filt == "bilinear" else PP_PIL_BICUBIC, crop=crop,
                         crop_round=1 if crop_round == "torchvision" else 0, mean=mean or IMAGENET_MEAN, std=std or IMAGENET_STD)


# --------------------------------------------------------------------------- what every family shares
def fold_layer_scale(weight: np.ndarray, bias: np.ndarray, lam: np.ndarray):
    """LayerScale folded into the linear layer in front of it, in f32: (lambda[o] * W[o][:], lambda[o] * b[o]).  It has no file slot and needs
    none: y = x + lambda * (W a + b) = x + (lambda * W) a + lambda * b; the fold happens before the file type's rounding."""
    lam = np.asarray(lam, np.float32).reshape(-1)
    return (np.asarray(weight, np.float32) * lam[:, None]).astype(np.float32), (np.asarray(bias, np.float32) * lam).astype(np.float32)


# One family's names for the tensors of a transformer block, each without its .weight / .bias.  layer: the block's prefix behind the state dict's
# own, with {i} for the layer; qkv: the three projections the file fuses; ls1 / ls2: the LayerScale tensors behind the attention and the MLP.
BlockNames = namedtuple("BlockNames", "layer qkv norm1 proj norm2 fc1 fc2 ls1 ls2", defaults=("", ""))


_HF_QKV = ("attention.attention.query", "attention.attention.key", "attention.attention.value")
VIT_BLOCKS_V4 = BlockNames("vit.encoder.layer.{i}.", _HF_QKV, "layernorm_before", "attention.output.dense", "layernorm_after", "intermediate.dense", "output.dense")
VIT_BLOCKS_V5 = BlockNames("vit.layers.{i}.", ("attention.q_proj", "attention.k_proj", "attention.v_proj"), "layernorm_before", "attention.o_proj", "layernorm_after",
                           "mlp.fc1", "mlp.fc2")
DINOV2_BLOCKS = BlockNames("encoder.layer.{i}.", _HF_QKV, "norm1", "attention.output.dense", "norm2", "mlp.fc1", "mlp.fc2", "layer_scale1.lambda1", "layer_scale2.lambda1")
DINOV3_BLOCKS = BlockNames("layer.{i}.", ("attention.q_proj", "attention.k_proj", "attention.v_proj"), "norm1", "attention.o_proj", "norm2", "mlp.up_proj", "mlp.down_proj",
                           "layer_scale1.lambda1", "layer_scale2.lambda1")
# the gated MLPs (gated_mlp=True): DINOv2's weights_in is already gate rows then up rows; DINOv3's gate_proj / up_proj are concatenated under the
# name `mlp.gate_up` by dinov3_state_dict_to_timm before the blocks are mapped
DINOV2_GLU_BLOCKS = DINOV2_BLOCKS._replace(fc1="mlp.weights_in", fc2="mlp.weights_out")
DINOV3_GLU_BLOCKS = DINOV3_BLOCKS._replace(fc1="mlp.gate_up")
CLIP_BLOCKS = BlockNames("encoder.layers.{i}.", ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), "layer_norm1", "self_attn.out_proj", "layer_norm2",
                         "mlp.fc1", "mlp.fc2")          # SigLIP's too


def _put(out: dict, dst: str, sd, src: str, layer_scale: str = "") -> None:
    w, b = sd[src + ".weight"], sd[src + ".bias"]
    out[dst + ".weight"], out[dst + ".bias"] = fold_layer_scale(w, b, sd[layer_scale]) if layer_scale else (w, b)


def map_blocks(out: dict, sd, names: BlockNames, num_layers: int, pre: str = "") -> None:
    """Append the blocks of `sd` to `out` under the file's names and in its order: per layer norm1, attn.qkv (q, k, v concatenated along the
    rows, timm's order: vit.cpp:826-834), attn.proj, norm2, mlp.fc1, mlp.fc2, each as .weight then .bias.  LayerScale, where the family
    has it, is folded."""
    for i in range(num_layers):
        q, p = pre + names.layer.format(i=i), f"blocks.{i}."
        qkv = [q + n for n in names.qkv]
        if any(n + ".bias" not in sd for n in qkv):
            raise ValueError("qkv_bias=False: the file format carries the fused qkv bias")
        _put(out, p + "norm1", sd, q + names.norm1)
        out[p + "attn.qkv.weight"] = np.concatenate([sd[n + ".weight"] for n in qkv], 0)
        out[p + "attn.qkv.bias"] = np.concatenate([sd[n + ".bias"] for n in qkv], 0)
        _put(out, p + "attn.proj", sd, q + names.proj, names.ls1 and q + names.ls1)
        _put(out, p + "norm2", sd, q + names.norm2)
        _put(out, p + "mlp.fc1", sd, q + names.fc1)
        _put(out, p + "mlp.fc2", sd, q + names.fc2, names.ls2 and q + names.ls2)


def _zero_head(out: dict, D: int) -> None:
    """The one-class class-token head of zeros that keeps a file without classifier well-formed (NO_HEAD_LABELS); embeddings are read through vitx_feat_*."""
    out["head.weight"] = np.zeros((1, D), np.float32); out["head.bias"] = np.zeros((1,), np.float32)


def _require_mlp_4x(cfg, field: str, want: int, note: str = "") -> None:
    have = getattr(cfg, field, want)
    if have != want:
        raise ValueError(f"{field} {have}: the file format holds a 4 x hidden MLP{note}")


_GATED_HOWTO = ("pass gated_mlp=True (convert.py --gated-mlp) to write it with the `glu` tensor: such a file cannot be read by the reference or by an engine "
                "build before the gated MLP")


def _glu_tensor(F: int) -> np.ndarray:
    """The `glu` tensor {1 = SwiGLU, F, 0, 0} of a gated MLP of hidden width F (include/vitx.h "gated MLP")."""
    if F < 64 or F % 64:
        raise ValueError(f"gated MLP of hidden width {F}: the forward path takes multiples of 64 (the GEMMs' K step)")
    return np.array([1, F, 0, 0], np.float32)


def _f32(tensors: dict) -> Dict[str, np.ndarray]:
    """Every tensor (a numpy array or a torch tensor) as a contiguous f32 array, in the order given."""
    return {k: np.ascontiguousarray(np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v, np.float32)) for k, v in tensors.items()}


def grid_side(pos_embed, prefix_rows: int) -> int:
    """g of a position table [1][prefix_rows + g^2][D] (prefix_rows 1: the class token's row; 0: a model without class token)."""
    n = int(np.shape(pos_embed)[1])
    g = int(round(max(n - prefix_rows, 0) ** 0.5))
    if g < 1 or g * g + prefix_rows != n:
        raise ValueError(f"pos_embed {tuple(np.shape(pos_embed))}: not {'1 + ' if prefix_rows else ''}a square grid")
    return g


# --------------------------------------------------------------------------- the families' embeddings, final norm and head
def state_dict_to_timm(sd: Dict[str, np.ndarray], num_layers: int) -> Dict[str, np.ndarray]:
    """An HF ViTForImageClassification state dict (numpy arrays) under the file's names, in the order the loader reads them.  The two namings of
    the blocks are told apart by probing for transformers 5's `vit.layers.0`."""
    e = "vit.embeddings."
    out = {"cls_token": sd[e + "cls_token"], "pos_embed": sd[e + "position_embeddings"]}
    _put(out, "patch_embed.proj", sd, e + "patch_embeddings.projection")
    map_blocks(out, sd, VIT_BLOCKS_V5 if "vit.layers.0.attention.q_proj.weight" in sd else VIT_BLOCKS_V4, num_layers)
    _put(out, "norm", sd, "vit.layernorm")
    _put(out, "head", sd, "classifier")
    return _f32(out)


def dinov2_state_dict_to_timm(sd: Dict[str, np.ndarray], cfg, no_head: bool = False, gated_mlp: bool = False) -> Dict[str, np.ndarray]:
    """An HF Dinov2[WithRegisters]{ForImageClassification, Model} state dict (numpy arrays) under the file's names and order.  register_tokens ->
    `reg_token` [1][R][D] directly after cls_token; the classifier is the [C][2 D] head over concat(cls, mean of the patch tokens) (include/vitx.h
    "register tokens and the pooled head": the reference's loader cannot read such a file); LayerScale is folded (fold_layer_scale); mask_token is
    dropped.  qk-norm, fc_norm and distillation tokens are refused by name.  no_head: a backbone, which gets the zero head.
    use_swiglu_ffn (ViT-g/14) is refused by name unless gated_mlp: then mlp.weights_in -> mlp.fc1 ([2 F][D]: HF chunks it into gate, up in that
    order), mlp.weights_out -> mlp.fc2 with LayerScale folded as ever, and `glu` = {1, F, 0, 0} in front, F read off weights_out's shape."""
    swiglu = bool(getattr(cfg, "use_swiglu_ffn", False))
    if swiglu and not gated_mlp:
        raise ValueError("use_swiglu_ffn: the SwiGLU MLP of the DINOv2 giant models is not converted by default; " + _GATED_HOWTO)
    if gated_mlp and not swiglu:
        raise ValueError("gated_mlp=True, but the model has the plain MLP (use_swiglu_ffn is off)")
    for k in sd:
        for bad, what in (("q_norm", "qk-norm"), ("k_norm", "qk-norm"), ("fc_norm", "fc_norm"), ("dist_token", "a distillation token"), ("distillation", "a distillation token")):
            if bad in k:
                raise ValueError(f"tensor {k!r}: {what} is not supported")
    if not swiglu:
        _require_mlp_4x(cfg, "mlp_ratio", 4)
    pre = next((p for p in ("dinov2_with_registers.", "dinov2.", "") if p + "embeddings.cls_token" in sd), None)
    if pre is None:
        raise ValueError("not a DINOv2 state dict: embeddings.cls_token is missing")
    e = pre + "embeddings."
    out = {}
    if swiglu:
        w_out = pre + DINOV2_GLU_BLOCKS.layer.format(i=0) + "mlp.weights_out.weight"
        if w_out not in sd:
            raise ValueError(f"use_swiglu_ffn, but {w_out} is missing")
        out["glu"] = _glu_tensor(int(np.shape(sd[w_out])[1]))
    out["cls_token"] = sd[e + "cls_token"]
    if e + "register_tokens" in sd:
        out["reg_token"] = sd[e + "register_tokens"]
    out["pos_embed"] = sd[e + "position_embeddings"]
    _put(out, "patch_embed.proj", sd, e + "patch_embeddings.projection")
    map_blocks(out, sd, DINOV2_GLU_BLOCKS if swiglu else DINOV2_BLOCKS, cfg.num_hidden_layers, pre)
    _put(out, "norm", sd, pre + "layernorm")
    if no_head:
        _zero_head(out, int(np.shape(out["cls_token"])[-1]))
    elif "classifier.weight" not in sd:
        raise ValueError("the model has no classifier: convert a backbone with no_head=True (--no-head)")
    else:
        _put(out, "head", sd, "classifier")
    return _f32(out)


def clip_state_dict_to_timm(sd: Dict[str, np.ndarray], cfg, no_head: bool = False) -> Dict[str, np.ndarray]:
    """An HF CLIPVisionModelWithProjection / CLIPModel / CLIPVisionModel state dict (numpy arrays) under the file's names and order.
    class_embedding -> cls_token, position_embedding -> pos_embed, pre_layrnorm -> `pre_norm.*` directly after pos_embed, the bias-free patch
    convolution gets a zero bias, post_layernorm -> norm, and the bias-free visual_projection [E][D] becomes head.weight with a zero head.bias:
    the file has E "classes" (labelled dim_0 .. dim_{E-1}), its logits are CLIP's image_embeds and its probabilities mean nothing -- zero-shot
    probabilities come from a bank of text embeddings (zeroshot_bank).  no_head: a tower without projection, which gets the zero head."""
    pre = next((p for p in ("vision_model.", "") if p + "embeddings.class_embedding" in sd), None)
    if pre is None:
        raise ValueError("not a CLIP vision state dict: embeddings.class_embedding is missing")
    e = pre + "embeddings."
    D = int(np.shape(sd[e + "class_embedding"])[-1])
    _require_mlp_4x(cfg, "intermediate_size", 4 * D)
    if e + "patch_embedding.bias" in sd:
        raise ValueError("patch_embedding.bias: not a CLIP vision tower (its patch convolution has no bias)")
    out = {"cls_token": np.reshape(sd[e + "class_embedding"], (1, 1, D)), "pos_embed": np.reshape(sd[e + "position_embedding.weight"], (1, -1, D))}
    _put(out, "pre_norm", sd, pre + "pre_layrnorm")
    out["patch_embed.proj.weight"] = sd[e + "patch_embedding.weight"]
    out["patch_embed.proj.bias"] = np.zeros((D,), np.float32)
    map_blocks(out, sd, CLIP_BLOCKS, cfg.num_hidden_layers, pre)
    _put(out, "norm", sd, pre + "post_layernorm")
    if no_head:
        _zero_head(out, D)
    elif "visual_projection.weight" not in sd:
        raise ValueError("the model has no visual_projection: convert a CLIPVisionModel with no_head=True (--no-head)")
    else:
        out["head.weight"] = sd["visual_projection.weight"]
        out["head.bias"] = np.zeros((int(np.shape(out["head.weight"])[0]),), np.float32)
    return _f32(out)


def dinov3_state_dict_to_timm(sd: Dict[str, np.ndarray], cfg, gated_mlp: bool = False) -> Dict[str, np.ndarray]:
    """An HF DINOv3ViTModel state dict (numpy arrays) under the file's names and order.  The position signal is rotary (include/vitx.h "rotary
    position embeddings"): `rope` = {1, rope_theta, 0, 0} in front, and a pos_embed [1][1 + g^2][D] of zeros at the config's image_size, so that the
    patch embedding and the resampler stay what they are.  register_tokens -> `reg_token`; LayerScale is folded; key_bias=False (the published
    models) becomes a zero k bias; mask_token is dropped.  The blocks live under `model.layer.N.` (transformers 5.15; `layer.N.` is accepted too).
    A plain MLP that is not 4 x hidden is refused.  A backbone: the zero head, whose VITX_FEAT_CLS is HF's pooler_output.
    use_gated_mlp (ViT-H+) is refused by name unless gated_mlp: then mlp.fc1 = cat(gate_proj, up_proj) ([2 F][D], F = intermediate_size),
    down_proj -> mlp.fc2 with LayerScale folded, zero biases where mlp_bias=False, and `glu` = {1, F, 0, 0} directly after `rope`.  The gate is
    silu: any other hidden_act of a gated model is refused."""
    gated = bool(getattr(cfg, "use_gated_mlp", False))
    if gated and not gated_mlp:
        raise ValueError("use_gated_mlp: the gated (SwiGLU) MLP of DINOv3 ViT-H+ / 7B is not converted by default; " + _GATED_HOWTO)
    if gated_mlp and not gated:
        raise ValueError("gated_mlp=True, but the model has the plain MLP (use_gated_mlp is off)")
    if gated and getattr(cfg, "hidden_act", "silu") != "silu":
        raise ValueError(f"hidden_act {getattr(cfg, 'hidden_act', None)!r}: the gate of a gated MLP is silu (SwiGLU); other gate functions are not supported")
    D = int(cfg.hidden_size)
    if not gated:
        _require_mlp_4x(cfg, "intermediate_size", 4 * D)
    if "embeddings.cls_token" not in sd:
        raise ValueError("not a DINOv3 state dict: embeddings.cls_token is missing")
    pre = next((p for p in ("model.", "") if p + "layer.0.attention.q_proj.weight" in sd), None)
    if pre is None:
        raise ValueError("not a DINOv3 state dict: layer.0.attention.q_proj.weight is missing")
    theta = np.float32(getattr(cfg, "rope_theta", 100.0))
    if not np.isfinite(theta) or not theta > 0:
        raise ValueError(f"rope_theta {theta}: it must be finite and positive")
    if (D // cfg.num_attention_heads) % 4:
        raise ValueError(f"head_dim {D // cfg.num_attention_heads}: rotary position embeddings need a multiple of 4")
    sd = dict(sd)
    for i in range(cfg.num_hidden_layers):                            # a projection without bias (key_bias=False) has a zero bias
        for n in DINOV3_BLOCKS.qkv:
            k = f"{pre}layer.{i}.{n}"
            if k + ".weight" in sd and k + ".bias" not in sd:
                sd[k + ".bias"] = np.zeros((int(np.shape(sd[k + ".weight"])[0]),), np.float32)
    if gated:
        for i in range(cfg.num_hidden_layers):                        # fc1 = gate rows, then up rows; a projection without bias (mlp_bias=False) has a zero bias
            q = f"{pre}layer.{i}.mlp."
            for n in ("gate_proj", "up_proj", "down_proj"):
                if q + n + ".bias" not in sd:
                    sd[q + n + ".bias"] = np.zeros((int(np.shape(sd[q + n + ".weight"])[0]),), np.float32)
            sd[q + "gate_up.weight"] = np.concatenate([sd[q + "gate_proj.weight"], sd[q + "up_proj.weight"]], 0)
            sd[q + "gate_up.bias"] = np.concatenate([sd[q + "gate_proj.bias"], sd[q + "up_proj.bias"]], 0)
    g = int(cfg.image_size) // int(cfg.patch_size)
    e = "embeddings."
    out = {"rope": np.array([1, theta, 0, 0], np.float32)}
    if gated:
        out["glu"] = _glu_tensor(int(np.shape(sd[f"{pre}layer.0.mlp.down_proj.weight"])[1]))
    out["cls_token"] = sd[e + "cls_token"]
    if e + "register_tokens" in sd and int(np.shape(sd[e + "register_tokens"])[1]) > 0:
        out["reg_token"] = sd[e + "register_tokens"]
    out["pos_embed"] = np.zeros((1, 1 + g * g, D), np.float32)
    _put(out, "patch_embed.proj", sd, e + "patch_embeddings")
    map_blocks(out, sd, DINOV3_GLU_BLOCKS if gated else DINOV3_BLOCKS, cfg.num_hidden_layers, pre)
    _put(out, "norm", sd, "norm")
    _zero_head(out, D)
    return _f32(out)


_POOL_ORDER = ("latent", "q.weight", "q.bias", "kv.weight", "kv.bias", "proj.weight", "proj.bias", "norm.weight", "norm.bias",
               "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


def siglip_state_dict_to_timm(sd: Dict[str, np.ndarray], cfg) -> Dict[str, np.ndarray]:
    """An HF SiglipVisionModel / SiglipModel state dict (numpy arrays) under the file's names and order.  There is NO class token:
    position_embedding [g^2][D] -> pos_embed [1][g^2][D]; post_layernorm -> norm; the multi-head attention-pooling head becomes the thirteen
    `attn_pool.*` tensors after norm.bias (include/vitx.h "no class token and the attention-pooling head", timm's AttentionPoolLatent names):
    head.probe -> latent, head.attention.in_proj_weight / in_proj_bias split into q (rows 0 .. D) and kv (rows D .. 3 D), out_proj -> proj,
    head.layernorm -> norm, head.mlp -> mlp.  A tower has no classifier: the file gets the zero head, and its pooled embedding -- SigLIP's
    pooler_output / image_embeds -- is read with --embed-kind cls / VITX_FEAT_CLS."""
    pre = next((p for p in ("vision_model.", "") if p + "embeddings.position_embedding.weight" in sd), None)
    if pre is None:
        raise ValueError("not a SigLIP vision state dict: embeddings.position_embedding.weight is missing")
    e, h = pre + "embeddings.", pre + "head."
    if e + "patch_embedding.weight" not in sd or np.ndim(sd[e + "patch_embedding.weight"]) != 4:
        raise ValueError("Siglip2VisionModel (NaFlex) is not supported: its patch embedding is a Linear over flattened patches, not a convolution")
    D = int(cfg.hidden_size)
    _require_mlp_4x(cfg, "intermediate_size", 4 * D, " (SO400M's 4304 is not supported)")
    if getattr(cfg, "vision_use_head", True) is False or h + "probe" not in sd:
        raise ValueError("vision_use_head = False: the tower has no attention-pooling head, and the file format has no slot for a SigLIP tower without it")
    out = {"pos_embed": np.reshape(sd[e + "position_embedding.weight"], (1, -1, D))}
    _put(out, "patch_embed.proj", sd, e + "patch_embedding")
    map_blocks(out, sd, CLIP_BLOCKS, cfg.num_hidden_layers, pre)
    _put(out, "norm", sd, pre + "post_layernorm")
    w, b = np.asarray(sd[h + "attention.in_proj_weight"]), np.asarray(sd[h + "attention.in_proj_bias"])
    if w.shape != (3 * D, D) or b.shape != (3 * D,):
        raise ValueError(f"head.attention.in_proj_weight {w.shape}: expected [{3 * D}][{D}]")
    out["attn_pool.latent"] = np.reshape(sd[h + "probe"], (1, 1, D))
    out["attn_pool.q.weight"] = w[:D]; out["attn_pool.q.bias"] = b[:D]
    out["attn_pool.kv.weight"] = w[D:]; out["attn_pool.kv.bias"] = b[D:]
    for dst, src in (("proj", "attention.out_proj"), ("norm", "layernorm"), ("mlp.fc1", "mlp.fc1"), ("mlp.fc2", "mlp.fc2")):
        _put(out, "attn_pool." + dst, sd, h + src)
    _zero_head(out, D)
    return _f32(out)


# --------------------------------------------------------------------------- text towers (include/vitx.h "the text tower")
# (tests/test_cpu_text.py reads the macro out of kernels.h and holds this tuple to it)
LN_WIDTHS = (64, 128, 192, 256, 384, 512, 768, 1024, 1280, 1536, 320, 448, 576, 640, 896, 1152, 1408, 1664, 2048)     # VITX_LN_WIDTHS (kernels.h)
TEXT_MAX_TOKENS = 128


def _text_prefix(sd) -> str:
    pre = next((p for p in ("text_model.", "") if p + "embeddings.token_embedding.weight" in sd), None)
    if pre is None:
        raise ValueError("not a text-tower state dict: embeddings.token_embedding.weight is missing")
    return pre


def _text_front(sd, cfg, pre: str) -> Dict[str, np.ndarray]:
    e = pre + "embeddings."
    D = int(cfg.hidden_size)
    _require_mlp_4x(cfg, "intermediate_size", 4 * D)
    out = {"token_embed.weight": sd[e + "token_embedding.weight"], "pos_embed": sd[e + "position_embedding.weight"]}
    map_blocks(out, sd, CLIP_BLOCKS, cfg.num_hidden_layers, pre)
    _put(out, "norm", sd, pre + "final_layer_norm")
    return out


def clip_text_state_dict(sd: Dict[str, np.ndarray], cfg, no_head: bool = False) -> Dict[str, np.ndarray]:
    """An HF CLIPTextModelWithProjection / CLIPModel state dict under a text file's names and order: token_embedding -> token_embed.weight [V][D],
    position_embedding -> pos_embed [T][D], the blocks through map_blocks, final_layer_norm -> norm, the bias-free text_projection [E][D] ->
    head.weight with a zero head.bias."""
    out = _text_front(sd, cfg, _text_prefix(sd))
    if "text_projection.weight" not in sd:
        raise ValueError("the model has no text_projection: a text file holds the projected tower (CLIPTextModelWithProjection or CLIPModel)")
    out["head.weight"] = sd["text_projection.weight"]
    out["head.bias"] = np.zeros((int(np.shape(out["head.weight"])[0]),), np.float32)
    return _f32(out)


def siglip_text_state_dict(sd: Dict[str, np.ndarray], cfg, no_head: bool = False) -> Dict[str, np.ndarray]:
    """An HF SiglipTextModel / SiglipModel state dict under a text file's names and order; the tower's own `head` (a Linear with bias) is the projection."""
    pre = _text_prefix(sd)
    out = _text_front(sd, cfg, pre)
    _put(out, "head", sd, pre + "head")
    return _f32(out)


# --------------------------------------------------------------------------- one write path for every HuggingFace family
def _config_labels(cfg, num_classes: int):
    return {int(k): str(v) for k, v in (getattr(cfg, "id2label", None) or {}).items()} or None


# name: as the refusals call the family; mapper(sd, cfg, no_head) -> the file's tensors; prefix_rows: rows of pos_embed in front of the patch grid;
# labels(cfg, num_classes) -> id2label of a model converted with its head; head: "always" -- no_head is refused --, "optional" -- no_head converts a
# model without classifier / projection -- or "never" -- the family has no classifier, no_head is accepted and not required; loaders: the
# transformers classes main() loads a checkpoint with, (with its head, with --no-head).
Family = namedtuple("Family", "name mapper prefix_rows labels head loaders")


_VIT = Family("ViT", lambda sd, cfg, no_head: state_dict_to_timm(sd, cfg.num_hidden_layers), 1, _config_labels, "always", ("ViTForImageClassification",) * 2)
_DINOV2 = Family("DINOv2", dinov2_state_dict_to_timm, 1, _config_labels, "optional", ("AutoModelForImageClassification", "AutoModel"))
_CLIP = Family("CLIP", clip_state_dict_to_timm, 1, lambda cfg, E: {i: f"dim_{i}" for i in range(E)}, "optional", ("CLIPVisionModelWithProjection", "CLIPVisionModel"))
_SIGLIP = Family("SigLIP", lambda sd, cfg, no_head: siglip_state_dict_to_timm(sd, cfg), 0, None, "never", ("SiglipVisionModel",) * 2)
_DINOV3 = Family("DINOv3", lambda sd, cfg, no_head, gated_mlp=False: dinov3_state_dict_to_timm(sd, cfg, gated_mlp), 1, None, "never", ("DINOv3ViTModel",) * 2)
# text towers (convert_hf_text_model): no patch grid (prefix_rows is not read), no labels -- the "classes" are the projection's columns --, always with the projection
_CLIP_TEXT = Family("CLIP text", clip_text_state_dict, 0, lambda cfg, E: {}, "always", ("CLIPTextModelWithProjection",) * 2)
_SIGLIP_TEXT = Family("SigLIP text", siglip_text_state_dict, 0, lambda cfg, E: {}, "always", ("SiglipTextModel",) * 2)
_TWO_TOWERS = ("clip", "siglip")          # converted as their vision tower (config.vision_config); convert_hf_text_model takes config.text_config
# by model_type, the vision tower's or, for main(), the checkpoint's; any other model_type is taken for a ViT
FAMILIES = {"vit": _VIT, "dinov2": _DINOV2, "dinov2_with_registers": _DINOV2, "clip_vision_model": _CLIP, "clip": _CLIP, "siglip_vision_model": _SIGLIP, "siglip": _SIGLIP,
            "dinov3_vit": _DINOV3, "clip_text_model": _CLIP_TEXT, "siglip_text_model": _SIGLIP_TEXT}


def _family_tensors(model, cfg, fam, no_head: bool, head_dim_note: str = "", gated_mlp: bool = False):
    """The front both converters share: the head-dim refusal, the state dict as numpy arrays, the config's activation and epsilon, and the
    family's mapper.  Returns (the file's tensors in its order, activation, eps); each converter then states its header and calls write_model."""
    hd = cfg.hidden_size // cfg.num_attention_heads
    if cfg.hidden_size % cfg.num_attention_heads or hd % 8 or not 8 <= hd <= 128:
        raise ValueError(f"head_dim {hd}: the forward path takes multiples of 8 up to 128{head_dim_note}")
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    if gated_mlp and fam not in (_DINOV2, _DINOV3):
        raise ValueError(f"gated_mlp=True: a {fam.name} model has no gated MLP this converter knows (DINOv2 use_swiglu_ffn, DINOv3 use_gated_mlp)")
    tensors = fam.mapper(sd, cfg, no_head, gated_mlp=True) if gated_mlp else fam.mapper(sd, cfg, no_head)
    # a gated DINOv3 model states its GATE function in hidden_act (silu, checked by the mapper): the file's activation slot is carried and not
    # applied in such a file (include/vitx.h "gated MLP") and says tanh-GELU, the slot's zero
    act = ACT_TANH if "glu" in tensors and fam is _DINOV3 else hf_activation(cfg)
    return tensors, act, float(getattr(cfg, "layer_norm_eps", 1e-6))


def convert_hf_model(model, path: str, ftype: int = 1, vitstr: bool = False, no_head: bool = False, preprocessor_config: dict | None = None,
                     gated_mlp: bool = False) -> HParams:
    """model: a transformers model of one of FAMILIES, in eval mode (the module docstring lists the classes); no_head=True converts a model
    without classifier or projection, whose file gets the zero head labelled "(no head)" (a SigLIP tower always does).  The activation and the
    LayerNorm epsilon are the config's (with_arch); the class count and the image size are read off head.weight and pos_embed.
    preprocessor_config: the checkpoint's preprocessor_config.json as a dict -- its preprocessing is written as the `preproc` tensor (hf_preproc);
    None writes the file without one.  Writes `path`; returns the hparams written.
    gated_mlp=True opts in to the gated (SwiGLU) MLP of a Dinov2* model with use_swiglu_ffn or a DINOv3ViTModel with use_gated_mlp: the file carries
    the `glu` tensor, which neither the reference nor an engine build before it can read; without it such a model is refused by name.
    vitstr=True: the model is a ViTSTR scene-text recogniser (the reference's extensions/vitstr.cpp/convert-pth-to-ggml.py: a ViT with ONE input
    channel whose classifier is applied to the first 25 tokens); the file then carries the character set as labels, and the one-channel patch
    kernel is what makes vit_model_load / vitx_model_load treat it as a ViTSTR model (vitstr.cpp:482)."""
    cfg = model.config
    cls_name = type(model).__name__
    if cls_name.startswith("Siglip2") or getattr(cfg, "model_type", "").startswith("siglip2"):
        raise ValueError(f"{cls_name} (Siglip2VisionModel, NaFlex) is not supported: its patch embedding is a Linear over flattened patches")
    if cls_name == "SiglipForImageClassification":
        raise ValueError("SiglipForImageClassification is not supported: it classifies the mean of the patch tokens and has no attention-pooling head (no slot for it)")
    if getattr(cfg, "model_type", "") in _TWO_TOWERS:
        cfg = cfg.vision_config
    fam = FAMILIES.get(getattr(cfg, "model_type", ""), _VIT)
    if fam in (_CLIP_TEXT, _SIGLIP_TEXT):
        raise ValueError(f"{cls_name} is a text tower: convert it with convert_hf_text_model (--text-out)")
    if vitstr and preprocessor_config is not None:
        raise ValueError("a ViTSTR model's preprocessing is fixed: convert it without a preprocessor_config")
    if vitstr and getattr(cfg, "num_channels", 3) != 1:
        raise ValueError("a ViTSTR model takes one (grey) input channel")
    if vitstr and fam.name != "ViT":
        raise ValueError(f"a {fam.name} model is not a ViTSTR model")
    if no_head and fam.head == "always":
        raise ValueError("no_head converts a DINOv2 backbone (Dinov2Model, Dinov2WithRegistersModel), a CLIPVisionModel or a SigLIP tower")
    headless = fam.head == "never" or no_head
    tensors, act, eps = _family_tensors(model, cfg, fam, no_head, " (64 runs the tuned attention kernels)", gated_mlp)
    g = grid_side(tensors["pos_embed"], fam.prefix_rows)          # the checkpoint's own grid (config.image_size states it too)
    hp = HParams(cfg.hidden_size, cfg.num_hidden_layers, cfg.num_attention_heads, int(tensors["head.weight"].shape[0]), cfg.patch_size, g * cfg.patch_size, ftype)
    id2label = NO_HEAD_LABELS if headless else fam.labels(cfg, hp.num_classes)
    if vitstr:
        from .synth import VITSTR_LABELS
        if hp.num_classes != len(VITSTR_LABELS):
            raise ValueError(f"ViTSTR's character set has {len(VITSTR_LABELS)} classes ([GO], [s], 94 printable characters), the model has {hp.num_classes}")
        id2label = dict(VITSTR_LABELS)
    write_model(path, hp, with_arch(tensors, act, eps), id2label=id2label, ftype=ftype,
                preproc=hf_preproc(preprocessor_config, hp.img_size) if preprocessor_config is not None else None)
    return hp


def convert_hf_text_model(model, path: str, ftype: int = 1) -> HParams:
    """The text tower of a transformers CLIPTextModelWithProjection, CLIPModel, SiglipTextModel or SiglipModel as a text-tower file (include/vitx.h
    "the text tower"): header hidden D, layers L, heads H, num_classes = E (the projected width), patch_size = 0 (the mark of a text file),
    img_size = T (max_position_embeddings); tensors token_embed.weight, pos_embed, blocks.*, norm.*, head.*, and always
    `arch` = {activation, eps, causal, eos + 1}: causal 1 for CLIP, 0 for SigLIP; SigLIP pools the last position (slot 3 = 0), CLIP pools as
    transformers does today: the FIRST position whose id equals config.eos_token_id.  Legacy CLIP configs (eos_token_id == 2) pool at
    argmax(ids) instead; for those the file names eos = vocab_size - 1, the id for which both rules agree on tokenised input (CLIP's tokenizer
    gives <|endoftext|> the highest id, and pads with it).  A two-tower model also writes `zs` = {kind, exp(logit_scale), logit_bias, 0}.
    The token table is never block-quantised (ggml_file.write_model).  Writes `path`; returns the hparams written."""
    cfg = model.config
    mt = getattr(cfg, "model_type", "")
    zs = None
    if mt in _TWO_TOWERS:
        sd_all = model.state_dict()
        scale = float(np.exp(np.float64(sd_all["logit_scale"].detach().double().reshape(-1)[0].item())))
        bias = float(sd_all["logit_bias"].detach().double().reshape(-1)[0].item()) if mt == "siglip" else 0.0
        zs = np.array([ZS_SIGMOID if mt == "siglip" else ZS_SOFTMAX, scale, bias, 0.0], np.float32)
        cfg = cfg.text_config
    fam = FAMILIES.get(getattr(cfg, "model_type", ""))
    if fam not in (_CLIP_TEXT, _SIGLIP_TEXT):
        raise ValueError(f"convert_hf_text_model: model_type '{getattr(cfg, 'model_type', '')}' is no CLIP or SigLIP text tower")
    D, T = int(cfg.hidden_size), int(cfg.max_position_embeddings)
    if D not in LN_WIDTHS:
        raise ValueError(f"hidden_size {D} has no LayerNorm instantiation ({', '.join(str(w) for w in sorted(LN_WIDTHS))})")
    if not 1 <= T <= TEXT_MAX_TOKENS:
        raise ValueError(f"max_position_embeddings {T}: the text attention takes 1 .. {TEXT_MAX_TOKENS} tokens")
    tensors, act, eps = _family_tensors(model, cfg, fam, False)
    V, E = int(tensors["token_embed.weight"].shape[0]), int(tensors["head.weight"].shape[0])
    if tuple(tensors["pos_embed"].shape) != (T, D):
        raise ValueError(f"position_embedding {tuple(tensors['pos_embed'].shape)}: expected [{T}][{D}]")
    if fam is _CLIP_TEXT:
        eos = int(getattr(cfg, "eos_token_id", 2))
        if eos == 2:
            eos = V - 1
        if not 0 <= eos < V:
            raise ValueError(f"eos_token_id {eos} is outside the vocabulary of {V}")
        causal, slot = 1, eos + 1
    else:
        causal, slot = 0, 0
    out = {"arch": np.array([act, np.float32(eps), causal, slot], np.float32)}
    if zs is not None:
        out["zs"] = zs
    out.update(tensors)
    hp = HParams(D, cfg.num_hidden_layers, cfg.num_attention_heads, E, 0, T, ftype)
    write_model(path, hp, out, id2label=fam.labels(cfg, E), ftype=ftype)
    return hp


# --------------------------------------------------------------------------- timm state dicts
_TIMM_UNSUPPORTED = {"fc_norm.": "fc_norm", "dist_token": "a distillation token", "head_dist.": "a distillation head", ".q_norm.": "qk-norm", ".k_norm.": "qk-norm",
                     "attn_pool.pos_embed": "a position embedding inside the attention pooling"}
# The head count is NOT in a state_dict (the reference reads timm's module attribute): it is inferred only for the widths of timm's released ViTs,
# where it is unambiguous; any other width needs --heads (D // 64 would turn ViT-H/14's 16 heads of 80 into 20 heads of 64 -- a file that loads,
# runs and is wrong).
_TIMM_HEADS = {192: 3, 384: 6, 768: 12, 1024: 16, 1280: 16, 1152: 16, 1408: 16, 1664: 16}      # tiny, small, base, large, huge, so400m, giant, gigantic


def _placed_after(t: dict, anchor: str, names) -> dict:
    """`t` with the tensors `names`, in that order, directly after `anchor`; every other tensor keeps its place."""
    moved = {k: t[k] for k in names}
    out = {}
    for k, v in t.items():
        if k not in moved:
            out[k] = v
        if k == anchor:
            out.update(moved)
    return out


def convert_timm_state_dict(sd, path: str, ftype: int = 1, heads: int = 0, id2label=None, act: str = "tanh", eps: float = 1e-6, preproc: dict | None = None) -> HParams:
    """sd: a timm VisionTransformer state_dict (name -> array / tensor), e.g. torch.load("vit_base_patch16_224.pth").  It already carries the names
    the file uses -- the reference's convert-pth-to-ggml.py:96-158 writes `timm_model.state_dict()` verbatim -- so no `timm` is needed: hidden
    size, depth, classes, patch and image size come from the tensor shapes (the reference reads them off the timm module), `norm_pre.*` is skipped
    exactly as there (:117-120), the ViTSTR extension's checkpoints lose their "module.vitstr." prefix (extensions/vitstr.cpp/convert-pth-to-ggml.py:
    226-229) and are recognised by their one-channel patch kernel.  The tensors keep the state dict's own order, apart from two placements: reg_token
    goes directly after cls_token, and `attn_pool.*`, in the file's order, then head.* go behind everything else.
    DINOv2-class checkpoints are taken: `blocks.N.ls1.gamma` / `ls2.gamma` (LayerScale) are folded into attn.proj / mlp.fc2 in f32, and a `pos_embed`
    of g^2 rows beside `reg_token` (timm's no_embed_class layout of the reg4 DINOv2 models: the class token gets no position term there) gets a zero
    row in front, which is exact.  `attn_pool.*` (AttentionPoolLatent: SigLIP) is taken, without cls_token only, as the file's attention-pooling
    head; a checkpoint without head.* (num_classes 0) gets the zero head.  Tensors the file has no slot for (_TIMM_UNSUPPORTED) are refused by name.
    A state dict carries no config: `act` ("tanh", "erf", "quick") and `eps` state the model's activation and LayerNorm epsilon.  The default
    (tanh, 1e-6) writes the reference's file, without `arch`; timm's VisionTransformer was trained with nn.GELU and wants act="erf" (its eps is 1e-6).
    preproc: the keyword arguments of cli_preproc (resize, crop, filt, mean, std, crop_round) -- the checkpoint's preprocessing, written as the
    `preproc` tensor; None or all unset: no tensor."""
    if act not in _ACT_NAMES:
        raise ValueError(f"act {act!r}: one of {sorted(_ACT_NAMES)}")
    if isinstance(sd, dict) and "model" in sd and not hasattr(sd["model"], "shape"):
        sd = sd["model"]
    t = {k.replace("module.vitstr.", ""): v for k, v in sd.items()}
    t = {k: v for k, v in t.items() if not k.startswith("norm_pre")}
    for k in t:
        for u, what in _TIMM_UNSUPPORTED.items():
            if u in k:
                raise ValueError(f"tensor {k!r}: {what} is not supported (the file format has no slot for it)")
    t = _f32(t)
    map_head = any(k.startswith("attn_pool.") for k in t)
    if map_head:
        if "cls_token" in t or "reg_token" in t:
            raise ValueError("attn_pool.* beside cls_token / reg_token: the attention-pooling head is taken only from a model without a class token")
        pool = [f"attn_pool.{n}" for n in _POOL_ORDER]
        missing = [k for k in pool if k not in t]
        extra = [k for k in t if k.startswith("attn_pool.") and k not in pool]
        if missing or extra:
            raise ValueError(f"the attention-pooling head is not the thirteen tensors the file holds: missing {missing}, unknown {extra}")
        D = int(t["pos_embed"].shape[-1]) if "pos_embed" in t else 0
        if "head.weight" not in t:                        # num_classes 0
            _zero_head(t, D)
            id2label = id2label if id2label is not None else NO_HEAD_LABELS
        t["attn_pool.latent"] = t["attn_pool.latent"].reshape(1, 1, D)
    for need in ("cls_token", "pos_embed", "patch_embed.proj.weight", "patch_embed.proj.bias", "norm.weight", "norm.bias", "head.weight", "head.bias"):
        if need not in t and not (map_head and need == "cls_token"):
            raise ValueError(f"not a timm VisionTransformer state_dict: {need!r} is missing")
    D = int(t["pos_embed"].shape[-1] if map_head else t["cls_token"].shape[-1])
    L = 1 + max(int(k.split(".")[1]) for k in t if k.startswith("blocks."))
    # LayerScale: folded, no file slot.  A model has it on both branches of every block or not at all: a partial set is a damaged checkpoint
    ls_keys = [f"blocks.{i}.{ls}.gamma" for i in range(L) for ls in ("ls1", "ls2")]
    ls_have = [k for k in ls_keys if k in t]
    if ls_have and len(ls_have) != len(ls_keys):
        raise ValueError(f"LayerScale is incomplete: {ls_have[0]!r} is present, {next(k for k in ls_keys if k not in t)!r} is missing")
    for gk in ls_have:
        p = gk.replace(".ls1.gamma", ".attn.proj.").replace(".ls2.gamma", ".mlp.fc2.")
        t[p + "weight"], t[p + "bias"] = fold_layer_scale(t[p + "weight"], t[p + "bias"], t.pop(gk))
    if "reg_token" in t:
        n_rows = int(t["pos_embed"].shape[1])
        if int(round(n_rows ** 0.5)) ** 2 == n_rows and n_rows > 1:       # no_embed_class: g^2 rows, none for the class token
            t["pos_embed"] = np.ascontiguousarray(np.concatenate([np.zeros((1, 1, D), np.float32), t["pos_embed"]], axis=1))
        t = _placed_after(t, "cls_token", ["reg_token"])
    if map_head:
        last = [k for k in t if not k.startswith(("attn_pool.", "head."))][-1]
        t = _placed_after(t, last, pool + [k for k in t if k.startswith("head.")])
    Dw, cin, P, P2 = t["patch_embed.proj.weight"].shape
    g = grid_side(t["pos_embed"], 0 if map_head else 1)
    if Dw != D or P != P2 or cin not in (1, 3):
        raise ValueError(f"unexpected shapes: patch kernel {t['patch_embed.proj.weight'].shape}, pos_embed {t['pos_embed'].shape}")
    H = heads or _TIMM_HEADS.get(D, 0)
    if H <= 0:
        raise ValueError(f"hidden size {D} is not a released timm ViT width ({sorted(_TIMM_HEADS)}): pass the head count (--heads)")
    if D % H or (D // H) % 8 or not 8 <= D // H <= 128:
        raise ValueError(f"head_dim {D // H if H and D % H == 0 else '?'}: the forward path takes multiples of 8 up to 128 (pass --heads for a model whose head_dim is not 64)")
    hp = HParams(D, L, H, int(t["head.weight"].shape[0]), int(P), g * int(P), ftype)
    if cin == 1 and id2label is None:
        from .synth import VITSTR_LABELS
        if hp.num_classes == len(VITSTR_LABELS):
            id2label = dict(VITSTR_LABELS)
    # pos_embed, the patch kernel and bias, 12 per block, norm.* and head.*; the class token (+ registers) or the thirteen of the pooling head
    expected = 3 + 12 * L + 4 + (len(_POOL_ORDER) if map_head else 1 + ("reg_token" in t))
    if len(t) != expected:
        raise ValueError(f"{len(t)} tensors after filtering, the file format holds exactly {expected} for {L} layers (vit.cpp:512-574)")
    slots = cli_preproc(hp.img_size, **preproc) if preproc else None
    if cin == 1 and slots is not None:
        raise ValueError("a ViTSTR model's preprocessing is fixed: the --pp-* options do not apply")
    write_model(path, hp, with_arch(t, _ACT_NAMES[act], eps), id2label=id2label, ftype=ftype, preproc=slots)
    return hp


# --------------------------------------------------------------------------- zero-shot banks
def _l2_rows(x: np.ndarray) -> np.ndarray:
    return x / np.sqrt((x * x).sum(axis=1, keepdims=True))


def zeroshot_bank(model, input_ids, attention_mask=None, groups=None):
    """The zero-shot bank of a transformers CLIPModel / SiglipModel: (embeds [K][E] float64, kind, scale, bias).

    Row p of `input_ids` [P][T] is one tokenised prompt; its text embedding (the text tower's pooled, projected output) is L2-normalised.
    groups = None: K = P, class k is prompt k.  groups [P] of class ids 0 .. K-1: the normalised rows of each class are averaged and the mean is
    normalised again (prompt ensembling; every class needs at least one prompt).  kind = ZS_SOFTMAX for CLIP, ZS_SIGMOID for SigLIP;
    scale = exp(logit_scale), bias = logit_bias (0 for CLIP): logits_per_image = scale * image_embeds . embeds^T + bias.
    The arithmetic past the text tower is float64 whatever the model's dtype."""
    import torch
    mt = getattr(model.config, "model_type", "")
    if mt not in ("clip", "siglip"):
        raise ValueError(f"zeroshot_bank: a CLIPModel or a SiglipModel is needed (both towers and logit_scale), not model_type '{mt}'")
    ids = torch.as_tensor(np.asarray(input_ids), dtype=torch.long)
    if ids.ndim != 2:
        raise ValueError("zeroshot_bank: input_ids must be [prompts][tokens]")
    kw = {} if attention_mask is None else {"attention_mask": torch.as_tensor(np.asarray(attention_mask), dtype=torch.long)}
    with torch.no_grad():
        f = model.get_text_features(input_ids=ids, **kw)
    if not torch.is_tensor(f):             # transformers 5.x returns the tower's output object: pooler_output holds the projected features
        f = f.pooler_output
    e = _l2_rows(f.detach().to(torch.float64).cpu().numpy())
    if groups is not None:
        g = np.asarray(groups, dtype=np.int64)
        if g.shape != (e.shape[0],) or g.min() < 0:
            raise ValueError("zeroshot_bank: groups must give one class id >= 0 per prompt")
        K = int(g.max()) + 1
        counts = np.bincount(g, minlength=K)
        if (counts == 0).any():
            raise ValueError(f"zeroshot_bank: class {int(np.flatnonzero(counts == 0)[0])} has no prompt")
        mean = np.zeros((K, e.shape[1]), np.float64)
        np.add.at(mean, g, e)
        e = _l2_rows(mean / counts[:, None])
    scale = float(np.exp(np.float64(model.logit_scale.detach().to(torch.float64).reshape(-1)[0].item())))
    bias = float(model.logit_bias.detach().to(torch.float64).reshape(-1)[0].item()) if mt == "siglip" else 0.0
    return e, (ZS_SIGMOID if mt == "siglip" else ZS_SOFTMAX), scale, bias


def save_bank(path: str, embeds, kind: int, scale: float, bias: float, labels=None) -> None:
    """The bank file: an .npz with embeds [K][E] f32, labels [K] (class_<k> where none are given), kind, scale, bias."""
    e = np.asarray(embeds, np.float32)
    lab = [f"class_{k}" for k in range(e.shape[0])] if labels is None else [str(l) for l in labels]
    if e.ndim != 2 or len(lab) != e.shape[0]:
        raise ValueError(f"save_bank: {len(lab)} labels for embeds of shape {e.shape}")
    with open(path, "wb") as f:            # (np.savez on a name would append .npz)
        np.savez(f, embeds=e, labels=np.asarray(lab, dtype=np.str_), kind=np.int32(kind), scale=np.float32(scale), bias=np.float32(bias))


def load_bank(path: str) -> dict:
    """-> {"embeds" [K][E] f32, "labels" list of K str, "kind" int, "scale" float, "bias" float}; ValueError for a file that is not a bank."""
    with np.load(path, allow_pickle=False) as z:
        missing = [k for k in ("embeds", "labels", "kind", "scale", "bias") if k not in z.files]
        if missing:
            raise ValueError(f"load_bank: '{path}' lacks {', '.join(missing)}")
        b = dict(embeds=np.ascontiguousarray(z["embeds"], np.float32), labels=[str(l) for l in z["labels"]], kind=int(z["kind"]),
                 scale=float(z["scale"]), bias=float(z["bias"]))
    if b["embeds"].ndim != 2 or len(b["labels"]) != b["embeds"].shape[0] or b["kind"] not in (ZS_SOFTMAX, ZS_SIGMOID):
        raise ValueError(f"load_bank: '{path}' is not a consistent bank (embeds {b['embeds'].shape}, {len(b['labels'])} labels, kind {b['kind']})")
    return b


def _main_bank(a, transformers, model_type: str) -> None:
    """--zero-shot-out: the bank of the checkpoint's text tower, from token ids or from prompts."""
    both = (transformers.CLIPModel if model_type == "clip" else transformers.SiglipModel).from_pretrained(a.model).eval()
    mask = None
    if a.zero_shot_ids:
        ids = np.load(a.zero_shot_ids)
        mask_path = a.zero_shot_ids[:-4] + ".mask.npy" if a.zero_shot_ids.endswith(".npy") else a.zero_shot_ids + ".mask.npy"
        if os.path.isfile(mask_path):
            mask = np.load(mask_path)
        labels = None
    else:
        with open(a.zero_shot_prompts) as f:
            labels = [l.rstrip("\n") for l in f if l.strip()]
        tok = transformers.AutoTokenizer.from_pretrained(a.model)(labels, padding="max_length", truncation=True, return_tensors="np")
        ids = tok["input_ids"]
        mask = tok.get("attention_mask") if model_type == "clip" else None        # SigLIP was trained without a mask
    if a.zero_shot_labels:
        with open(a.zero_shot_labels) as f:
            labels = [l.rstrip("\n") for l in f if l.strip()]
    embeds, kind, scale, bias = zeroshot_bank(both, ids, mask)
    save_bank(a.zero_shot_out, embeds, kind, scale, bias, labels)
    print(f"wrote {a.zero_shot_out}: {embeds.shape[0]} classes of width {embeds.shape[1]}, {'sigmoid' if kind == ZS_SIGMOID else 'softmax'}, scale {scale:.6g}, bias {bias:.6g}")


# ---- dense heads (include/vitx.h "dense prediction"): an mmseg BNHead state dict -> the .npz binding.dense_head reads -----------------------
_BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def dense_head(state_dict, layers, hidden_size=None, eps=1e-5, names=None):
    """The linear segmentation head of an mmseg BNHead checkpoint (the form DINOv2's linear heads are published in) as {"weight" [K, Dc] f32, "bias"
    [K] f32, "layers", "names"}: decode_head.conv_seg.weight [K, Dc, 1, 1] and .bias [K], with the evaluation-mode SyncBN decode_head.bn.* in front of
    the convolution folded in, in float64:  g = gamma / sqrt(var + eps);  W' = W diag(g);  b' = b + W (beta - mean g).  A plain weight [K, Dc] / bias
    [K] pair is taken as it is.  `layers`: the backbone layers (indices, ascending) whose tokens the head was trained on, Dc = len(layers) * D;
    hidden_size, when given, is the backbone's D and a head of another width is refused by name.  No mmseg import, no download."""
    sd = state_dict.get("state_dict", state_dict)
    get = lambda k: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], np.float64)
    layers = [int(l) for l in layers]
    if not layers or len(layers) > 4 or sorted(set(layers)) != layers or layers[0] < 0:
        raise ValueError(f"dense_head: layers {layers} must be 1 to 4 ascending, distinct layer indices")
    if "decode_head.conv_seg.weight" in sd:
        wkey, bkey = "decode_head.conv_seg.weight", "decode_head.conv_seg.bias"
    elif "weight" in sd and "bias" in sd:
        wkey, bkey = "weight", "bias"
    else:
        raise ValueError("dense_head: neither decode_head.conv_seg.weight nor a plain weight / bias pair in the state dict")
    W, b = get(wkey), get(bkey)
    if W.ndim == 4 and W.shape[2:] == (1, 1):
        W = W[:, :, 0, 0]
    if W.ndim != 2 or b.shape != (W.shape[0],):
        raise ValueError(f"dense_head: {wkey} {tuple(get(wkey).shape)} is not [K, Dc, 1, 1] or [K, Dc] with {bkey} [K]")
    K, Dc = W.shape
    if hidden_size is not None and Dc != len(layers) * int(hidden_size):
        raise ValueError(f"dense_head: {wkey} has width {Dc}, the backbone gives {len(layers)} layers x hidden size {int(hidden_size)} = {len(layers) * int(hidden_size)}")
    if Dc % len(layers):
        raise ValueError(f"dense_head: {wkey} has width {Dc}, not a multiple of the {len(layers)} layers")
    if wkey.startswith("decode_head") and all(f"decode_head.bn.{k}" in sd for k in _BN_KEYS):
        gamma, beta, mean, var = (get(f"decode_head.bn.{k}") for k in _BN_KEYS)
        for k, v in zip(_BN_KEYS, (gamma, beta, mean, var)):
            if v.shape != (Dc,):
                raise ValueError(f"dense_head: decode_head.bn.{k} {tuple(v.shape)} does not match the head's width {Dc}")
        g = gamma / np.sqrt(var + float(eps))
        b = b + W @ (beta - mean * g)
        W = W * g[None, :]
    if not (np.isfinite(W).all() and np.isfinite(b).all()):
        raise ValueError("dense_head: the folded head is not finite")
    if names is not None and len(names) != K:
        raise ValueError(f"dense_head: {len(names)} names for {K} classes")
    return {"weight": W.astype(np.float32), "bias": b.astype(np.float32), "layers": layers, "names": None if names is None else [str(s) for s in names]}


def write_dense_head(path, head) -> None:
    """The .npz binding.dense_head reads: weight, bias, layers and -- when the head has them -- names (a unicode array: no pickle)."""
    arrays = dict(weight=np.asarray(head["weight"], np.float32), bias=np.asarray(head["bias"], np.float32), layers=np.asarray(head["layers"], np.int32))
    if head.get("names"):
        arrays["names"] = np.asarray(head["names"], dtype=np.str_)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def _main_dense_head(argv) -> int:
    ap = argparse.ArgumentParser(description="an mmseg BNHead checkpoint (.pth) -> a dense head file (.npz) for vit_cli.py --dense-head")
    ap.add_argument("--dense-head-in", required=True, metavar="CKPT.pth", help="torch-saved state dict with decode_head.conv_seg.* (and decode_head.bn.*), or a plain weight / bias pair")
    ap.add_argument("--dense-head-out", required=True, metavar="HEAD.npz")
    ap.add_argument("--dense-layers", required=True, metavar="L1,L2,..", help="the backbone layers (0-based, ascending) whose tokens the head reads, e.g. 8,9,10,11")
    ap.add_argument("--dense-hidden", type=int, default=0, metavar="D", help="the backbone's hidden size: a head of another width is refused")
    ap.add_argument("--dense-eps", type=float, default=1e-5, help="epsilon of the head's BatchNorm (default 1e-5, torch's)")
    ap.add_argument("--dense-names", default=None, metavar="NAMES.txt", help="one class name per line")
    a = ap.parse_args(argv)
    import torch
    sd = torch.load(a.dense_head_in, map_location="cpu", weights_only=True)
    names = [l.rstrip("\n") for l in open(a.dense_names)] if a.dense_names else None
    head = dense_head(sd, [int(x) for x in a.dense_layers.split(",")], a.dense_hidden or None, a.dense_eps, names)
    write_dense_head(a.dense_head_out, head)
    print(f"wrote {a.dense_head_out}: {head['weight'].shape[0]} classes, width {head['weight'].shape[1]}, layers {head['layers']}")
    return 0


# ---- depth heads (include/vitx.h "depth estimation"): an mmseg-style binned depth head's state dict -> the .npz binding.depth_head reads ------
def depth_head(state_dict, layers, hidden_size, min_depth=0.001, max_depth=10.0, bins="UD", upsample=4, norm=False):
    """The binned linear depth head of a DINOv2-style depther checkpoint as {"wp" [K, m D], "wc" [K, m D] or None, "bias" [K], "bins" [K], "layers",
    "upsample", "min_depth", "max_depth", "norm"}: decode_head.conv_depth.weight [K, 2 m D, 1, 1] (or [K, 2 m D]) and .bias [K].  Per layer the D patch
    columns come first, then the D class columns (the class token is concatenated to every patch token); they are split into wp and wc.  A width of
    m D is a head without a class half (wc None); any other width is refused by name.  bins: "UD" / "SID" centres between min_depth and max_depth."""
    from . import binding
    sd = state_dict.get("state_dict", state_dict)
    get = lambda k: np.asarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], np.float64)
    layers = [int(l) for l in layers]
    if not layers or len(layers) > 4 or sorted(set(layers)) != layers or layers[0] < 0:
        raise ValueError(f"depth_head: layers {layers} must be 1 to 4 ascending, distinct layer indices")
    wkey, bkey = "decode_head.conv_depth.weight", "decode_head.conv_depth.bias"
    if wkey not in sd or bkey not in sd:
        raise ValueError(f"depth_head: no {wkey} / {bkey} in the state dict")
    W, b = get(wkey), get(bkey)
    if W.ndim == 4 and W.shape[2:] == (1, 1):
        W = W[:, :, 0, 0]
    if W.ndim != 2 or b.shape != (W.shape[0],):
        raise ValueError(f"depth_head: {wkey} {tuple(get(wkey).shape)} is not [K, C, 1, 1] or [K, C] with {bkey} [K]")
    K, width = W.shape
    m, D = len(layers), int(hidden_size)
    if width == 2 * m * D:
        blocks = W.reshape(K, m, 2, D)
        wp, wc = blocks[:, :, 0, :].reshape(K, m * D), blocks[:, :, 1, :].reshape(K, m * D)
    elif width == m * D:
        wp, wc = W, None
    else:
        raise ValueError(f"depth_head: {wkey} has width {width}, the backbone gives {m} layers x hidden size {D}: {2 * m * D} with the class token, {m * D} without")
    if not (np.isfinite(W).all() and np.isfinite(b).all()):
        raise ValueError("depth_head: the head is not finite")
    if int(upsample) not in (1, 2, 4):
        raise ValueError(f"depth_head: upsample {upsample} is not 1, 2 or 4")
    return {"wp": np.ascontiguousarray(wp, np.float32), "wc": None if wc is None else np.ascontiguousarray(wc, np.float32), "bias": b.astype(np.float32),
            "bins": binding.depth_bins(K, float(min_depth), float(max_depth), bins), "layers": layers, "upsample": int(upsample),
            "min_depth": float(min_depth), "max_depth": float(max_depth), "norm": bool(norm)}


def write_depth_head(path, head) -> None:
    """The .npz binding.depth_head reads."""
    arrays = dict(wp=np.asarray(head["wp"], np.float32), bias=np.asarray(head["bias"], np.float32), bins=np.asarray(head["bins"], np.float32),
                  layers=np.asarray(head["layers"], np.int32), upsample=np.int32(head["upsample"]), min_depth=np.float64(head["min_depth"]),
                  max_depth=np.float64(head["max_depth"]), norm=np.bool_(head["norm"]))
    if head.get("wc") is not None:
        arrays["wc"] = np.asarray(head["wc"], np.float32)
    with open(path, "wb") as f:
        np.savez(f, **arrays)


def _main_depth_head(argv) -> int:
    ap = argparse.ArgumentParser(description="a binned linear depth head checkpoint (.pth) -> a depth head file (.npz) for vit_cli.py --depth-head")
    ap.add_argument("--depth-head-in", required=True, metavar="CKPT.pth", help="torch-saved state dict with decode_head.conv_depth.weight / .bias")
    ap.add_argument("--depth-head-out", required=True, metavar="HEAD.npz")
    ap.add_argument("--depth-layers", required=True, metavar="L1,L2,..", help="the backbone layers (0-based, ascending) whose tokens the head reads, e.g. 2,5,8,11")
    ap.add_argument("--depth-hidden", type=int, required=True, metavar="D", help="the backbone's hidden size: it splits the head into its patch and class halves")
    ap.add_argument("--depth-min", type=float, default=0.001); ap.add_argument("--depth-max", type=float, default=10.0)
    ap.add_argument("--depth-bins", default="UD", choices=["UD", "SID"], help="bin centres: uniform (default) or log-spaced")
    ap.add_argument("--depth-upsample", type=int, default=4, choices=[1, 2, 4])
    ap.add_argument("--depth-norm", action="store_true", help="the head was trained on final-norm tokens (default: the raw residual stream)")
    a = ap.parse_args(argv)
    import torch
    sd = torch.load(a.depth_head_in, map_location="cpu", weights_only=True)
    head = depth_head(sd, [int(x) for x in a.depth_layers.split(",")], a.depth_hidden, a.depth_min, a.depth_max, a.depth_bins, a.depth_upsample, a.depth_norm)
    write_depth_head(a.depth_head_out, head)
    print(f"wrote {a.depth_head_out}: {head['wp'].shape[0]} bins, width {head['wp'].shape[1]}, layers {head['layers']}, class half: {'yes' if head['wc'] is not None else 'no'}")
    return 0


def main(argv=None) -> int:
    if any(str(x).split("=")[0] == "--depth-head-in" for x in (sys.argv[1:] if argv is None else argv)):
        return _main_depth_head(argv)
    if any(str(x).split("=")[0] == "--dense-head-in" for x in (sys.argv[1:] if argv is None else argv)):
        return _main_dense_head(argv)          # a head is a file of its own: no model file is read or written
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("model"); ap.add_argument("out"); ap.add_argument("--ftype", type=int, default=1, help="0 f32, 1 f16 (default), 2/3/6/7/8 q4_0/q4_1/q5_0/q5_1/q8_0")
    ap.add_argument("--vitstr", action="store_true", help="one-channel ViTSTR scene-text model: write the character set as labels")
    ap.add_argument("--no-head", action="store_true", help="a DINOv2 backbone (Dinov2Model / Dinov2WithRegistersModel): the file gets a one-class head of zeros "
                                                           "labelled '(no head)'; read the embeddings with --embed / vitx_feat_*")
    ap.add_argument("--gated-mlp", action="store_true", help="opt in to the gated (SwiGLU) MLP of DINOv2 ViT-g/14 (use_swiglu_ffn) / DINOv3 ViT-H+ (use_gated_mlp): the file "
                                                            "carries the `glu` tensor, which the reference and engine builds before it cannot read")
    ap.add_argument("--timm-state-dict", action="store_true", help="`model` is a torch-saved timm VisionTransformer state_dict (.pth); no timm import needed")
    ap.add_argument("--heads", type=int, default=0, help="attention heads of a timm checkpoint (inferred only for the widths of released timm ViTs; required otherwise)")
    ap.add_argument("--act", default="tanh", choices=sorted(_ACT_NAMES), help="MLP activation of a timm checkpoint (a state dict carries no config): tanh = ggml's GELU, the "
                                                                                  "reference's (default); erf = nn.GELU, what timm's VisionTransformer uses; quick = QuickGELU")
    ap.add_argument("--eps", type=float, default=1e-6, help="LayerNorm epsilon of a timm checkpoint (default 1e-6, timm's)")
    ap.add_argument("--labels", default=None, help="JSON file {class id: label} for a timm checkpoint (default: none are written)")
    ap.add_argument("--img-size", type=int, default=0, metavar="N",
                    help="write the file at N x N instead of the checkpoint's size: pos_embed is resampled (vitx_model_resize_file), nothing else changes")
    ap.add_argument("--pos-interp", default="bicubic", choices=["bicubic", "bicubic-aa"],
                    help="with --img-size: F.interpolate(mode='bicubic') without (HuggingFace ViT / Dinov2, DINO) or with antialias=True (timm; "
                         "transformers 5.x for Dinov2WithRegisters)")
    ap.add_argument("--no-preproc", action="store_true", help="write the file without the `preproc` tensor even when a preprocessor_config.json lies beside the model")
    ap.add_argument("--pp-resize", type=int, default=0, metavar="N", help="timm checkpoint: Resize(N), the shortest edge (default: the crop)")
    ap.add_argument("--pp-crop", type=int, default=0, metavar="N", help="timm checkpoint: CenterCrop(N) (default and only value: the model's img_size)")
    ap.add_argument("--pp-filter", default="", choices=["", "bilinear", "bicubic"], help="timm checkpoint: Pillow's resize filter (default bicubic)")
    ap.add_argument("--pp-mean", type=float, nargs=3, default=None, metavar=("R", "G", "B"), help="timm checkpoint: Normalize mean on the 0..1 scale (default ImageNet's)")
    ap.add_argument("--pp-std", type=float, nargs=3, default=None, metavar=("R", "G", "B"), help="timm checkpoint: Normalize std on the 0..1 scale (default ImageNet's)")
    ap.add_argument("--pp-crop-round", default="", choices=["", "floor", "torchvision"],
                    help="timm checkpoint: the crop offset of an odd difference: floor (default; transformers) or torchvision (CenterCrop rounds half to even)")
    ap.add_argument("--zero-shot-ids", default=None, metavar="IDS.npy", help="CLIPModel / SiglipModel directory: also write a zero-shot bank from these token ids, "
                                                                              "an integer array [prompts][tokens] (IDS.mask.npy beside it, if present, is the attention mask)")
    ap.add_argument("--zero-shot-prompts", default=None, metavar="PROMPTS.txt",
                    help="the same from one prompt per line, tokenised with the tokenizer found in the model directory (padding='max_length', as both publishers do). "
                         "UNTESTED: the tokenisation step has never run in this project's tests -- no tokenizer files were available to them; everything after "
                         "the token ids is the tested --zero-shot-ids path")
    ap.add_argument("--zero-shot-labels", default=None, metavar="LABELS.txt", help="one class name per line (default: the prompts themselves, or class_<k>)")
    ap.add_argument("--zero-shot-out", default=None, metavar="BANK.npz", help="where the bank goes (embeds, labels, kind, scale, bias)")
    ap.add_argument("--text-out", default=None, metavar="TEXT.gguf", help="CLIPModel / SiglipModel (or a text tower alone): also write the text tower as a text-tower file "
                                                                          "(convert_hf_text_model; vit_cli.py --text-model)")
    a = ap.parse_args(argv)
    if a.text_out and a.timm_state_dict:
        ap.error("--text-out needs a HuggingFace CLIP / SigLIP checkpoint, not a timm state dict")
    if (a.zero_shot_ids is None) == (a.zero_shot_prompts is None) and a.zero_shot_out:
        ap.error("--zero-shot-out needs exactly one of --zero-shot-ids and --zero-shot-prompts")
    if (a.zero_shot_ids or a.zero_shot_prompts or a.zero_shot_labels) and not a.zero_shot_out:
        ap.error("--zero-shot-ids / --zero-shot-prompts / --zero-shot-labels need --zero-shot-out BANK.npz")
    if a.zero_shot_out and a.timm_state_dict:
        ap.error("a zero-shot bank needs the text tower of a HuggingFace CLIPModel / SiglipModel, not a timm state dict")
    if not a.timm_state_dict and any((a.pp_resize, a.pp_crop, a.pp_filter, a.pp_mean, a.pp_std, a.pp_crop_round)):
        ap.error("--pp-* describe a timm checkpoint (--timm-state-dict); a HuggingFace checkpoint brings its preprocessor_config.json")
    if a.timm_state_dict:
        import torch
        sd = torch.load(a.model, map_location="cpu", weights_only=True)
        labels = {int(k): str(v) for k, v in json.load(open(a.labels)).items()} if a.labels else None
        pp_cli = dict(resize=a.pp_resize, crop=a.pp_crop, filt=a.pp_filter, mean=a.pp_mean, std=a.pp_std, crop_round=a.pp_crop_round)
        hp = convert_timm_state_dict(sd, a.out, a.ftype, heads=a.heads, id2label=labels, act=a.act, eps=a.eps, preproc=None if a.no_preproc else pp_cli)
    else:
        import transformers
        model_type = transformers.AutoConfig.from_pretrained(a.model).model_type
        if a.zero_shot_out:
            if model_type not in _TWO_TOWERS:
                ap.error(f"a zero-shot bank needs a CLIPModel or SiglipModel checkpoint (both towers), not model_type '{model_type}'")
            _main_bank(a, transformers, model_type)
        if a.text_out:
            if model_type not in _TWO_TOWERS + ("clip_text_model", "siglip_text_model"):
                ap.error(f"--text-out needs a CLIP or SigLIP checkpoint, not model_type '{model_type}'")
            tcls = {"clip": "CLIPModel", "siglip": "SiglipModel"}.get(model_type) or FAMILIES[model_type].loaders[0]
            thp = convert_hf_text_model(getattr(transformers, tcls).from_pretrained(a.model).eval(), a.text_out, a.ftype)
            print(f"wrote {a.text_out}: text tower, hidden {thp.hidden_size}, layers {thp.num_hidden_layers}, heads {thp.num_attention_heads}, width {thp.num_classes}, tokens {thp.img_size}, ftype {a.ftype}")
            if model_type not in _TWO_TOWERS:
                return 0                                   # a text tower alone: there is no vision file to write
        fam = FAMILIES.get(model_type, _VIT)
        m = getattr(transformers, fam.loaders[1 if a.no_head and fam.head == "optional" else 0]).from_pretrained(a.model).eval()
        pc, pc_path = None, os.path.join(a.model, "preprocessor_config.json")
        if not a.no_preproc and not a.vitstr:
            if os.path.isfile(pc_path):
                with open(pc_path) as f:
                    pc = json.load(f)
            else:
                print(f"note: no preprocessor_config.json beside '{a.model}': the file is written without a `preproc` tensor")
        hp = convert_hf_model(m, a.out, a.ftype, vitstr=a.vitstr, no_head=a.no_head, preprocessor_config=pc, gated_mlp=a.gated_mlp)
    if a.img_size and a.img_size != hp.img_size:           # written at the checkpoint's size first, then replaced by its --img-size version
        from . import binding
        tmp = a.out + f".src{os.getpid()}"
        os.replace(a.out, tmp)
        try:
            binding.resize_file(tmp, a.out, a.img_size, binding.POS_BICUBIC_AA if a.pos_interp == "bicubic-aa" else binding.POS_BICUBIC)
        finally:
            os.remove(tmp)
        hp.img_size = a.img_size
    print(f"wrote {a.out}: hidden {hp.hidden_size}, layers {hp.num_hidden_layers}, heads {hp.num_attention_heads}, classes {hp.num_classes}, patch {hp.patch_size}, img {hp.img_size}, ftype {a.ftype}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
