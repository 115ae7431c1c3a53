"""Data, float64 restatement and CPU-side conditions of the text-tower tests (tests/test_cpu_text.py, tests/test_gpu_text.py; include/vitx.h
"the text tower").  Nothing here touches a GPU or libvitx.so.

forward64(t, ids) restates the forward of a text-tower file in float64:
    X = tok[ids] + pos;  per layer: x += proj(attention(qkv(LN1 x))), x += fc2(act(fc1(LN2 x)));  e = head(LN_final(x[pooled]))
with the file's activation, eps, causal mask and pooling rule (arch = {activation, eps, causal, eos + 1}: the FIRST position whose id is eos, or
the last position): the token-embedding front, the layer stack of ref64.blocks64, the pooling and the head.  `wround` is applied to every matrix,
`uround` to every activation that enters a GEMM and to the stored qkv (the attention operands), `tround` to the token table (the f16 table of an
ftype 1 file).

The attention data: the cases of the issue, the causal staircase (every key of an (item, head) the same vector: every numerator exactly 1;
v[j][d] = (2 j + 1) u_d, u_d a power of two: row t of the causal output is exactly (t + 1) u_d, every row of the unmasked output T u_d), and
masked versions of exact_data's float64 reference and f32 emulation, made of exact_data's own functions row by row (row t of a causal
attention IS the unmasked attention of query t over keys 0 .. t)."""
import numpy as np

import arch_data as AD
import exact_data as X
import ref64 as R64
import zs_data as Z

ATTN_CASES = [(3, 1, 2, 64), (3, 15, 2, 64), (3, 16, 2, 64), (3, 17, 2, 64), (2, 33, 2, 72), (2, 64, 3, 64), (2, 77, 2, 64), (2, 128, 1, 128), (2, 77, 2, 8)]
case_id = lambda c: "n%d_T%d_H%d_hd%d" % c


# ------------------------------------------------------------------------------------------------ the causal staircase
def staircase_qkv(n, T, H, hd, sign, seed):
    """qkv [n * T][3 * H * hd] f32 (exact in f16 and bf16) and u [n][H][hd].  Per (item, head): every key is the same +-1 vector kappa;
    q_i = sign * g * kappa on a random half of the columns (exact_data.flat_qkv's queries: every raw score of the item is the same integer);
    v[j][d] = (2 j + 1) * u_d with u_d = 2^e, e in -3 .. 2."""
    rng = np.random.default_rng(seed)
    g = X.flat_gain(hd)
    qkv = np.zeros((n, T, 3, H, hd), np.float32)
    u = np.empty((n, H, hd), np.float32)
    for b in range(n):
        for h in range(H):
            kappa = rng.integers(0, 2, hd) * 2.0 - 1.0
            half = np.argsort(rng.random((T, hd)), axis=1) < hd // 2
            uu = np.exp2(rng.integers(-3, 3, hd)).astype(np.float32)
            qkv[b, :, 0, h] = sign * g * kappa * half; qkv[b, :, 1, h] = kappa
            qkv[b, :, 2, h] = (2.0 * np.arange(T)[:, None] + 1.0) * uu
            u[b, h] = uu
    return qkv.reshape(n * T, 3 * H * hd), u


def staircase_expected(u, T, causal):
    """[n * T][H * hd] f32: row t = (t + 1) u (causal) or T u (no mask)."""
    n, H, hd = u.shape
    steps = (np.arange(T) + 1.0) if causal else np.full(T, float(T))
    return (steps[None, :, None, None] * u[:, None]).astype(np.float32).reshape(n * T, H * hd)


def staircase_f32(qkv, n, T, H, hd, causal, leak=None, drop=None):
    """The schedule in f32 on the CPU: numerators exactly 1 on the kept keys (all scores of an item are equal), f32 sum of the numerators, f32
    P.V, times fl(1 / sum).  leak = (t, j): row t also counts key j > t; drop = (t, j): row t loses key j <= t.  [n * T][H * hd] f32."""
    f = np.float32
    v = qkv.reshape(n, T, 3, H, hd)[:, :, 2].astype(f)
    out = np.empty((n, T, H, hd), f)
    for t in range(T):
        keep = np.arange(T) <= t if causal else np.ones(T, bool)
        if leak is not None and leak[0] == t:
            keep[leak[1]] = True
        if drop is not None and drop[0] == t:
            keep[drop[1]] = False
        s = f(0.0); pv = np.zeros((n, H, hd), f)
        for j in np.flatnonzero(keep):
            s = f(s + f(1.0)); pv = (pv + v[:, j]).astype(f)
        out[:, t] = (pv * f(f(1.0) / s)).astype(f)
    return out.reshape(n * T, H * hd)


# ------------------------------------------------------------------------------------------------ masked reference, bound and emulation
def masked_ref(q, k, v, scale, causal, want_bound=False):
    """exact_data.attention_ref with the mask applied: masked scores are -inf in float64, i.e. row t attends keys 0 .. t."""
    import torch
    if not causal:
        return X.attention_ref(q, k, v, scale, want_bound=want_bound)
    outs = [X.attention_ref(q[:, t:t + 1], k[:, :t + 1], v[:, :t + 1], scale, want_bound=want_bound) for t in range(q.shape[1])]
    if not want_bound:
        return torch.cat(outs, dim=1)
    return torch.cat([o[0] for o in outs], dim=1), torch.cat([o[1] for o in outs], dim=1)


def masked_emu(q, k, v, scale, dtype_name, causal):
    """exact_data.attention_emu in this kernel's schedule ("single": two passes, the row maximum first), with the mask"""
    import torch
    if not causal:
        return X.attention_emu(q, k, v, scale, dtype_name, "single")
    return torch.cat([X.attention_emu(q[:, t:t + 1], k[:, :t + 1], v[:, :t + 1], scale, dtype_name, "single") for t in range(q.shape[1])], dim=1)


def masked_faults(q, k, v, scale, causal, n, H):
    """The three faults on the float64 reference: {name: out64}.  Without a mask they are exact_data.attention_faults' (one more key: token 0 of
    the next item's same head; the last key missing; the scale 2 % too large).  Causal: leak = every row t < T - 1 also sees key t + 1 (one
    future key); drop = every row t >= 1 loses key 0 (one past key); scale as before."""
    import torch
    if not causal:
        return X.attention_faults(q, k, v, scale, n, H)
    T = q.shape[1]
    leak = torch.cat([X.attention_ref(q[:, t:t + 1], k[:, :min(t + 2, T)], v[:, :min(t + 2, T)], scale) for t in range(T)], dim=1)
    drop = torch.cat([X.attention_ref(q[:, t:t + 1], k[:, (1 if t else 0):t + 1], v[:, (1 if t else 0):t + 1], scale) for t in range(T)], dim=1)
    return {"leak": leak, "drop": drop, "scale": masked_ref(q, k, v, scale * 1.02, True)}


# ------------------------------------------------------------------------------------------------ the two micro text towers
CLIP_CFG = dict(vocab_size=96, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=24,
                projection_dim=64, eos_token_id=95, bos_token_id=94, pad_token_id=0, layer_norm_eps=float(np.float32(1e-5)))
SIGLIP_CFG = dict(vocab_size=96, hidden_size=128, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, max_position_embeddings=16,
                  layer_norm_eps=float(np.float32(1e-6)))          # eps as the file carries it (an f32): the model and the file then state the same number
HEADS = 2
N_PROMPTS = 17
PROMPT_SEED = 5


def hf_model(family):
    """The randomly initialised transformers text tower of a family, float64, eval.  Nothing is downloaded."""
    import torch
    import transformers
    torch.manual_seed(11 if family == "clip" else 12)
    if family == "clip":
        m = transformers.CLIPTextModelWithProjection(transformers.CLIPTextConfig(**CLIP_CFG))
    else:
        m = transformers.SiglipTextModel(transformers.SiglipTextConfig(**SIGLIP_CFG))
    return m.double().eval()


def text_file(pkg, family, ftype=1):
    """Path of the (cached) text-tower file of a family's micro model."""
    return R64.cached_file(f"text-{family}-micro-ft{ftype}", lambda tmp: pkg.convert.convert_hf_text_model(hf_model(family), tmp, ftype))


def prompts(family, n=N_PROMPTS, seed=PROMPT_SEED):
    """ids [n][T] int32.  CLIP: BOS, words, EOS at position 5 (row 0), T - 1 (row 1) and anywhere from 2 on (the rest), pad id 0 behind it;
    SigLIP: words to the end (no EOS: the last position is pooled)."""
    cfg = CLIP_CFG if family == "clip" else SIGLIP_CFG
    T, V = cfg["max_position_embeddings"], cfg["vocab_size"]
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, V - 2, (n, T)).astype(np.int32)
    if family == "clip":
        ids[:, 0] = CLIP_CFG["bos_token_id"]
        at = rng.integers(2, T, n); at[0] = 5; at[1] = T - 1
        for i in range(n):
            ids[i, at[i]] = CLIP_CFG["eos_token_id"]; ids[i, at[i] + 1:] = CLIP_CFG["pad_token_id"]
    return ids


def text_arch(t):
    """(activation, eps, causal, eos) of a text file's tensors; eos -1: pool the last position"""
    a = np.asarray(t["arch"], np.float32).reshape(-1)
    return int(a[0]), float(a[1]), int(a[2]), int(a[3]) - 1


def pooled_positions(ids, eos):
    ids = np.asarray(ids)
    if eos < 0:
        return np.full(ids.shape[0], ids.shape[1] - 1)
    hit = ids == eos
    assert hit.any(axis=1).all(), "a prompt without EOS"
    return hit.argmax(axis=1)


def forward64(t, ids, heads=HEADS, wround=None, uround=None, tround=None):
    """t: {name: f32 array} of a text-tower file (prefix_data.file_tensors); ids [n][T].  Returns the projected embeddings [n][E] float64."""
    f8 = lambda a: np.asarray(a, np.float64)
    W = (lambda a: f8(wround(a))) if wround else f8
    U = (lambda a: f8(uround(a))) if uround else f8
    act, eps, causal, eos = text_arch(t)
    eps = float(np.float32(eps))
    ids = np.asarray(ids)
    n, T = ids.shape
    tok = f8(tround(t["token_embed.weight"]) if tround else t["token_embed.weight"])
    D = tok.shape[1]
    x = tok[ids] + f8(t["pos_embed"]).reshape(T, D)
    mask = np.where(np.arange(T)[None, :] > np.arange(T)[:, None], -np.inf, 0.0) if causal else None
    x = R64.blocks64(t, x, heads, act, eps, mask=mask, wround=wround, uround=uround, round_qkv=True)[0]
    rows = x[np.arange(n), pooled_positions(ids, eos)]
    z = U(AD.layernorm64(rows, f8(t["norm.weight"]), f8(t["norm.bias"]), eps))
    return z @ W(t["head.weight"]).T + f8(t["head.bias"])


# ------------------------------------------------------------------------------------------------ zero-shot through the engine
def zs_family_file(pkg, family):
    """The vision micro file of zs_data whose embedding width matches the family's text tower (CLIP: 64; SigLIP-class: D = 128)."""
    return Z.model_file(pkg, family)


def zs_groups(n=N_PROMPTS):
    """17 prompts in 12 classes: the first five classes are ensembles of two prompts"""
    return np.array([0, 0, 1, 1, 2, 2, 3, 3, 4, 4] + list(range(5, 5 + n - 10)))


def bank64(e, groups):
    """convert.zeroshot_bank's ensembling of embeddings e [P][E] in float64"""
    e = Z.normalise64(e)
    K = int(groups.max()) + 1
    mean = np.zeros((K, e.shape[1]))
    np.add.at(mean, groups, e)
    return Z.normalise64(mean / np.bincount(groups, minlength=K)[:, None])


def zs_constants(family):
    """(kind, scale, bias) of a family's zero-shot test: zs_data's, of the order of the released models' (a tower converted alone carries no `zs`)"""
    return (Z.SOFTMAX, Z.CLIP_SCALE, 0.0) if family == "clip" else (Z.SIGMOID, Z.SIGLIP_SCALE, Z.SIGLIP_BIAS)


def variant_tensors(t, T=None, D=None, V=None):
    """The tensors of a text file re-drawn at another context length, width or vocabulary (random values of the same scale, same names and order):
    files the loader accepts and a text context may refuse."""
    rng = np.random.default_rng(1)
    D0 = t["token_embed.weight"].shape[1]
    D = D or D0
    out = {}
    for k, v in t.items():
        shape = tuple(D * (s // D0) if s % D0 == 0 else s for s in v.shape) if k not in ("arch", "zs") else v.shape
        if k == "pos_embed" and T:
            shape = (T, D)
        if k == "token_embed.weight" and V:
            shape = (V, D)
        if k == "head.weight":
            shape = (v.shape[0], D)
        out[k] = v if shape == v.shape else (rng.standard_normal(shape) * 0.02).astype(np.float32)
    return out


def write_variant(pkg, t, path, ftype=1, heads=HEADS, **change):
    tt = variant_tensors(t, **change)
    V, D = tt["token_embed.weight"].shape
    L = 1 + max(int(k.split(".")[1]) for k in tt if k.startswith("blocks."))
    hp = pkg.ggml_file.HParams(D, L, heads, tt["head.weight"].shape[0], 0, tt["pos_embed"].shape[0], ftype)
    pkg.ggml_file.write_model(path, hp, tt, id2label={}, ftype=ftype)
    return hp
