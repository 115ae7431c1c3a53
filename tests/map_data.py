"""Models without a class token whose embedding comes from a multi-head attention-pooling (MAP) head (include/vitx.h "no class token and the
attention-pooling head": SigLIP), shared by tests/test_cpu_map_head.py -- which pins the restatement of such a file to transformers'
SiglipVisionModel -- and tests/test_gpu_map_head.py.

What the family owns of the float64 restatement tests/ref64.py (T = 0 prefix tokens there: an image is its patch rows, patch t takes pos_embed[t]):
the gates on the pooled embedding, the micro fixture, and the head (head64, u64, pool64) in two forms that are identical in exact arithmetic:
    textbook   q = Wq latent + bq; k_t = Wk F[t] + bk; v_t = Wv F[t] + bv; p_h = softmax_t(q_h . k_{t,h} / sqrt(d)); o_h = sum_t p_{h,t} v_{t,h}
    folded     u_h = Wk_h^T q_h / sqrt(d); s_{h,t} = u_h . F[t]; p_h = softmax_t(s_h); M_h = sum_t p_{h,t} F[t]; o_h = Wv_h M_h + bv_h
then a = Wproj o + bproj and e = a + fc2(act(fc1(LN(a)))).  The folded form carries the engine's rounding points (`uround` on M, o, LN(a), the fc1
output and e as the head operand; `wround` on every matrix; u is rounded to f32 as vitx_model_pool_query stores it)."""
import numpy as np

import arch_data as AD

MICRO = AD.MICRO
# make_weights draws every matrix at 0.02 (clipped at 0.04): with the probe, q.weight and the K rows at that scale the scores differ by 1e-3 and
# p_h is flat -- a kernel that ignored the scores would pass.  These factors spread them over a few units (asserted in tests/test_cpu_map_head.py).
Q_SCALE, K_SCALE = 64.0, 48.0
POOL_NAMES = ("latent", "q.weight", "q.bias", "kv.weight", "kv.bias", "proj.weight", "proj.bias", "norm.weight", "norm.bias",
              "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias")


# ---- the end-to-end gates on the pooled embedding e of the MICRO fixture file (ftype 1), the 17 images of tests/test_gpu_map_head.py, by operand
# type (0 fp16, 1 bf16).  Each gate is 2 x the larger of two figures, the margin ORACLE_COS gets in tests/test_gpu_features.py:
#   *_GPU  measured once on the MI355X (VITX_FEAT_CLS of a 17-image forward against the unrounded restatement);
#   *_CPU  the restatement with operand rounding (uround / wround) against the unrounded restatement: the reference's own noise
#          (tests/test_cpu_map_head.py recomputes both).
# COS: 1 - cos(e, restatement), worst image.  It sees a wrong direction of e: the flat-softmax mutant is at 8.9e-2.
# LEN: | mean over the images of |e| / |e_restatement|  -  1 |.  The wrong MLP activation in the head (QuickGELU for tanh-GELU) mostly RESCALES e:
#      1 - cos 1.6e-5, inside bf16's own 1.75e-5, and the probabilities move by 9.8e-3 against bf16's gate of 2e-2 -- but every image's e gets
#      0.35 .. 0.53 % shorter, the mean 0.44 %, while operand rounding moves single images by up to 0.14 % with either sign and the mean by
#      0.034 %.  The mean length is the quantity that separates this mutant under bf16.
COS_GPU = {0: 1.12e-7, 1: 1.54e-5}
COS_CPU = {0: 9.2e-8, 1: 1.75e-5}
LEN_GPU = {0: 1.3e-5, 1: 4.26e-4}
LEN_CPU = {0: 8.4e-6, 1: 3.45e-4}


def cos_gate(dtype):
    return 2 * max(COS_GPU[dtype], COS_CPU[dtype])


def len_gate(dtype):
    return 2 * max(LEN_GPU[dtype], LEN_CPU[dtype])


def mean_length(e, ref):
    """mean over the images of |e| / |ref| - 1 (signed), in float64."""
    e = np.asarray(e, np.float64); ref = np.asarray(ref, np.float64)
    return float((np.linalg.norm(e, axis=1) / np.linalg.norm(ref, axis=1)).mean() - 1.0)


def pool_tensors(D, seed=4242, q_scale=Q_SCALE, k_scale=K_SCALE):
    """The thirteen attn_pool.* tensors, drawn as pkg.synth.make_weights draws matrices and vectors."""
    rng = np.random.default_rng(seed)
    mat = lambda *shape: np.clip(rng.standard_normal(shape, dtype=np.float32) * np.float32(0.02), -0.04, 0.04).astype(np.float32)
    vec = lambda n, mean=0.0: (np.float32(mean) + rng.standard_normal(n, dtype=np.float32) * np.float32(0.02)).astype(np.float32)
    t = {}
    t["attn_pool.latent"] = mat(1, 1, D)
    t["attn_pool.q.weight"] = (mat(D, D) * np.float32(q_scale)).astype(np.float32); t["attn_pool.q.bias"] = vec(D)
    kv = mat(2 * D, D); kv[:D] *= np.float32(k_scale)
    t["attn_pool.kv.weight"] = kv; t["attn_pool.kv.bias"] = vec(2 * D)           # a non-zero K bias: it must cancel in the softmax
    t["attn_pool.proj.weight"] = mat(D, D); t["attn_pool.proj.bias"] = vec(D)
    t["attn_pool.norm.weight"] = vec(D, 1.0); t["attn_pool.norm.bias"] = vec(D)
    # the MLP of the head at arch_data.CLIP_MLP_SCALE: at 0.02 its activation sees |x| < 0.5, where tanh- and erf-GELU coincide to 1e-4, and the
    # wrong activation would move e by 1 - cos = 6e-10 (measured on this restatement): no gate could see it
    t["attn_pool.mlp.fc1.weight"] = (mat(4 * D, D) * np.float32(AD.CLIP_MLP_SCALE[0])).astype(np.float32); t["attn_pool.mlp.fc1.bias"] = vec(4 * D)
    t["attn_pool.mlp.fc2.weight"] = (mat(D, 4 * D) * np.float32(AD.CLIP_MLP_SCALE[1])).astype(np.float32); t["attn_pool.mlp.fc2.bias"] = vec(D)
    return t


def fixture_tensors(pkg, name=MICRO, head=True, activation=AD.ACT_TANH, eps=1e-6):
    """Synthetic weights of pkg.synth.make_weights (head scale 4) without the class token, pos_embed without its class row, + attn_pool.* after
    norm.bias.  head=False: the one-class head of zeros a converted tower has."""
    hp = pkg.synth.hparams_for(name)
    w = pkg.synth.make_weights(hp, head_scale=4.0)
    D = hp.hidden_size
    out = {}
    if (activation, np.float32(eps)) != (AD.ACT_TANH, np.float32(1e-6)):
        out["arch"] = np.array([activation, eps, 0, 0], np.float32)
    for k, v in w.items():
        if k == "cls_token":
            continue
        if k == "pos_embed":
            v = np.ascontiguousarray(v[:, 1:])
        if k == "head.weight":
            out.update(pool_tensors(D))
            if not head:
                out["head.weight"] = np.zeros((1, D), np.float32); out["head.bias"] = np.zeros((1,), np.float32)
                break
        out[k] = v
    if not head:
        hp.num_classes = 1
    return hp, out


def fixture_file(pkg, ftype=1, name=MICRO, head=True, activation=AD.ACT_TANH):
    from ref64 import cached_file
    return cached_file(f"map-{name}-h{int(head)}-a{activation}-ft{ftype}",
                       lambda tmp: pkg.ggml_file.write_model(tmp, *fixture_tensors(pkg, name, head, activation), ftype=ftype, id2label=None if head else {0: "(no head)"}))


def u64(t, heads):
    """u [H][D] in float64: u_h = Wk_h^T q_h / sqrt(d), q = Wq latent + bq.  Also returns sum |terms| of every element's K-side sum (the
    bound of tests/test_cpu_map_head.py)."""
    f8 = lambda a: np.asarray(a, np.float64)
    D = t["attn_pool.latent"].shape[-1]
    d = D // heads
    q = f8(t["attn_pool.q.weight"]) @ f8(t["attn_pool.latent"]).reshape(D) + f8(t["attn_pool.q.bias"])
    wk = f8(t["attn_pool.kv.weight"])[:D]
    u = np.empty((heads, D)); mag = np.empty((heads, D))
    for h in range(heads):
        qh = q[h * d:(h + 1) * d]
        u[h] = wk[h * d:(h + 1) * d].T @ qh / np.sqrt(d)
        mag[h] = np.abs(wk[h * d:(h + 1) * d]).T @ np.abs(qh) / np.sqrt(d)
    return u, mag


def pool64(F, u, flat=False):
    """F [n][N][D], u [H][D] -> (M [n][H][D], p [n][H][N]) in float64.  flat: the mutant that ignores the scores."""
    F = np.asarray(F, np.float64); u = np.asarray(u, np.float64)
    s = np.einsum("hk,ntk->nht", u, F)
    if flat:
        s = np.zeros_like(s)
    p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
    return np.einsum("nht,ntk->nhk", p, F), p


def head64(t, F, heads, folded=True, flat=False, activation=None, eps=None, wround=None, uround=None):
    """The MAP head on the final-norm rows F [n][N][D]: dict(e [n][D], M [n][H][D] (folded only), p [n][H][N])."""
    f8 = lambda a: np.asarray(a, np.float64)
    W = (lambda a: f8(wround(a))) if wround else f8
    U = (lambda a: f8(uround(a))) if uround else f8
    f_act, f_eps, _ = AD.arch_of(t)
    activation = f_act if activation is None else activation
    eps = float(np.float32(f_eps if eps is None else eps))
    n, N, D = F.shape
    d = D // heads
    g = lambda k: t["attn_pool." + k]
    wkv, bkv = g("kv.weight"), f8(g("kv.bias"))
    M = None
    if folded:
        u, _ = u64(t, heads)
        if wround or uround:
            u = f8(np.asarray(u, np.float32))              # the engine keeps u in f32
        M, p = pool64(F, u, flat)
        wv = W(wkv[D:])
        o = np.concatenate([U(M[:, h]) @ wv[h * d:(h + 1) * d].T for h in range(heads)], 1) + bkv[D:]
        o = U(o)
    else:
        q = f8(g("q.weight")) @ f8(g("latent")).reshape(D) + f8(g("q.bias"))
        k = F @ f8(wkv[:D]).T + bkv[:D]
        v = F @ f8(wkv[D:]).T + bkv[D:]
        s = np.einsum("hj,nthj->nht", q.reshape(heads, d), k.reshape(n, N, heads, d)) / np.sqrt(d)
        if flat:
            s = np.zeros_like(s)
        p = np.exp(s - s.max(-1, keepdims=True)); p /= p.sum(-1, keepdims=True)
        o = np.einsum("nht,nthj->nhj", p, v.reshape(n, N, heads, d)).reshape(n, D)
    a = o @ W(g("proj.weight")).T + f8(g("proj.bias"))
    hdn = U(AD.act64(U(AD.layernorm64(a, f8(g("norm.weight")), f8(g("norm.bias")), eps)) @ W(g("mlp.fc1.weight")).T + f8(g("mlp.fc1.bias")), activation))
    e = a + hdn @ W(g("mlp.fc2.weight")).T + f8(g("mlp.fc2.bias"))
    return dict(e=e, M=M, p=p, a=a)


def one_minus_cos(a, b):
    """1 - cos per row, [n][D] x [n][D] -> [n], in float64."""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    return 1.0 - (a * b).sum(-1) / np.sqrt((a * a).sum(-1) * (b * b).sum(-1))
