"""vit.h's batch entry points and its vit_state / vit_text_state context cache (csrc/vit_api.cpp) on the MI355X, run by tests/cpp/vit_h_driver.cpp in a
child process and compared with the C ABI called through `binding` here: the same model file, pixels, operand type and batch.  The wrappers add no
arithmetic, so every comparison is bit for bit.  An image's bits do not depend on its batch or on the capacity of its context (test_gpu_features.py,
test_gpu_pack.py), so the reference contexts are created at the batch of the call."""
import numpy as np
import pytest

import dense_data as DD
import depth_data as PD
import text_data as TD
import vit_h_data as VH
import zs_data as ZD

pytestmark = pytest.mark.gpu

F16, BF16 = 0, 1
S = 56                                    # the side of every micro file here; patch 14, D 128, 2 layers
RECT = (28, 70)                           # a rectangular state's (img_h, img_w)
SMALL = 28                                # a resized state's img_size: a 2 x 2 grid, so the position table is DOWNsampled (antialias changes it)
PACK_SHAPES = [(56, 56), (28, 70), (42, 28), (28, 70), (70, 42), (56, 56)]      # four distinct shapes, two of them repeated
OUT = [(0, 0), (23, 45), (0, 0), (45, 23)]


def _exact(n, h, w, seed):
    """[n][h][w][3] f32 multiples of 1/16 in [-4, 4) (prefix_data.exact_images' rule)."""
    return (np.random.default_rng(seed).integers(-64, 64, (n, h, w, 3)) / 16.0).astype(np.float32)


SQUARE = ZD.images()                      # 17 images 56 x 56: driver images 0 .. 16
RECTS = _exact(3, *RECT, seed=11)         # 17 .. 19
SMALLS = _exact(3, SMALL, SMALL, seed=12)  # 20 .. 22
PACK = [_exact(1, h, w, seed=20 + i)[0] for i, (h, w) in enumerate(PACK_SHAPES)]     # 23 .. 28
AT_RECT, AT_SMALL, AT_PACK = 17, 20, 23
ALL_IMAGES = list(SQUARE) + list(RECTS) + list(SMALLS) + PACK


@pytest.fixture(scope="module")
def driver(binding, tmp_path_factory):
    return VH.build_driver(tmp_path_factory.mktemp("vit_h_driver"))


@pytest.fixture(scope="module")
def files(pkg):
    reg = lambda pool: pkg.synth.cached_synthetic("vit_micro_patch14_56", ftype=1, head_scale=4.0, registers=4, head_pool=pool)
    return {"clip": ZD.model_file(pkg, "clip"), "siglip": ZD.model_file(pkg, "siglip"), "reg": reg(0), "regmean": reg(1)}


@pytest.fixture()
def data(tmp_path):
    return VH.Data(tmp_path / "data", ALL_IMAGES)


def _forward(binding, path, imgs, dtype=F16, **kw):
    """The class probabilities of a fresh binding.Context on imgs."""
    model = binding.Model(path)
    ctx = binding.Context(model, device=0, max_batch=len(imgs), dtype=dtype, **kw)
    probs = ctx.forward(np.asarray(imgs))
    ctx.close(); model.close()
    return probs


def _pack_forward(binding, path, imgs, dtype=F16):
    model = binding.Model(path)
    tokens = int(binding.pack_check(model, [a.shape[:2] for a in imgs], 2 ** 31 - 1, len(imgs))[-1])
    pack = binding.PackContext(model, device=0, max_tokens=tokens, max_images=len(imgs), dtype=dtype)
    probs, _ = pack.forward(imgs)
    pack.close(); model.close()
    return probs


def _check_predict(st, probs):
    """state.prediction is `probs`; the sorted pairs are its permutation, image by image."""
    assert st.rc == 0
    assert VH.same(st.arr("prediction", "<f4"), probs.ravel()), st.index
    rows = st.rows("pairs", VH.PAIR)
    assert len(rows) == len(probs)
    for r, p in zip(rows, probs):
        VH.check_sorted_pairs(r, p)


def _check_refused(st):
    """Return code 1, empty output, no head left on."""
    assert st.rc == 1, st.index
    assert st.arr("counts", "<i4").size == 0, st.index
    assert st.heads_off(), st.status


# ------------------------------------------------------------------------------------------------ vit_predict_batch, vit_pack_batch
@pytest.mark.parametrize("name", ["clip", "siglip", "reg", "regmean"])
def test_predict_and_pack_equal_forward(binding, torch_gpu, driver, files, data, tmp_path, name):
    """vit_predict_batch on 9 images and on one; vit_pack_batch (the class-token files) on six images of four shapes, two of them repeated."""
    packs = name in ("clip", "reg")
    lines = [VH.step("predict", n=9, at=0), VH.step("predict", n=1, at=4)] + ([VH.step("pack", n=len(PACK), at=AT_PACK)] if packs else [])
    steps, _ = VH.run(driver, files[name], data, lines, tmp_path / "out")
    ref = _forward(binding, files[name], SQUARE[:9])
    _check_predict(steps[0], ref)
    _check_predict(steps[1], ref[4:5])
    assert steps[1].status["max_batch"] == 9
    if packs:
        _check_predict(steps[2], _pack_forward(binding, files[name], PACK))
        assert steps[2].status["pack"] == 1 and steps[2].status["pack_images"] == len(PACK)


# ------------------------------------------------------------------------------------------------ vit_embed_batch
@pytest.mark.parametrize("name", ["clip", "reg", "siglip"])
def test_embed_equals_feat_read_in_the_documented_order(binding, torch_gpu, driver, files, data, tmp_path, name):
    """Every combination of CLS / MEAN / TOKENS, with and without L2: out[i] = [cls D][mean D][tokens (N - T) D] of feat_read, state.prediction the
    probabilities of the same forward, and the features off again afterwards."""
    combos = [(k, l2) for k in range(1, 8) for l2 in (0, 1)]
    n = 3
    flags = lambda k, l2: ((binding.FEAT_CLS if k & 1 else 0) | (binding.FEAT_MEAN if k & 2 else 0) | (binding.FEAT_TOKENS if k & 4 else 0) | (binding.FEAT_L2 if l2 else 0))
    lines = [VH.step("embed", n=n, at=j % 5, flags=flags(k, l2)) for j, (k, l2) in enumerate(combos)]
    steps, _ = VH.run(driver, files[name], data, lines, tmp_path / "out")
    model = binding.Model(files[name])
    ctx = binding.Context(model, device=0, max_batch=n, dtype=F16)
    last = model.hparams.num_hidden_layers - 1
    for j, ((k, l2), st) in enumerate(zip(combos, steps)):
        ctx.feat_enable(cls=bool(k & 1), mean=bool(k & 2), tokens=bool(k & 4), l2=bool(l2))
        probs = ctx.forward(SQUARE[j % 5:j % 5 + n])
        f = ctx.feat_read(n)[last]
        want = np.concatenate([f[kind].reshape(n, -1) for kind in ("cls", "mean", "tokens") if kind in f], axis=1)
        assert st.rc == 0
        got = st.rows("feat", "<f4")
        assert len(got) == n and all(VH.same(g, w) for g, w in zip(got, want)), (name, k, l2)
        assert VH.same(st.arr("prediction", "<f4"), probs.ravel()), (name, k, l2)
        assert st.heads_off(), st.status
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ vit_zeroshot_batch
@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_zeroshot_gives_topk_of_zeroshot_read(binding, torch_gpu, driver, files, data, tmp_path, family):
    """A softmax (CLIP) and a sigmoid (SigLIP) bank of K = 1, 5, 65 classes; topk -1, 3 and K + 2: out[i] is vitx_topk's order over zeroshot_read's row."""
    n = 4
    model = binding.Model(files[family])
    E = model.hparams.num_classes if family == "clip" else model.hparams.hidden_size
    kind, scale, bias = (binding.ZS_SOFTMAX, ZD.CLIP_SCALE, 0.0) if family == "clip" else (binding.ZS_SIGMOID, ZD.SIGLIP_SCALE, ZD.SIGLIP_BIAS)
    banks = {K: ZD.unit_rows(np.random.default_rng(K).standard_normal((K, E))) for K in (1, 5, 65)}
    for K, b in banks.items():
        data.put(f"bank{K}", b, "<f4")
    cases = [(K, topk) for K in banks for topk in (-1, 3, K + 2)]
    lines = [VH.step("zeroshot", n=n, at=2, topk=topk, bank=f"bank{K}", K=K, E=E, kind=kind, scale=VH.fhex(scale), bias=VH.fhex(bias)) for K, topk in cases]
    steps, _ = VH.run(driver, files[family], data, lines, tmp_path / "out")
    ctx = binding.Context(model, device=0, max_batch=n, dtype=F16)
    for (K, topk), st in zip(cases, steps):
        ctx.zeroshot_set(banks[K], kind, scale, bias)
        probs = ctx.forward(SQUARE[2:2 + n])
        zs = ctx.zeroshot_read(n)
        k = min(topk if topk > 0 else K, K)
        assert st.rc == 0
        rows = st.rows("pairs", VH.PAIR)
        assert [r.size for r in rows] == [k] * n, (K, topk)
        for r, z in zip(rows, zs):
            idx, val = binding.topk(z, k)
            assert r["i"].tolist() == idx and VH.same(r["v"], np.asarray(val, np.float32)), (K, topk)
        assert VH.same(st.arr("prediction", "<f4"), probs.ravel())
        assert st.heads_off(), st.status
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ vit_nn_batch
@pytest.mark.parametrize("name", ["clip", "regmean"])
def test_nn_equals_nn_read(binding, torch_gpu, driver, files, data, tmp_path, name):
    """A gallery of 40 rows, with and without labels, both sources, k = 1 and 5: index, score and vote are nn_read's."""
    n, G, NL = 3, 40, 4
    model = binding.Model(files[name])
    ctx = binding.Context(model, device=0, max_batch=n, dtype=F16)
    rng = np.random.default_rng(7)
    labels = rng.integers(0, NL, G).astype(np.int32)
    data.put("labels", labels, "<i4")
    cases, lines = [], []
    for source in (binding.NN_EMBED, binding.NN_LOGITS):
        E = ctx.nn_width(source)
        if E % 64:
            continue                                  # this file's logits row is no multiple of the GEMMs' K step: the source does not exist for it
        gal = ZD.unit_rows(rng.standard_normal((G, E)))
        data.put(f"gal{source}", gal, "<f4")
        for k in (1, 5):
            for voting in (True, False):
                cases.append((source, gal, k, voting))
                lines.append(VH.step("nn", n=n, at=1, gallery=f"gal{source}", G=G, E=E, k=k, source=source, labels="labels" if voting else None,
                                     n_labels=NL if voting else 0, temperature=VH.fhex(0.07)))
    assert len({c[0] for c in cases}) == (2 if name == "clip" else 1)
    steps, _ = VH.run(driver, files[name], data, lines, tmp_path / "out")
    for (source, gal, k, voting), st in zip(cases, steps):
        ctx.nn_set(gal, k, source, labels if voting else None, NL if voting else 0, 0.07)
        probs = ctx.forward(SQUARE[1:1 + n])
        idx, score, vote = ctx.nn_read(n)
        assert st.rc == 0
        rows = st.rows("nn_pairs", VH.PAIR)
        assert [r.size for r in rows] == [k] * n
        for i, r in enumerate(rows):
            assert r["i"].tolist() == idx[i].tolist() and VH.same(r["v"], score[i]), (source, k, voting, i)
        votes = st.rows("vote", "<f4", counts="vote_counts")
        assert [v.size for v in votes] == [NL if voting else 0] * n
        if voting:
            assert all(VH.same(v, vote[i]) for i, v in enumerate(votes)), (source, k)
        assert VH.same(st.arr("prediction", "<f4"), probs.ravel())
        assert st.heads_off(), st.status
    ctx.close(); model.close()


# ------------------------------------------------------------------------------------------------ vit_dense_batch, vit_depth_batch
def _states(binding, model, n):
    """(script lines that put the state there, the reference context, the images, their first index) of a square and of a rectangular state."""
    yield [], binding.Context(model, device=0, max_batch=n, dtype=F16), SQUARE[:n], 0, (S, S)
    yield [VH.step("set", shape=f"{RECT[0]}x{RECT[1]}")], binding.Context(model, device=0, max_batch=n, dtype=F16, img_shape=RECT), RECTS[:n], AT_RECT, RECT


def test_dense_equals_dense_read(binding, torch_gpu, driver, files, data, tmp_path):
    """One layer and two, bias present and empty, score on and off, out 0 x 0 (the state's shape) and non-square, in a square and in a rectangular
    state: h, w, labels and score are dense_read's."""
    n, K = 3, 21
    model = binding.Model(files["reg"])
    D = model.hparams.hidden_size
    heads = []                                        # (layers, weight, bias or None, score)
    for j, (layers, with_bias, score) in enumerate((([], True, True), ([0, 1], False, False), ([0, 1], True, False), ([0], False, True))):
        _, w, b = DD.exact_head(1, K, D * max(len(layers), 1), seed=j)
        data.put(f"w{j}", w, "<f4"); data.put(f"b{j}", b, "<f4")
        heads.append((layers, w, b if with_bias else None, score))
    lines, checks = [], []
    for setup, ctx, imgs, at, shape in _states(binding, model, n):
        lines += setup
        checks += [None] * len(setup)
        for j, ((layers, w, b, score), (oh, ow)) in enumerate(zip(heads, OUT)):
            lines.append(VH.step("dense", n=n, at=at, weight=f"w{j}", bias=f"b{j}" if b is not None else None, K=K, Dc=w.shape[1], layers=layers, out_h=oh, out_w=ow, score=score))
            ctx.dense_set(w, b, layers or None, (oh, ow) if oh else None, score=score)
            probs = ctx.forward(imgs)
            lab, sc, _ = ctx.dense_read(n)
            checks.append((lab, sc, probs, (oh, ow) if oh else shape))
        ctx.close()
    steps, _ = VH.run(driver, files["reg"], data, lines, tmp_path / "out")
    for st, chk in zip(steps, checks):
        if chk is None:
            continue
        lab, sc, probs, (oh, ow) = chk
        assert st.rc == 0 and lab.shape == (n, oh, ow)
        assert st.arr("hw", "<i4").tolist() == [oh, ow] * n, st.index
        assert st.arr("counts", "<i4").tolist() == [oh * ow, oh * ow if sc is not None else 0] * n, st.index
        assert (st.arr("labels", "u1") == lab.ravel()).all(), st.index
        assert len(np.unique(lab)) > 1
        if sc is not None:
            assert VH.same(st.arr("score", "<f4"), sc.ravel()), st.index
        assert VH.same(st.arr("prediction", "<f4"), probs.ravel())
        assert st.heads_off(), st.status
    model.close()


def test_depth_equals_depth_read(binding, torch_gpu, driver, files, data, tmp_path):
    """With and without the class half, upsample 1 and 4, norm on and off, one layer and two, out 0 x 0 and non-square, in a square and in a
    rectangular state: h, w and depth are depth_read's."""
    n, K = 3, 8
    model = binding.Model(files["reg"])
    D = model.hparams.hidden_size
    bins = PD.bins_ud(K)
    data.put("bins", bins, "<f4")
    heads = []                                        # (layers, wp, wc or None, bias, upsample, norm)
    for j, (layers, with_wc, u, norm) in enumerate((([], True, 4, True), ([0, 1], False, 1, False), ([0, 1], True, 1, False), ([0], False, 4, True))):
        _, _, wp, wc, b = PD.exact_head(1, 1, K, D * max(len(layers), 1), seed=j)
        data.put(f"wp{j}", wp, "<f4"); data.put(f"wc{j}", wc, "<f4"); data.put(f"b{j}", b, "<f4")
        heads.append((layers, wp, wc if with_wc else None, b, u, norm))
    lines, checks = [], []
    for setup, ctx, imgs, at, shape in _states(binding, model, n):
        lines += setup
        checks += [None] * len(setup)
        for j, ((layers, wp, wc, b, u, norm), (oh, ow)) in enumerate(zip(heads, OUT)):
            lines.append(VH.step("depth", n=n, at=at, wp=f"wp{j}", wc=f"wc{j}" if wc is not None else None, bias=f"b{j}", bins="bins", K=K, Dc=wp.shape[1], layers=layers,
                                 upsample=u, min_depth=VH.fhex(0.001), max_depth=VH.fhex(10.0), norm=norm, out_h=oh, out_w=ow))
            ctx.depth_set(wp, wc, b, bins, layers or None, u, 0.001, 10.0, (oh, ow) if oh else None, norm=norm)
            probs = ctx.forward(imgs)
            checks.append((ctx.depth_read(n)[0], probs, (oh, ow) if oh else shape))
        ctx.close()
    steps, _ = VH.run(driver, files["reg"], data, lines, tmp_path / "out")
    for st, chk in zip(steps, checks):
        if chk is None:
            continue
        dm, probs, (oh, ow) = chk
        assert st.rc == 0 and dm.shape == (n, oh, ow)
        assert st.arr("hw", "<i4").tolist() == [oh, ow] * n, st.index
        assert st.arr("counts", "<i4").tolist() == [oh * ow] * n, st.index
        assert VH.same(st.arr("depth", "<f4"), dm.ravel()), st.index
        assert not VH.same(dm[0], dm[1])
        assert VH.same(st.arr("prediction", "<f4"), probs.ravel())
        assert st.heads_off(), st.status
    model.close()


# ------------------------------------------------------------------------------------------------ vit_text_embed_batch
def _text(binding, path, ids, l2, dtype=F16):
    model = binding.Model(path)
    t = binding.TextContext(model, max_prompts=len(ids), dtype=dtype)
    out = t.embed(ids, l2=l2)
    t.close(); model.close()
    return out


@pytest.mark.parametrize("family", ["clip", "siglip"])
def test_text_embed_equals_the_text_context(pkg, binding, torch_gpu, driver, data, tmp_path, family):
    """Flags 0 and VITX_TEXT_L2, 1 prompt and 17."""
    path = TD.text_file(pkg, family)
    ids = TD.prompts(family)
    data.put("ids", ids, "<i4")
    cases = [(1, 0), (17, binding.TEXT_L2), (17, 0), (1, binding.TEXT_L2)]
    steps, _ = VH.run(driver, path, data, [VH.step("text", n=n, flags=fl, ids="ids") for n, fl in cases], tmp_path / "out")
    for (n, fl), st in zip(cases, steps):
        want = _text(binding, path, ids[:n], bool(fl))
        assert st.rc == 0
        rows = st.rows("text", "<f4")
        assert len(rows) == n and all(VH.same(r, w) for r, w in zip(rows, want)), (n, fl)
    assert [st.status["text_max_prompts"] for st in steps] == [1, 17, 17, 17]


# ------------------------------------------------------------------------------------------------ the state cache
def _head_steps(binding, data, model, n, at=0):
    """One step of every opt-in output on `model`'s file (widths from the file): dense, depth, zeroshot, nn, embed."""
    D, C = model.hparams.hidden_size, model.hparams.num_classes
    _, w, b = DD.exact_head(1, 5, D, seed=1)
    _, _, wp, wc, db = PD.exact_head(1, 1, 6, D, seed=2)
    rng = np.random.default_rng(3)
    data.put("cw", w, "<f4"); data.put("cb", b, "<f4"); data.put("cwp", wp, "<f4"); data.put("cwc", wc, "<f4"); data.put("cdb", db, "<f4")
    data.put("cbins", PD.bins_ud(6), "<f4"); data.put("cbank", ZD.unit_rows(rng.standard_normal((5, C))), "<f4"); data.put("cgal", ZD.unit_rows(rng.standard_normal((12, D))), "<f4")
    return [VH.step("dense", n=n, at=at, weight="cw", bias="cb", K=5, Dc=D, score=1),
            VH.step("depth", n=n, at=at, wp="cwp", wc="cwc", bias="cdb", bins="cbins", K=6, Dc=D, upsample=2, min_depth=VH.fhex(0.001), max_depth=VH.fhex(10.0)),
            VH.step("zeroshot", n=n, at=at, topk=3, bank="cbank", K=5, E=C, kind=0, scale=VH.fhex(100.0), bias=VH.fhex(0.0)),
            VH.step("nn", n=n, at=at, gallery="cgal", G=12, E=D, k=2, source=binding.NN_EMBED, temperature=VH.fhex(0.07)),
            VH.step("embed", n=n, at=at, flags=binding.FEAT_CLS | binding.FEAT_TOKENS)]


def test_every_head_is_off_after_its_call(binding, torch_gpu, driver, files, data, tmp_path):
    """(a) predict, dense, depth, zeroshot, nn, embed, predict on one state: every call succeeds and returns something, every head reads "off" after
    its step, and the two predicts give the same bits -- those of a context that never had a head."""
    model = binding.Model(files["clip"])
    lines = [VH.step("predict", n=3)] + _head_steps(binding, data, model, 3) + [VH.step("predict", n=3)]
    model.close()
    steps, _ = VH.run(driver, files["clip"], data, lines, tmp_path / "out")
    ref = _forward(binding, files["clip"], SQUARE[:3])
    for st in steps:
        assert st.rc == 0 and st.heads_off(), (st.op, st.status)
        assert st.arr("counts", "<i4").size > 0, st.op
    _check_predict(steps[0], ref)
    _check_predict(steps[-1], ref)


def test_the_capacity_grows_once_and_never_shrinks(binding, torch_gpu, driver, files, data, tmp_path):
    """(b) predict 2, 9, 2."""
    steps, _ = VH.run(driver, files["clip"], data, [VH.step("predict", n=2), VH.step("predict", n=9, at=3), VH.step("predict", n=2, at=1)], tmp_path / "out")
    assert [st.status["max_batch"] for st in steps] == [2, 9, 9]
    _check_predict(steps[0], _forward(binding, files["clip"], SQUARE[:2]))
    _check_predict(steps[1], _forward(binding, files["clip"], SQUARE[3:12]))
    _check_predict(steps[2], _forward(binding, files["clip"], SQUARE[1:3]))


def test_a_reloaded_or_another_model_gets_a_fresh_context(binding, torch_gpu, driver, files, data, tmp_path):
    """(c) reload between two predicts, then a second file loaded into the same vit_model: the results are the new model's.  (The second file has the
    larger class count, so state.prediction holds whatever a stale context would write.)"""
    a, b = files["reg"], files["clip"]
    ma, mb = binding.Model(a), binding.Model(b)
    assert ma.num_classes <= mb.num_classes
    ma.close(); mb.close()
    lines = [VH.step("predict", n=3), VH.step("reload"), VH.step("predict", n=3), VH.step("reload", path=b), VH.step("predict", n=3), VH.step("pack", n=2, at=AT_PACK),
             VH.step("reload", path=a), VH.step("pack", n=2, at=AT_PACK)]
    steps, _ = VH.run(driver, a, data, lines, tmp_path / "out")
    ref_a, ref_b = _forward(binding, a, SQUARE[:3]), _forward(binding, b, SQUARE[:3])
    assert ref_a.shape != ref_b.shape or not VH.same(ref_a, ref_b)
    assert steps[1].rc == 0 and steps[3].rc == 0 and steps[6].rc == 0
    _check_predict(steps[0], ref_a)
    _check_predict(steps[2], ref_a)
    _check_predict(steps[4], ref_b)
    _check_predict(steps[5], _pack_forward(binding, b, PACK[:2]))
    _check_predict(steps[7], _pack_forward(binding, a, PACK[:2]))


def test_a_change_of_geometry_replaces_the_context(binding, torch_gpu, driver, files, data, tmp_path):
    """(d) set img_size, set pos_interp on the resized state, set shape, and back to the file's own: bits equal a fresh binding.Context of that geometry."""
    path = files["clip"]
    AA = binding.POS_BICUBIC_AA
    lines = [VH.step("predict", n=2),
             VH.step("set", img_size=SMALL), VH.step("predict", n=2, at=AT_SMALL),
             VH.step("set", pos_interp=AA), VH.step("predict", n=2, at=AT_SMALL),
             VH.step("set", img_size=0, shape=f"{RECT[0]}x{RECT[1]}"), VH.step("predict", n=2, at=AT_RECT),
             VH.step("set", pos_interp=binding.POS_BICUBIC), VH.step("predict", n=2, at=AT_RECT),
             VH.step("set", shape="0x0"), VH.step("predict", n=2)]
    steps, _ = VH.run(driver, path, data, lines, tmp_path / "out")
    own = _forward(binding, path, SQUARE[:2])
    small = _forward(binding, path, SMALLS[:2], img_size=SMALL, pos_interp=binding.POS_BICUBIC)
    small_aa = _forward(binding, path, SMALLS[:2], img_size=SMALL, pos_interp=AA)
    rect_aa = _forward(binding, path, RECTS[:2], img_shape=RECT, pos_interp=AA)
    rect = _forward(binding, path, RECTS[:2], img_shape=RECT, pos_interp=binding.POS_BICUBIC)
    assert not VH.same(small, small_aa) and not VH.same(rect, rect_aa), "the two conventions must differ for the test to see a stale context"
    for i, want, shape in ((0, own, (S, S)), (2, small, (SMALL, SMALL)), (4, small_aa, (SMALL, SMALL)), (6, rect_aa, RECT), (8, rect, RECT), (10, own, (S, S))):
        _check_predict(steps[i], want)
        assert (steps[i].status["img_h"], steps[i].status["img_w"]) == shape, i


def test_a_change_of_dtype_replaces_the_contexts(binding, torch_gpu, driver, files, data, tmp_path):
    """(e) predict, set dtype=bf16, predict, pack, set dtype=f16, pack, predict: every result is the reference of the dtype set at that moment."""
    path = files["clip"]
    lines = [VH.step("predict", n=3), VH.step("set", dtype=BF16), VH.step("predict", n=3), VH.step("pack", n=3, at=AT_PACK),
             VH.step("set", dtype=F16), VH.step("pack", n=3, at=AT_PACK), VH.step("predict", n=3)]
    steps, _ = VH.run(driver, path, data, lines, tmp_path / "out")
    f16, bf16 = _forward(binding, path, SQUARE[:3], F16), _forward(binding, path, SQUARE[:3], BF16)
    assert not VH.same(f16, bf16)
    _check_predict(steps[0], f16)
    _check_predict(steps[2], bf16)
    _check_predict(steps[3], _pack_forward(binding, path, PACK[:3], BF16))
    _check_predict(steps[5], _pack_forward(binding, path, PACK[:3], F16))
    _check_predict(steps[6], f16)


def test_a_change_of_text_dtype_replaces_the_text_context(pkg, binding, torch_gpu, driver, data, tmp_path):
    """(f) text, set text_dtype=bf16, text, set text_dtype=f16, text."""
    path = TD.text_file(pkg, "clip")
    ids = TD.prompts("clip")[:3]
    data.put("ids", ids, "<i4")
    t = VH.step("text", n=3, flags=0, ids="ids")
    steps, _ = VH.run(driver, path, data, [t, VH.step("set", text_dtype=BF16), t, VH.step("set", text_dtype=F16), t], tmp_path / "out")
    f16, bf16 = _text(binding, path, ids, False, F16), _text(binding, path, ids, False, BF16)
    assert not VH.same(f16, bf16)
    for i, want in ((0, f16), (2, bf16), (4, f16)):
        assert steps[i].rc == 0
        assert VH.same(np.concatenate(steps[i].rows("text", "<f4")), want.ravel()), i


def test_a_device_that_does_not_exist_is_refused_after_a_successful_call(pkg, binding, torch_gpu, driver, files, data, tmp_path):
    """(g) set device=<device count> after a call that worked: the next predict, pack and text call return 1 with a message -- none answers from the
    context of device 0 -- and the state works again once the device is put back."""
    ndev = torch_gpu.cuda.device_count()
    path = files["clip"]
    lines = [VH.step("predict", n=2), VH.step("pack", n=2, at=AT_PACK), VH.step("set", device=ndev), VH.step("predict", n=2), VH.step("pack", n=2, at=AT_PACK),
             VH.step("set", device=0), VH.step("predict", n=2), VH.step("pack", n=2, at=AT_PACK)]
    steps, err = VH.run(driver, path, data, lines, tmp_path / "out")
    ref, pref = _forward(binding, path, SQUARE[:2]), _pack_forward(binding, path, PACK[:2])
    _check_predict(steps[0], ref); _check_predict(steps[1], pref)
    _check_refused(steps[3]); _check_refused(steps[4])
    assert err.count(f"device {ndev} out of range") == 2, err[-2000:]
    _check_predict(steps[6], ref); _check_predict(steps[7], pref)

    tpath = TD.text_file(pkg, "clip")
    ids = TD.prompts("clip")[:2]
    data.put("ids", ids, "<i4")
    t = VH.step("text", n=2, flags=0, ids="ids")
    steps, err = VH.run(driver, tpath, data, [t, VH.step("set", text_device=ndev), t, VH.step("set", text_device=0), t], tmp_path / "out_text")
    want = _text(binding, tpath, ids, False)
    assert steps[0].rc == 0 and VH.same(np.concatenate(steps[0].rows("text", "<f4")), want.ravel())
    assert steps[2].rc == 1 and steps[2].arr("counts", "<i4").size == 0 and f"device {ndev} out of range" in err
    assert steps[4].rc == 0 and VH.same(np.concatenate(steps[4].rows("text", "<f4")), want.ravel())


# ------------------------------------------------------------------------------------------------ refused calls
def test_refused_calls_leave_the_state_usable(binding, torch_gpu, driver, files, data, tmp_path):
    """A dense head whose Dc is not the model's, a bank of the wrong width, k = 0, a wrong-sized image for vit_embed_batch, an image model for
    vit_text_embed_batch: each returns 1 with empty output and a message, leaves no head on, and the next predict gives the reference bits."""
    path = files["clip"]
    model = binding.Model(path)
    D, C = model.hparams.hidden_size, model.hparams.num_classes
    model.close()
    rng = np.random.default_rng(5)
    _, w, b = DD.exact_head(1, 5, D // 2, seed=1)
    data.put("w", w, "<f4"); data.put("b", b, "<f4")
    data.put("bank", ZD.unit_rows(rng.standard_normal((5, C // 2))), "<f4")
    data.put("gal", ZD.unit_rows(rng.standard_normal((12, D))), "<f4")
    data.put("ids", TD.prompts("clip")[:1], "<i4")
    refused = [VH.step("dense", n=3, weight="w", bias="b", K=5, Dc=D // 2),
               VH.step("zeroshot", n=3, bank="bank", K=5, E=C // 2, kind=0, scale=VH.fhex(100.0), bias=VH.fhex(0.0)),
               VH.step("nn", n=3, gallery="gal", G=12, E=D, k=0, source=binding.NN_EMBED),
               VH.step("embed", n=1, at=AT_RECT, flags=binding.FEAT_CLS),
               VH.step("text", n=1, flags=0, ids="ids")]
    lines = [VH.step("predict", n=3)]
    for r in refused:
        lines += [r, VH.step("predict", n=3)]
    steps, err = VH.run(driver, path, data, lines, tmp_path / "out")
    ref = _forward(binding, path, SQUARE[:3])
    for i, st in enumerate(steps):
        if i % 2 == 0:
            _check_predict(st, ref)
        else:
            _check_refused(st)
    for who in ("vit_dense_batch: ", "vit_zeroshot_batch: ", "vit_nn_batch: ", "vit_embed_batch: image 0 is", "vit_text_embed_batch: this is an image model"):
        assert who in err, (who, err[-3000:])
    assert steps[-2].status["text"] == 0
