"""tests/cpp/vit_h_driver.cpp builds and links against vit.cpp_amd/vit.h and libvitx.so, and the argument checks of vit.h's batch entry points that
return before any device call return 1 -- with empty output and no context -- on a machine without a GPU, after a host-only vit_model_load."""
import numpy as np
import pytest

import dense_data as DD
import depth_data as PD
import text_data as TD
import vit_h_data as VH
import zs_data as ZD


@pytest.fixture(scope="module")
def driver(binding, tmp_path_factory):
    return VH.build_driver(tmp_path_factory.mktemp("vit_h_driver"))


def test_argument_checks_return_1_before_any_device_call(pkg, binding, driver, tmp_path):
    path = ZD.model_file(pkg, "clip")
    model = binding.Model(path)
    D, C, S = model.hparams.hidden_size, model.hparams.num_classes, model.img_size
    model.close()
    rng = np.random.default_rng(0)
    imgs = list(ZD.images()[:2]) + [np.zeros((30, 30, 3), np.float32)]          # image 2: no multiple of the patch size, and not the state's shape
    data = VH.Data(tmp_path / "data", imgs)
    K = 5
    _, w, b = DD.exact_head(1, K, D, seed=0)
    _, _, wp, wc, db = PD.exact_head(1, 1, K, D, seed=0)
    data.put("w", w, "<f4"); data.put("b", b, "<f4"); data.put("w_short", w.ravel()[:-1], "<f4"); data.put("b_long", np.zeros(K + 1), "<f4")
    data.put("wp", wp, "<f4"); data.put("wc", wc, "<f4"); data.put("wc_short", wc.ravel()[:-1], "<f4"); data.put("db", db, "<f4")
    data.put("bins", PD.bins_ud(K), "<f4"); data.put("bins_short", PD.bins_ud(K - 1), "<f4")
    data.put("bank", ZD.unit_rows(rng.standard_normal((K, C))), "<f4")
    data.put("gal", ZD.unit_rows(rng.standard_normal((12, D))), "<f4"); data.put("labels_short", np.zeros(11), "<i4")
    data.put("ids", TD.prompts("clip")[:1], "<i4")
    dense = dict(n=1, weight="w", bias="b", K=K, Dc=D)
    depth = dict(n=1, wp="wp", wc="wc", bias="db", bins="bins", K=K, Dc=D)
    zs = dict(n=1, bank="bank", K=K, E=C, kind=0)
    nn = dict(n=1, gallery="gal", G=12, E=D, k=2, source=1)
    lines = [VH.step("predict", n=0), VH.step("pack", n=0), VH.step("pack", n=1, at=2), VH.step("embed", n=0, flags=1), VH.step("embed", n=1, flags=0),
             VH.step("embed", n=1, at=2, flags=1),
             VH.step("zeroshot", **{**zs, "n": 0}), VH.step("zeroshot", **{**zs, "K": 0}), VH.step("zeroshot", **{**zs, "K": K - 1}), VH.step("zeroshot", **{**zs, "at": 2}),
             VH.step("nn", **{**nn, "n": 0}), VH.step("nn", **{**nn, "G": 0}), VH.step("nn", **{**nn, "G": 11}), VH.step("nn", **nn, labels="labels_short", n_labels=2),
             VH.step("nn", **{**nn, "at": 2}),
             VH.step("dense", **{**dense, "n": 0}), VH.step("dense", **{**dense, "K": 0}), VH.step("dense", **{**dense, "weight": "w_short"}),
             VH.step("dense", **{**dense, "bias": "b_long"}), VH.step("dense", **dense, layers=[64]), VH.step("dense", **dense, layers=[-1]), VH.step("dense", **{**dense, "at": 2}),
             VH.step("depth", **{**depth, "n": 0}), VH.step("depth", **{**depth, "K": -1}), VH.step("depth", **{**depth, "bins": "bins_short"}),
             VH.step("depth", **{**depth, "wc": "wc_short"}), VH.step("depth", **depth, layers=[0, 64]), VH.step("depth", **{**depth, "at": 2}),
             VH.step("text", n=0, flags=0, ids="ids"), VH.step("text", n=1, flags=0, ids="ids")]
    steps, err = VH.run(driver, path, data, lines, tmp_path / "out")
    for st, ln in zip(steps, lines):
        assert st.rc == 1, ln
        assert st.arr("counts", "<i4").size == 0, ln
        assert st.status["ctx"] == 0 and st.status["pack"] == 0 and st.status["text"] == 0, ln
    for who in ("vit_predict_batch", "vit_pack_batch", "vit_embed_batch", "vit_zeroshot_batch", "vit_nn_batch", "vit_dense_batch", "vit_depth_batch", "vit_text_embed_batch"):
        assert who + ": " in err, who
    assert "layer 64 outside 0 .. 63" in err and "layer -1 outside 0 .. 63" in err


def test_a_script_step_the_driver_does_not_know_is_an_error_of_the_run(pkg, binding, driver, tmp_path):
    """The helper fails a run whose child exits non-zero (here: status 2 for an unknown step), with the child's message."""
    data = VH.Data(tmp_path / "data", list(ZD.images()[:1]))
    with pytest.raises(AssertionError, match="unknown op 'frobnicate'"):
        VH.run(driver, ZD.model_file(pkg, "clip"), data, ["frobnicate n=1"], tmp_path / "out")
