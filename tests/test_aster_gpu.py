"""The ASTER recogniser on the GPU against what the reference itself computed on the same weights and images
(tests/golden/aster_e2e.npz, tools/gen_golden_aster.py): the two new front kernels, the STN head, the encoder, the decoder on the
encoder's features, `ASTER.read` / `forward`, and `io.evaluate(recognizer=<ASTER>)`.

Error bars: 4 x the distance of the reference's own fp32 result from its float64 run (recorded in the fixture as err_*) + 1e-7 x the
largest value -- the rule of the project's other float64 comparisons.  For a stage fed with the RECORDED fp32 input of the reference the
unit is the reference's error at that input (err_stn_in, err_rect_at_src); for a stage behind our own front it is the error of the
reference's whole chain up to there (err_ctrl, err_rect, err_feats)."""
import os

import numpy as np
import pytest
import torch

import tatt_amd
from tatt_amd import aster, io

import aster_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
KW = dict(arch="ResNet_ASTER", rec_num_classes=97, sDim=512, attDim=512, max_len_labels=100, eos=94, STN_ON=True)


@pytest.fixture(scope="module")
def e2e():
    return np.load(os.path.join(GOLD, "aster_e2e.npz"))


@pytest.fixture(scope="module")
def model(e2e):
    m = R.e2e_model(tatt_amd.ASTER, **KW)
    with torch.no_grad():      # the TPS kernel inverse comes out of LAPACK (machine-dependent last bits): the recorded one, as from a checkpoint
        m.tps.inverse_kernel.copy_(torch.from_numpy(e2e["tps_inverse_kernel"]))
    return m.to(DEV).eval()


def _bar(e2e, name, ref):
    return 4.0 * float(e2e["err_" + name]) + 1e-7 * float(np.abs(ref).max())


def _err(got, want):
    return float(np.abs(got.detach().cpu().numpy().astype(np.float64) - want).max())


def test_resize_bilinear_ac(e2e):
    img = torch.from_numpy(e2e["images"][:2]).to(DEV)
    assert tuple(img.shape) == (2, 3, 32, 128)
    got = aster.resize_bilinear_ac(img, (32, 64))
    err, bar = _err(got, e2e["stn_in"][:2]), _bar(e2e, "stn_in", e2e["stn_in"])
    print("resize_bilinear_ac: %.3e (bar %.3e)" % (err, bar))
    assert err <= bar
    # a strided view (the eval loop hands over images[:, :3] of four-plane tensors)
    four = torch.cat([img, img[:, :1]], 1)
    assert _err(aster.resize_bilinear_ac(four[:, :3], (32, 64)), e2e["stn_in"][:2]) <= bar
    same = aster.resize_bilinear_ac(img, (32, 128))                  # align_corners: the identity at equal sizes
    assert _err(same, e2e["images"][:2]) <= 1e-6


def test_grid_sample_sized(e2e):
    img = torch.from_numpy(e2e["images"][:2]).to(DEV)
    src = torch.from_numpy(e2e["src"][:2]).to(DEV).contiguous()
    got = aster.grid_sample_sized(img, src, (32, 100)).permute(0, 3, 1, 2)
    err, bar = _err(got, e2e["rect"][:2]), _bar(e2e, "rect_at_src", e2e["rect"])
    print("grid_sample_sized at the recorded grid: %.3e (bar %.3e)" % (err, bar))
    assert err <= bar


def test_control_points_and_rectification(model, e2e):
    img = torch.from_numpy(e2e["images"]).to(DEV)
    with torch.no_grad():
        ctrl = model.control_points(img)
        rect = model.rectify(img).permute(0, 3, 1, 2)
    err_c, err_r = _err(ctrl, e2e["ctrl"]), _err(rect, e2e["rect"])
    print("control points %.3e (bar %.3e), rectified image %.3e (bar %.3e)" % (err_c, _bar(e2e, "ctrl", e2e["ctrl"]), err_r,
                                                                                 _bar(e2e, "rect", e2e["rect"])))
    assert np.abs(e2e["ctrl"][0] - e2e["ctrl"][1]).max() > 1e-3          # (the fixture's images do get control points of their own)
    assert err_c <= _bar(e2e, "ctrl", e2e["ctrl"])
    assert err_r <= _bar(e2e, "rect", e2e["rect"])


def test_encoder_features(model, e2e):
    img = torch.from_numpy(e2e["images"]).to(DEV)
    rect = torch.from_numpy(e2e["rect"]).to(DEV)
    with torch.no_grad():
        on_recorded = model.encode(rect.permute(0, 2, 3, 1))
        whole = model.features(img)
    assert tuple(whole.shape) == (3, 25, 512)
    bar = _bar(e2e, "feats", e2e["feats"])
    e1, e2 = _err(on_recorded, e2e["feats"]), _err(whole, e2e["feats"])
    print("encoder features: on the recorded rectified image %.3e, from the images %.3e (bar %.3e, reference fp32 %.3e)"
          % (e1, e2, bar, float(e2e["err_feats"])))
    assert np.abs(e2e["feats"][0] - e2e["feats"][1]).max() > 1e-2       # (features that depend on the image)
    assert e1 <= bar
    assert e2 <= bar
    tatt_amd.sync_check()


def test_decoder_on_recorded_features(model, e2e):
    feats = torch.from_numpy(e2e["feats"]).to(DEV)
    tg = torch.ones(3, 100, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        lg = model.decode(feats, "forced", tg)
    bar, need = R.margin_bound(e2e["err_forced"], e2e["forced_maxabs"])
    want = R.forced(R.decoder_params(model.state_dict()), e2e["feats"], np.ones((3, 100), dtype=np.int64))
    err = _err(lg, want)
    print("forced logits on the recorded features: %.3e against float64 (bar %.3e, reference fp32 %.3e)" % (err, bar, float(e2e["err_forced"])))
    assert err <= bar
    assert (e2e["greedy_margin"] > need).all() and (e2e["beam_margin"] > need).all()
    with torch.no_grad():
        g_ids, g_scores = model.decode(feats, "greedy")
        b_ids, _ = model.decode(feats, "beam")
    assert R.upto_eos(g_ids.cpu().numpy(), 94) == R.upto_eos(e2e["greedy_ids"], 94)
    assert R.upto_eos(b_ids.cpu().numpy(), 94) == R.upto_eos(e2e["beam_ids"], 94)
    for r, row in enumerate(R.upto_eos(e2e["greedy_ids"], 94)):
        assert np.abs(g_scores[r, :len(row)].cpu().numpy() - e2e["greedy_scores"][r, :len(row)]).max() <= bar


def test_read_end_to_end(model, e2e):
    info = aster.AsterInfo("all")
    img = torch.from_numpy(e2e["images"]).to(DEV)
    before = aster.LAUNCHES["one_launch"]
    ids, scores = model.read(img, "beam")
    assert aster.LAUNCHES["one_launch"] == before + 1                    # the product path is the one launch
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (3, 100) and scores.dtype == torch.float32
    assert aster.get_string_aster(ids, info) == [str(s) for s in e2e["strings"]]
    assert R.upto_eos(ids.cpu().numpy(), 94) == R.upto_eos(e2e["beam_ids"], 94)
    g_ids, _ = model.read(img, "greedy")
    rows = R.upto_eos(e2e["greedy_ids"], 94)
    assert R.upto_eos(g_ids.cpu().numpy(), 94) == rows
    # the fixture's three beam rows are equal (random decoder weights follow their own output far more than the image), so the mapping
    # of images to rows is pinned with the greedy rows, which differ: a permuted batch gives the permuted rows
    assert len({tuple(r) for r in rows}) == 3
    perm = [2, 0, 1]
    p_ids, _ = model.read(img[perm].contiguous(), "greedy")
    assert R.upto_eos(p_ids.cpu().numpy(), 94) == [rows[i] for i in perm]
    pb_ids, _ = model.read(img[perm].contiguous(), "beam")
    assert R.upto_eos(pb_ids.cpu().numpy(), 94) == [R.upto_eos(e2e["beam_ids"], 94)[i] for i in perm]
    out = model({"images": img, "rec_targets": None, "rec_lengths": None})
    assert out["losses"] == {} and torch.equal(out["output"]["pred_rec"], ids) and bool((out["output"]["pred_rec_score"] == 1).all())
    tatt_amd.sync_check()


def test_evaluate_with_aster(model, monkeypatch):
    info = aster.AsterInfo("all")
    torch.manual_seed(5)
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=1, hidden_units=32).to(DEV).eval()
    g = torch.Generator().manual_seed(8)
    batches = [(torch.rand(3, 4, 16, 64, generator=g).to(DEV), torch.rand(3, 4, 32, 128, generator=g).to(DEV)) for _ in range(2)]
    # what the recogniser reads, computed here from the same calls: the labels are made from it (some right, some wrong)
    strings = {"sr": [], "lr": [], "hr": []}
    with torch.no_grad():
        for lr, hr in batches:
            sr = gen(lr)
            sr = sr[0] if isinstance(sr, tuple) else sr
            for name, im in (("sr", sr), ("lr", lr), ("hr", hr)):
                strings[name] += aster.get_string_aster(model.read(aster.parse_aster_data(im[:, :3]), "beam")[0], info)
    labels = [strings["sr"][0], "zz9", strings["lr"][2], strings["hr"][3], strings["sr"][4], "nothing"]
    full = [(lr, hr, None, labels[3 * i:3 * i + 3]) for i, (lr, hr) in enumerate(batches)]
    want = {k: round(sum(io.str_filt(p, "lower") == io.str_filt(t, "lower") for p, t in zip(strings[k], labels)) / 6, 4) for k in strings}
    torch.cuda.synchronize()
    count = {"n": 0}
    for meth in ("cpu", "item", "tolist", "numpy", "__float__", "__int__", "__bool__"):
        orig = getattr(torch.Tensor, meth)

        def wrapped(self, *a, _orig=orig, **k):
            if self.is_cuda:
                count["n"] += 1
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, meth, wrapped)
    res = io.evaluate(gen, full, recognizer=model, full_metrics=True)
    monkeypatch.undo()
    assert count["n"] == 1, "io.evaluate read the device %d times" % count["n"]
    assert res["n_images"] == 6 and res["n_batches"] == 2
    assert (res["accuracy"], res["accuracy_lr"], res["accuracy_hr"]) == (want["sr"], want["lr"], want["hr"])
    assert res["accuracy"] >= round(2 / 6, 4)
    for k in ("psnr", "ssim", "psnr_lr", "ssim_lr", "ned", "ned_lr", "ned_hr", "ned_skipped"):
        assert k in res and np.isfinite(res[k])
    crnn_keys = {"psnr", "ssim", "n_batches", "psnr_lr", "ssim_lr", "accuracy", "accuracy_lr", "accuracy_hr", "n_images", "ned", "ned_lr",
                 "ned_hr", "ned_skipped"}
    assert set(res) == crnn_keys
    tatt_amd.sync_check()
