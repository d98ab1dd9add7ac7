"""Golden data of the ASTER recogniser, recorded from the reference's own modules (imported through tools/_ref_import.py, with
`Tensor.cuda` patched to the identity: the reference's decoder hard-wires `.cuda()`).  Runs where the reference is, beside
tools/gen_golden.py; the tests never import the reference.

  tests/golden/aster_decode.npz  the decoder alone (C = 39, eos = 36, seed-1 weights with fc.weight x 30, randn features):
                                 recorded greedy ids / scores and beam ids of 8 rows, the float64 margins of tests/aster_ref.py, and per
                                 forced case the error of the reference's fp32 decoder against float64 (the unit of the GPU error bar)
  tests/golden/aster_e2e.npz     the whole recogniser (97 classes; seeds, `perturb`, fc.weight x 30 and the EOS shift: tests/aster_ref.py) on 3 images: STN input, control
                                 points, sampling grid, rectified image, encoder features, forced logits, greedy ids / scores, beam ids,
                                 the float64 versions' distance (the unit of the error bars), margins, and init checksums
  tests/golden/attn_decode_limits.npz (the `aster_*` entries; `--limits` writes these alone)
                                 the decoder at the widest geometry its one launch takes (T = 32, C = 128): per case the reference's
                                 fp32 error against float64 and the largest |logit|, and the feature seed of the greedy / beam case
No weights are stored (84 MB): the tests rebuild them from the seeds.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from _ref_import import import_reference            # noqa: E402
import aster_ref as R                               # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CHECK_KEYS = ["encoder.layer0.0.weight", "encoder.layer3.2.conv2.weight", "encoder.rnn.weight_hh_l1_reverse",
              "decoder.decoder.attention_unit.sEmbed.weight", "decoder.decoder.gru.weight_ih_l0", "decoder.decoder.fc.bias",
              "stn_head.stn_convnet.4.0.weight", "stn_head.stn_fc1.0.weight"]


def images(B, seed=R.IMG_SEED):
    """smooth seeded images in [-1, 1]: low-resolution noise enlarged bilinearly, so that sampling positions matter"""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(B, 3, 8, 32, generator=g)
    return torch.nn.functional.interpolate(low, (32, 128), mode="bilinear", align_corners=False) * 2 - 1


# the widest geometries: (B, L, C, T) of the forced and of the greedy / beam case, its EOS, the forced case's feature seed
LIMIT_FORCED, LIMIT_DECODE, LIMIT_EOS, LIMIT_FORCED_SEED = (2, 3, 128, 32), (2, 6, 128, 32), 125, 1


def limit_inputs(case, seed):
    B, L, C, T = case
    return R.features(B, T, seed), torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(seed))


def merge_limits(entries):
    """tests/golden/attn_decode_limits.npz is shared with tools/gen_golden_moran.py: replace this generator's entries, keep the others"""
    path = os.path.join(GOLD, "attn_decode_limits.npz")
    out = dict(np.load(path)) if os.path.exists(path) else {}
    out.update(entries)
    np.savez_compressed(path, **out)


def limits(RefHead):
    C = LIMIT_FORCED[2]
    head = R.make_head(R.HEAD_SEED, C)
    ref = RefHead(C, 512, 512, 512, 100)
    ref.load_state_dict(head.state_dict())
    P = R.decoder_params(head.state_dict(), "decoder.")

    def ref_err(case, seed):
        x, tg = limit_inputs(case, seed)
        want = R.forced(P, x.numpy(), tg.numpy())
        return np.abs(ref([x, tg, [case[1]] * case[0]]).numpy() - want).max(), np.abs(want).max()

    fe, fm = ref_err(LIMIT_FORCED, LIMIT_FORCED_SEED)
    for seed in range(1, 100):      # the first feature seed at which every row's greedy and beam margin exceeds the bound
        de, dm = ref_err(LIMIT_DECODE, seed)
        _, need = R.margin_bound(max(fe, de), max(fm, dm))
        x = limit_inputs(LIMIT_DECODE, seed)[0].numpy()
        g_ids, _, gm = R.greedy(P, x, LIMIT_DECODE[1], LIMIT_EOS)
        b_ids, bm = R.beam(P, x, LIMIT_DECODE[1], LIMIT_EOS)
        print("limits: seed", seed, "bound %.3e" % need, "greedy margins", gm, "beam margins", bm)
        if (gm > need).all() and (bm > need).all():
            break
    else:
        raise AssertionError("no feature seed below 100 clears the margin bound")
    print("limits: forced reference fp32 error %.3e at max|logit| %.2f, decode %.3e at %.2f, seed %d" % (fe, fm, de, dm, seed))
    print("limits: greedy", R.upto_eos(g_ids, LIMIT_EOS), "beam", R.upto_eos(b_ids, LIMIT_EOS))
    merge_limits({"aster_forced_case": np.array(LIMIT_FORCED + (LIMIT_FORCED_SEED,)), "aster_forced_ref_err": np.array(fe),
                  "aster_forced_maxabs": np.array(fm), "aster_decode_case": np.array(LIMIT_DECODE + (seed, LIMIT_EOS)),
                  "aster_decode_ref_err": np.array(de), "aster_decode_maxabs": np.array(dm)})


def main():
    import_reference()
    import types
    sys.modules.setdefault("editdistance", types.ModuleType("editdistance"))      # (imported by utils/metrics.py, unused here)
    torch.Tensor.cuda = lambda self, *a, **k: self
    from model.recognizer.recognizer_builder import RecognizerBuilder
    from model.recognizer.attention_recognition_head import AttentionRecognitionHead as RefHead
    import tatt_amd
    torch.set_grad_enabled(False)
    limits(RefHead)
    if "--limits" in sys.argv[1:]:
        return

    # ---- the decoder alone ------------------------------------------------------------------------------------------------------------
    out = {}
    errs, maxabs = [], []
    for i, (B, L, C, T) in enumerate(R.FORCED_CASES):
        head = R.make_head(R.HEAD_SEED, C)
        torch.manual_seed(R.HEAD_SEED)
        ref = R.scale_fc(RefHead(C, 512, 512, 512, 100))
        for k, v in head.state_dict().items():
            assert torch.equal(v, ref.state_dict()[k]), k              # seed for seed the same weights
        x, tg = R.forced_inputs(i)
        got = ref([x, tg, [L] * B]).numpy()
        want = R.forced(R.decoder_params(head.state_dict(), "decoder."), x.numpy(), tg.numpy())
        errs.append(np.abs(got - want).max())
        maxabs.append(np.abs(want).max())
        print("forced case", i, (B, L, C, T), "reference fp32 error %.3e at max|logit| %.2f" % (errs[-1], maxabs[-1]))
    out["forced_ref_err"], out["forced_maxabs"] = np.array(errs), np.array(maxabs)
    C, eos = 39, R.EOS[39]
    head = R.make_head(R.HEAD_SEED, C)
    ref = RefHead(C, 512, 512, 512, 100)
    ref.load_state_dict(head.state_dict())
    x = R.features(8, seed=R.DECODE_FEATURE_SEED)
    P = R.decoder_params(head.state_dict(), "decoder.")
    g_ids, g_scores = ref.sample([x, None, None])
    b_ids, _ = ref.beam_search(x, 5, eos)
    r_gi, r_gs, r_gm = R.greedy(P, x.numpy(), 100, eos)
    r_bi, r_bm = R.beam(P, x.numpy(), 100, eos)
    out.update(x=x.numpy(), greedy_ids=g_ids.numpy().astype(np.int32), greedy_scores=g_scores.numpy(),
               beam_ids=b_ids.numpy().astype(np.int32), greedy_margin=r_gm, beam_margin=r_bm)
    print("greedy margins", r_gm, "lengths", [len(r) for r in R.upto_eos(r_gi, eos)])
    print("beam margins", r_bm, "lengths", [len(r) for r in R.upto_eos(r_bi, eos)])
    print("greedy rows equal", [a == b for a, b in zip(R.upto_eos(g_ids.numpy(), eos), R.upto_eos(r_gi, eos))])
    print("beam rows equal", [a == b for a, b in zip(R.upto_eos(b_ids.numpy(), eos), R.upto_eos(r_bi, eos))])
    _, need = R.margin_bound(out["forced_ref_err"].max(), out["forced_maxabs"].max())
    print("margin bound %.3e: beam rows below it %d, greedy rows below it %d (at most 2 of 8 may be)" % (need, (r_bm <= need).sum(), (r_gm <= need).sum()))
    assert (r_bm <= need).sum() <= 2 and (r_gm <= need).sum() <= 2
    np.savez_compressed(os.path.join(GOLD, "aster_decode.npz"), **out)

    # ---- the whole recogniser -----------------------------------------------------------------------------------------------------------
    info = tatt_amd.aster.AsterInfo("all")
    eos = info.char2id[info.EOS]
    kw = dict(arch="ResNet_ASTER", rec_num_classes=info.rec_num_classes, sDim=512, attDim=512, max_len_labels=info.max_len, eos=eos,
              STN_ON=True)
    torch.manual_seed(R.E2E_SEED)
    ref = RecognizerBuilder(**kw)
    torch.manual_seed(R.E2E_SEED)
    mine = tatt_amd.ASTER(**kw)
    sd = ref.state_dict()
    assert list(sd) == list(mine.state_dict()), "state_dict keys differ"
    for k, v in mine.state_dict().items():
        assert v.shape == sd[k].shape and torch.equal(v, sd[k]), k
    mine.load_state_dict(sd, strict=True)
    e2e = {"keys": np.array(list(sd)), "shapes": np.array([str(tuple(v.shape)) for v in sd.values()]),
           "check_keys": np.array(CHECK_KEYS), "check_sums": np.array([float(sd[k].double().abs().sum()) for k in CHECK_KEYS])}
    ref = R.e2e_model(RecognizerBuilder, **kw)
    ref.eval()
    img = images(3)

    def run(model, x):
        stn_in = torch.nn.functional.interpolate(x, model.tps_inputsize, mode="bilinear", align_corners=True)
        _, ctrl = model.stn_head(stn_in)
        rect, src = model.tps(x, ctrl)
        feats = model.encoder(rect).contiguous()
        return stn_in, ctrl, src, rect, feats

    stn_in, ctrl, src, rect, feats = run(ref, img)
    ref64 = RecognizerBuilder(**kw).double()
    ref64.load_state_dict({k: v.double() for k, v in ref.state_dict().items()})
    ref64.eval()
    d = [t.double() for t in run(ref64, img.double())]
    for name, a, b in zip(("stn_in", "ctrl", "src", "rect", "feats"), (stn_in, ctrl, src, rect, feats), d):
        e2e["err_" + name] = np.array(float((a.double() - b).abs().max()))
        print("reference fp32 vs float64:", name, float(e2e["err_" + name]), "max |value|", float(b.abs().max()))
    # the sampler alone: fp32 sampling at the RECORDED fp32 grid against float64 sampling at the same grid
    at = torch.nn.functional.grid_sample(img.double(), (2.0 * src.double().clamp(0, 1) - 1.0).view(3, 32, 100, 2))
    e2e["err_rect_at_src"] = np.array(float((rect.double() - at).abs().max()))
    print("reference fp32 sampler at its own grid vs float64:", float(e2e["err_rect_at_src"]))
    tg = torch.ones(3, 100, dtype=torch.long)
    forced = ref.decoder([feats, tg, [100] * 3])
    g_ids, g_scores = ref.decoder.sample([feats, None, None])
    res = ref({"images": img, "rec_targets": tg.int(), "rec_lengths": [100] * 3})
    b_ids = res["output"]["pred_rec"]
    P = R.decoder_params(ref.state_dict())
    f64 = R.forced(P, feats.numpy(), tg.numpy())
    _, _, gm = R.greedy(P, feats.numpy(), 100, eos)
    r_bi, bm = R.beam(P, feats.numpy(), 100, eos)
    # the TPS kernel inverse is a LAPACK result (last bits depend on the machine) with entries up to 87: the tests load the recorded one, as
    # a checkpoint would
    e2e["tps_inverse_kernel"] = ref.tps.inverse_kernel.numpy()
    e2e.update(images=img.numpy(), stn_in=stn_in.numpy(), ctrl=ctrl.numpy(), src=src.numpy(), rect=rect.numpy(), feats=feats.numpy(),
               forced_logits=forced.numpy(), err_forced=np.array(np.abs(forced.numpy() - f64).max()),
               greedy_ids=g_ids.numpy().astype(np.int32), greedy_scores=g_scores.numpy(), beam_ids=b_ids.numpy().astype(np.int32),
               greedy_margin=gm, beam_margin=bm, strings=np.array(tatt_amd.aster.get_string_aster(b_ids, info)),
               id_cases=np.array([[10, 36, 62, 70, 96, 5, eos, 3], [eos, 1, 2, 3, 4, 5, 6, 7], [1, 95, 2, 96, 61, 35, 9, 0]], dtype=np.int32))
    from utils.metrics import get_string_aster as ref_gsa
    e2e["id_strings"] = np.array(ref_gsa(torch.from_numpy(e2e["id_cases"]).long(), torch.from_numpy(e2e["id_cases"]).long(), info)[0])
    e2e["forced_maxabs"] = np.array(np.abs(f64).max())
    _, bound = R.margin_bound(e2e["err_forced"], e2e["forced_maxabs"])
    print("e2e forced error of the reference %.3e, max |logit| %.2f, margin bound %.3e" % (float(e2e["err_forced"]), np.abs(f64).max(), bound))
    assert (bm > bound).all() and (gm > bound).all(), "choose other images: a row's margin is below the bound"
    print("beam strings", e2e["strings"], "margins", bm, "greedy margins", gm)
    print("beam rows equal the restatement", [a == b for a, b in zip(R.upto_eos(b_ids.numpy(), eos), R.upto_eos(r_bi, eos))])
    np.savez_compressed(os.path.join(GOLD, "aster_e2e.npz"), **e2e)
    for f in ("aster_decode.npz", "aster_e2e.npz"):
        print(f, os.path.getsize(os.path.join(GOLD, f)), "bytes")


if __name__ == "__main__":
    main()
