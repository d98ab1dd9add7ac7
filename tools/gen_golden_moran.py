"""Golden data of the MORAN recogniser, recorded from the reference's own modules (imported through tools/_ref_import.py, built with
inputDataType='torch.FloatTensor', CUDA=False).  Runs where the reference is, beside tools/gen_golden_aster.py; the tests never import
the reference.  Both grid_sample calls run as the installed torch runs them (align_corners=False).

  tests/golden/moran_decode.npz  the decoder alone (seeded Attention heads with generator.weight x 30, randn features): per forced case
                                 and direction the error of the reference's fp32 cell against float64 (the unit of the GPU error bar),
                                 and two greedy batches (one whose arg-max repeats, one whose arg-max keeps changing): the reference's
                                 fp32 ids, the float64 margins of tests/moran_ref.py
  tests/golden/moran_e2e.npz     the whole recogniser (seeds, `perturb`: tests/moran_ref.py) on 6 images: offsets of both passes,
                                 offsets_grid, rectified image, encoder features, L2R / R2L rows and ids, the float64 run's distance per
                                 stage (the unit of the error bars; for the sampler also alone, at the recorded offsets), margins, the
                                 key list, shapes, init checksums and an id table with its decoded strings
  tests/golden/attn_decode_limits.npz (the `moran_*` entries; `--limits` writes these alone)
                                 the decoder at the widest geometry its one launch takes (T = 32, C = 64): per case and direction the
                                 reference's fp32 error against float64 and the largest |logit|, and the greedy case's feature seed
No weights are stored (81 MB): the tests rebuild them from the seeds.
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
import moran_ref as R                               # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
CHECK_KEYS = ["MORN.cnn.1.weight", "MORN.cnn.15.bias", "ASRN.cnn.block0.0.weight", "ASRN.cnn.block3.0.downsample.0.weight",
              "ASRN.cnn.block5.2.conv2.0.weight", "ASRN.rnn.1.rnn.weight_hh_l0_reverse", "ASRN.rnn.0.embedding.weight",
              "ASRN.attentionL2R.char_embeddings", "ASRN.attentionL2R.attention_cell.rnn.weight_ih",
              "ASRN.attentionR2L.attention_cell.h2h.weight", "ASRN.attentionR2L.generator.bias"]
ARGS = (1, 37, 256, 32, 100)


def cell_forced(att, x, targets):
    """the reference's AttentionCell and generator, step by step in test mode with the given embedding rows: x (B, T, 256) -> (B, L, C)"""
    feats = x.permute(1, 0, 2).contiguous()
    C = att.num_classes
    h = torch.zeros(x.shape[0], att.hidden_size, dtype=x.dtype)
    out = []
    for i in range(targets.shape[1]):
        emb = att.char_embeddings.index_select(0, targets[:, i].clamp(0, C))
        h, _ = att.attention_cell(h, feats, emb, True)
        out.append(att.generator(h))
    return torch.stack(out, 1)


def morn_stages(morn, x):
    """MORN.forward (test=True, enhance=1) with its intermediate maps, on the reference's own sub-modules and grids"""
    F = torch.nn.functional
    B = x.shape[0]
    grid, gx, gy = morn.grid[:B], morn.grid_x[:B], morn.grid_y[:B]

    def inc(img):
        o = morn.cnn(img)
        pool = morn.pool(F.relu(o)) - morn.pool(F.relu(-o))
        return o, F.grid_sample(pool, grid).permute(0, 2, 3, 1).contiguous()

    o1, og = inc(x)
    rect1 = F.grid_sample(x, torch.cat([gx, gy + og], 3))
    o2, g2 = inc(rect1)
    og = og + g2
    rect = F.grid_sample(x, torch.cat([gx, gy + og], 3))
    return {"offsets": o1[:, 0], "offsets2": o2[:, 0], "offsets_grid": og[..., 0], "rect1": rect1, "rect": rect}


def to_double(ref):
    ref = ref.double()
    m = ref.MORN
    m.grid, m.grid_x, m.grid_y = m.grid.double(), m.grid_x.double(), m.grid_y.double()      # (plain attributes: .double() leaves them)
    m.inputDataType = "torch.DoubleTensor"
    return ref


# the widest geometries: (B, L, C, T) of the forced and of the greedy case, the forced case's feature seed
LIMIT_FORCED, LIMIT_GREEDY, LIMIT_FORCED_SEED = (2, 2, 64, 32), (2, 4, 64, 32), 1


def limit_inputs(case, seed):
    B, L, C, T = case
    return R.features(B, T, seed), torch.randint(0, C + 1, (B, L), generator=torch.Generator().manual_seed(seed))


def limits(RefAttention):
    from gen_golden_aster import merge_limits
    C = LIMIT_FORCED[2]
    heads = []
    for d in range(2):
        att = R.make_attention(R.HEAD_SEED + d, C)
        ref = RefAttention(256, 256, C, 256, CUDA=False)
        ref.load_state_dict(att.state_dict())
        heads.append((ref, R.decoder_params(att.state_dict(), "")))

    def ref_err(case, seed):
        x, tg = limit_inputs(case, seed)
        wants = [R.forced(P, x.numpy(), tg.numpy()) for _, P in heads]
        return (np.array([np.abs(cell_forced(ref, x, tg).numpy() - w).max() for (ref, _), w in zip(heads, wants)]),
                np.array([np.abs(w).max() for w in wants]))

    fe, fm = ref_err(LIMIT_FORCED, LIMIT_FORCED_SEED)
    for seed in range(1, 100):      # the first feature seed at which every row's greedy margin exceeds the bound, in both directions
        ge, gm = ref_err(LIMIT_GREEDY, seed)
        _, need = R.margin_bound(max(fe.max(), ge.max()), max(fm.max(), gm.max()))
        x = limit_inputs(LIMIT_GREEDY, seed)[0].numpy()
        margins = np.stack([R.greedy(P, x, LIMIT_GREEDY[1])[2] for _, P in heads])
        print("limits: seed", seed, "bound %.3e" % need, "greedy margins", margins)
        if (margins > need).all():
            break
    else:
        raise AssertionError("no feature seed below 100 clears the margin bound")
    print("limits: forced reference fp32 error", fe, "at max|logit|", fm, "greedy", ge, "at", gm, "seed", seed)
    merge_limits({"moran_forced_case": np.array(LIMIT_FORCED + (LIMIT_FORCED_SEED,)), "moran_forced_ref_err": fe, "moran_forced_maxabs": fm,
                  "moran_greedy_case": np.array(LIMIT_GREEDY + (seed,)), "moran_greedy_ref_err": ge, "moran_greedy_maxabs": gm})


def main():
    import_reference()
    from model.moran.moran import MORAN as RefMORAN
    from model.moran.asrn_res import Attention as RefAttention
    from utils.utils_moran import strLabelConverterForAttention
    import tatt_amd
    from tatt_amd import moran
    torch.set_grad_enabled(False)
    kw = dict(BidirDecoder=True, inputDataType="torch.FloatTensor", CUDA=False)
    limits(RefAttention)
    if "--limits" in sys.argv[1:]:
        return

    # ---- the decoder alone ------------------------------------------------------------------------------------------------------------
    out = {}
    errs, maxabs = np.zeros((len(R.FORCED_CASES), 2)), np.zeros((len(R.FORCED_CASES), 2))
    for i, (B, L, C, T) in enumerate(R.FORCED_CASES):
        x, tg = R.forced_inputs(i)
        for d in range(2):
            att = R.make_attention(R.HEAD_SEED + d, C)
            torch.manual_seed(R.HEAD_SEED + d)
            ref = RefAttention(256, 256, C, 256, CUDA=False)
            ref.generator.weight.mul_(R.GEN_SCALE)
            for k, v in att.state_dict().items():
                assert torch.equal(v, ref.state_dict()[k]), k              # seed for seed the same weights
            got = cell_forced(ref, x, tg).numpy()
            want = R.forced(R.decoder_params(att.state_dict(), ""), x.numpy(), tg.numpy())
            ref64 = cell_forced(ref.double(), x.double(), tg).numpy()
            assert np.abs(ref64 - want).max() < 1e-9, np.abs(ref64 - want).max()      # the restatement is the reference in float64
            errs[i, d], maxabs[i, d] = np.abs(got - want).max(), np.abs(want).max()
        print("forced case", i, (B, L, C, T), "reference fp32 error", errs[i], "at max|logit|", maxabs[i])
    out["forced_ref_err"], out["forced_maxabs"] = errs, maxabs
    _, need = R.margin_bound(errs.max(), maxabs.max())
    for name, seed, scale in R.GREEDY_CASES:
        x = R.features(R.GREEDY_B, R.GREEDY_T, seed)
        for d, dn in enumerate(("l2r", "r2l")):
            att = R.make_attention(R.HEAD_SEED + d, 37, scale)
            ref = RefAttention(256, 256, 37, 256, CUDA=False)
            ref.load_state_dict(att.state_dict())
            length = torch.full((R.GREEDY_B,), R.GREEDY_L, dtype=torch.int32)
            probs = ref(x.permute(1, 0, 2).contiguous(), length, None, test=True).view(R.GREEDY_B, R.GREEDY_L, 37)
            ids, lg, margin = R.greedy(R.decoder_params(att.state_dict(), ""), x.numpy(), R.GREEDY_L)
            ref_ids = probs.argmax(2).numpy()
            changes = (ids[:, 1:] != ids[:, :-1]).sum(1)
            print("greedy", name, dn, "margins", np.round(margin, 4), "changes per row", changes, "rows equal", (ref_ids == ids).all(1))
            assert (margin <= need).sum() * 4 <= R.GREEDY_B, "choose another feature seed: too many rows below the bound %g" % need
            assert ((ref_ids == ids).all(1) | (margin <= need)).all()
            if name == "repeat":
                assert (changes <= 5).any(), "no row whose arg-max repeats"
            else:
                assert (changes == R.GREEDY_L - 1).any(), "no row whose arg-max changes at every step"
            out["greedy_%s_%s_ids" % (name, dn)] = ref_ids.astype(np.int32)
            out["greedy_%s_%s_logits" % (name, dn)] = probs.numpy()
            out["greedy_%s_%s_margin" % (name, dn)] = margin
    np.savez_compressed(os.path.join(GOLD, "moran_decode.npz"), **out)

    # ---- the whole recogniser -----------------------------------------------------------------------------------------------------------
    torch.manual_seed(R.E2E_SEED)
    ref = RefMORAN(*ARGS, **kw)
    torch.manual_seed(R.E2E_SEED)
    mine = tatt_amd.MORAN(*ARGS, BidirDecoder=True)
    sd = ref.state_dict()
    assert list(sd) == list(mine.state_dict()) and len(sd) == 427, "state_dict keys differ"
    for k, v in mine.state_dict().items():
        assert v.shape == sd[k].shape and torch.equal(v, sd[k]), k
    mine.load_state_dict(sd, strict=True)
    e2e = {"keys": np.array(list(sd)), "shapes": np.array([str(tuple(v.shape)) for v in sd.values()]),
           "check_keys": np.array(CHECK_KEYS), "check_sums": np.array([float(sd[k].double().abs().sum()) for k in CHECK_KEYS])}
    ref = R.e2e_model(RefMORAN, inputDataType="torch.FloatTensor", CUDA=False)
    ref.eval()
    B, L = R.E2E_B, 20
    img = R.images(B)
    length = torch.full((B,), L, dtype=torch.int32)
    text = torch.zeros(B * L, dtype=torch.long)

    def run(model, x):
        st = morn_stages(model.MORN, x)
        assert torch.equal(st["rect"], model.MORN(x, True)), "the staged rectifier is not MORN.forward"
        l2r, r2l = model(x, length, text, text, test=True)
        conv = model.ASRN.cnn(st["rect"]).squeeze(2).permute(2, 0, 1).contiguous()
        st["feats"] = model.ASRN.rnn(conv).permute(1, 0, 2).contiguous()
        st["logits_l2r"], st["logits_r2l"] = l2r, r2l
        return st

    got = run(ref, img)
    ref64 = RefMORAN(*ARGS, **kw)
    ref64.load_state_dict(ref.state_dict())
    ref64 = to_double(ref64).eval()
    got64 = run(ref64, img.double())
    for name in ("offsets", "offsets2", "offsets_grid", "rect", "feats", "logits_l2r", "logits_r2l"):
        e2e["err_" + name] = np.array(float((got[name].double() - got64[name]).abs().max()))
        e2e["max_" + name] = np.array(float(got64[name].abs().max()))
        print("reference fp32 vs float64: %-12s %.3e   max |value| %.3f" % (name, float(e2e["err_" + name]), float(e2e["max_" + name])))
    # the sampler alone: the recorded fp32 image / increments against float64 sampling at the RECORDED fp32 offsets
    at = R.rectify_at(img.numpy(), got["offsets_grid"].numpy())
    e2e["err_rect_at_offsets"] = np.array(float(np.abs(got["rect"].double().numpy() - at).max()))
    inc = R.offsets_increment(got["offsets"].numpy(), (32, 100)) + R.offsets_increment(got["offsets2"].numpy(), (32, 100))
    e2e["err_grid_at_offsets"] = np.array(float(np.abs(got["offsets_grid"].double().numpy() - inc).max()))
    print("reference fp32 sampler alone vs float64: image %.3e, offsets_grid %.3e" % (float(e2e["err_rect_at_offsets"]),
                                                                                     float(e2e["err_grid_at_offsets"])))
    print("offsets_grid spans %.3f .. %.3f; mean |rect - image| %.3f" % (float(got["offsets_grid"].min()), float(got["offsets_grid"].max()),
                                                                        float((got["rect"] - img).abs().mean())))
    spec = R.whole(ref.state_dict(), img.numpy(), L)
    # the reference's decoder collects its rows in an fp32 buffer whatever the model's format (asrn_res.py:131), so its "float64" rows are
    # rounded to fp32: the distance of the rows is taken from the restatement, which that run equals up to this rounding
    for dn in ("l2r", "r2l"):
        want = R.rows(spec["logits_" + dn], [L] * B)
        assert np.abs(got64["logits_" + dn].numpy() - want).max() <= 2.0 ** -23 * np.abs(want).max()
        e2e["err_logits_" + dn] = np.array(float(np.abs(got["logits_" + dn].double().numpy() - want).max()))
        e2e["max_logits_" + dn] = np.array(float(np.abs(want).max()))
        print("reference fp32 vs the float64 restatement: logits_%s %.3e" % (dn, float(e2e["err_logits_" + dn])))
    for name in R.STAGES:
        print("restatement vs the reference's float64 run: %-12s %.3e" % (name, float(np.abs(got64[name].numpy() - spec[name]).max())))
    for dn in ("l2r", "r2l"):
        ids = got["logits_" + dn].view(B, L, 37).argmax(2).numpy()
        bar, need = R.margin_bound(e2e["err_logits_" + dn], e2e["max_logits_" + dn])
        margin = spec["margin_" + dn]
        print(dn, "bar %.3e, 100x bound %.3e, margins" % (bar, need), np.round(margin, 4), "rows equal", (ids == spec["ids_" + dn]).all(1))
        assert (margin <= need).sum() * 4 <= B, "choose other images: too many rows below the bound"
        assert ((ids == spec["ids_" + dn]).all(1) | (margin <= need)).all()
        e2e["ids_" + dn], e2e["margin_" + dn] = ids.astype(np.int32), margin
    conv = strLabelConverterForAttention(":".join(moran.ALPHABET), ":")
    flat = torch.from_numpy(e2e["ids_l2r"]).long().reshape(-1)
    e2e["strings"] = np.array([s.split("$")[0] for s in conv.decode(flat, length)])
    cases = np.array([[36, 1, 2, 3, 4, 5], [10, 11, 36, 12, 36, 13], [35, 0, 9, 10, 20, 30], [1, 2, 3, 4, 5, 36]], dtype=np.int32)
    e2e["id_cases"] = cases
    e2e["id_strings"] = np.array([s.split("$")[0] for s in conv.decode(torch.from_numpy(cases).long().reshape(-1),
                                                                      torch.full((4,), 6, dtype=torch.int32))])
    print("strings", e2e["strings"], "id table strings", e2e["id_strings"])
    e2e.update(images=img.numpy(), **{k: got[k].numpy() for k in ("offsets", "offsets2", "offsets_grid", "rect", "feats", "logits_l2r",
                                                                  "logits_r2l")})
    np.savez_compressed(os.path.join(GOLD, "moran_e2e.npz"), **e2e)
    for f in ("moran_decode.npz", "moran_e2e.npz"):
        print(f, os.path.getsize(os.path.join(GOLD, f)), "bytes")


if __name__ == "__main__":
    main()
