"""The ASTER recogniser's module surface and its host specification (no GPU): state_dict parity with the reference's RecognizerBuilder as
recorded in tests/golden/aster_e2e.npz, the restated helpers, and tests/aster_ref.py against the ids the reference itself decoded
(tools/gen_golden_aster.py).  Rows whose float64 decision margin is below the bound are left out, at most a quarter of them."""
import os

import numpy as np
import pytest
import torch

import tatt_amd
from tatt_amd import aster

import aster_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KW = dict(arch="ResNet_ASTER", rec_num_classes=97, sDim=512, attDim=512, max_len_labels=100, eos=94, STN_ON=True)


@pytest.fixture(scope="module")
def e2e():
    return np.load(os.path.join(GOLD, "aster_e2e.npz"))


@pytest.fixture(scope="module")
def dec():
    return np.load(os.path.join(GOLD, "aster_decode.npz"))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(R.E2E_SEED)
    return tatt_amd.ASTER(**KW)


def test_state_dict_keys_and_shapes(model, e2e):
    sd = model.state_dict()
    assert list(sd) == [str(k) for k in e2e["keys"]]
    assert len(sd) == 384
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in e2e["shapes"]]
    assert sum(p.numel() for p in model.parameters()) > 20e6


def test_initial_weights_seed_for_seed(model, e2e):
    sd = model.state_dict()
    for k, want in zip(e2e["check_keys"], e2e["check_sums"]):
        got = float(sd[str(k)].double().abs().sum())
        assert abs(got - want) <= 1e-9 * abs(want), (k, got, want)


def test_strict_load_of_reference_layout(model):
    other = tatt_amd.ASTER(**KW)
    other.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)


def test_helpers(e2e):
    info = aster.AsterInfo("all")
    assert info.rec_num_classes == 97 and info.char2id["EOS"] == 94 and info.char2id["PADDING"] == 95 and info.char2id["UNKNOWN"] == 96
    assert info.max_len == 100 and info.id2char[10] == "a" and info.id2char[36] == "A"
    low = aster.AsterInfo("lower")
    assert low.rec_num_classes == 39 and low.char2id["EOS"] == 36
    assert aster.AsterInfo("digit").rec_num_classes == 13 and aster.AsterInfo("upper").rec_num_classes == 65
    with pytest.raises(KeyError):
        aster.AsterInfo("chinese")
    x = torch.tensor([0.0, 0.25, 1.0])
    assert torch.equal(aster.parse_aster_data(x), torch.tensor([-1.0, -0.5, 1.0]))
    assert aster.get_string_aster(e2e["id_cases"], info) == [str(s) for s in e2e["id_strings"]]
    assert aster.get_string_aster(torch.from_numpy(e2e["beam_ids"]), info) == [str(s) for s in e2e["strings"]]


def _compare(got, want, margin, need, eos):
    keep = margin > need
    assert (~keep).sum() * 4 <= len(keep), "more than a quarter of the rows are below the margin bound: %s" % margin
    a, b = R.upto_eos(got, eos), R.upto_eos(want, eos)
    for i in np.nonzero(keep)[0]:
        assert a[i] == b[i], (i, a[i], b[i])
    return int(keep.sum())


def test_restatement_reproduces_the_reference_decoder(dec):
    eos = R.EOS[39]
    P = R.decoder_params(R.make_head(R.HEAD_SEED, 39).state_dict(), "decoder.")
    _, need = R.margin_bound(dec["forced_ref_err"].max(), dec["forced_maxabs"].max())
    x = dec["x"]
    assert np.array_equal(x, R.features(8, seed=R.DECODE_FEATURE_SEED).numpy())
    ids, scores, gm = R.greedy(P, x, 100, eos)
    assert np.allclose(gm, dec["greedy_margin"], rtol=1e-6, atol=1e-9)
    _compare(ids, dec["greedy_ids"], gm, need, eos)
    for i, row in enumerate(R.upto_eos(ids, eos)):
        n = len(row)
        assert np.abs(scores[i, :n] - dec["greedy_scores"][i, :n]).max() < 1e-4
    bids, bm, hist = R.beam(P, x, 100, eos, want_history=True)
    assert np.allclose(bm, dec["beam_margin"], rtol=1e-6, atol=1e-9)
    assert _compare(bids, dec["beam_ids"], bm, need, eos) >= 6
    lens = [len(r) for r in R.upto_eos(bids, eos)]
    assert min(lens) < 12 and max(lens) == 100                      # short rows and rows that never end, in one batch
    # the package's own host backtracking (the eager route's) against the specification's
    assert np.array_equal(aster.beam_backtrack(*hist, eos), bids)


def test_restatement_reproduces_the_reference_recogniser(e2e):
    """decoder of the whole-recogniser fixture, on the recorded encoder features"""
    m = R.e2e_model(tatt_amd.ASTER, **KW)
    P = R.decoder_params(m.state_dict())
    _, need = R.margin_bound(e2e["err_forced"], e2e["forced_maxabs"])
    ids, _, gm = R.greedy(P, e2e["feats"], 100, 94)
    _compare(ids, e2e["greedy_ids"], gm, need, 94)
    bids, bm = R.beam(P, e2e["feats"], 100, 94)
    assert _compare(bids, e2e["beam_ids"], bm, need, 94) == 3
    lg = R.forced(P, e2e["feats"], np.ones((3, 100), dtype=np.int64))
    assert np.abs(lg - e2e["forced_logits"]).max() <= 1.0001 * float(e2e["err_forced"])


def test_restatement_reproduces_the_reference_front_and_encoder(e2e):
    """The float64 restatement of the front and the encoder (aster_ref.stn_in / ctrl / src / rect / feats) on the fixture's images, with
    the recorded TPS kernel inverse cast to float64: each stage within err_<stage> + 1e-9 x max |value| of the fp32 array the reference
    recorded.  err_<stage> is the distance of exactly that array from the reference's own `.double()` run on the same doubled state
    (tools/gen_golden_aster.py), and a correct restatement is that run -- the bound is derived, not chosen."""
    m = R.e2e_model(tatt_amd.ASTER, **KW)
    got = R.front_and_encoder(m.state_dict(), torch.from_numpy(e2e["images"]), torch.float64, inverse_kernel=e2e["tps_inverse_kernel"])
    assert tuple(got["feats"].shape) == (3, 25, 512) and got["feats"].dtype == torch.float64
    worst = []
    for name in R.STAGES:
        want = e2e[name].astype(np.float64)
        dist = float(np.abs(got[name].numpy() - want).max())
        bound = float(e2e["err_" + name]) + 1e-9 * float(np.abs(want).max())
        print("restatement vs recorded fp32 %-6s: distance %.6e, recorded err_%s %.6e, bound %.6e" % (name, dist, name,
                                                                                                       float(e2e["err_" + name]), bound))
        worst.append((name, dist, bound))
    for name, dist, bound in worst:
        assert dist <= bound, (name, dist, bound)


def test_all_beams_can_end(dec):
    """`end_all_beams` does what the GPU tests rely on: every hypothesis of every image has ended well before L"""
    for eos in (36, 0):
        head = R.end_all_beams(R.make_head(R.HEAD_SEED, 39), eos)
        P = R.decoder_params(head.state_dict(), "decoder.")
        ids, bm, (sym, pred, score) = R.beam(P, R.features(3, seed=1).numpy(), 100, eos, want_history=True)
        dead = np.isinf(score).all(2)                                  # (L, B)
        assert dead[10:].all() and not dead[:3].any()
        assert [len(r) for r in R.upto_eos(ids, eos)] == [4, 4, 4]
        if eos == 0:
            assert (sym[10:, :, 0] == eos).all()                       # ended beams go on "emitting" class 0 = EOS: the tie rule's case


def test_training_mode_raises(model):
    model.train()
    with pytest.raises(NotImplementedError, match="evaluation"):
        model({"images": torch.zeros(1, 3, 32, 128)})
    model.eval()


def test_sessions_refuse_aster(model):
    from tatt_amd import infer
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=1, hidden_units=32)
    with pytest.raises(TypeError, match="io.evaluate"):
        infer.evaluate_session(gen, [], recognizer=model)
    with pytest.raises(TypeError, match="io.evaluate"):
        infer.InferenceSession(gen, recognizer=model, batch_size=1)
    with pytest.raises(TypeError, match="io.evaluate"):
        infer.SuperResolver(gen, recognizer=model)


def test_no_cpu_fallback(model):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.read(torch.zeros(1, 3, 32, 128))
