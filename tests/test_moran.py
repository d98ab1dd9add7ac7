"""The MORAN recogniser's module surface and its host specification (no GPU): state_dict parity with the reference's MORAN as recorded
in tests/golden/moran_e2e.npz, the restated helpers, and tests/moran_ref.py in float64 against the fp32 arrays the reference itself
produced (tools/gen_golden_moran.py).  Rows whose float64 decision margin is below the 100 x bound are left out of the id comparison,
at most a quarter of a batch."""
import os

import numpy as np
import pytest
import torch

import tatt_amd
from tatt_amd import moran

import moran_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARGS = (1, 37, 256, 32, 100)


@pytest.fixture(scope="module")
def e2e():
    return np.load(os.path.join(GOLD, "moran_e2e.npz"))


@pytest.fixture(scope="module")
def dec():
    return np.load(os.path.join(GOLD, "moran_decode.npz"))


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(R.E2E_SEED)
    return tatt_amd.MORAN(*ARGS, BidirDecoder=True)


@pytest.fixture(scope="module")
def spec(e2e):
    """the float64 restatement on the fixture's images, computed once"""
    m = R.e2e_model(tatt_amd.MORAN)
    return R.whole(m.state_dict(), e2e["images"], 20)


def test_state_dict_keys_and_shapes(model, e2e):
    sd = model.state_dict()
    assert len(sd) == 427
    assert list(sd) == [str(k) for k in e2e["keys"]]
    assert list(sd)[0] == "MORN.cnn.1.weight" and list(sd)[-1] == "ASRN.attentionR2L.generator.bias"
    assert [str(tuple(v.shape)) for v in sd.values()] == [str(s) for s in e2e["shapes"]]
    assert abs(sum(v.numel() * 4 for v in sd.values()) / 1e6 - 81.4) < 4.0
    assert not list(model.MORN.buffers(recurse=False))                    # the sampling grids are no buffers, as in the reference


def test_initial_weights_seed_for_seed(model, e2e):
    sd = model.state_dict()
    for k, want in zip(e2e["check_keys"], e2e["check_sums"]):
        got = float(sd[str(k)].double().abs().sum())
        assert abs(got - want) <= 1e-9 * abs(want), (k, got, want)


def test_strict_load_of_reference_layout(model):
    other = tatt_amd.MORAN(*ARGS, BidirDecoder=True)
    other.load_state_dict({k: v.clone() for k, v in model.state_dict().items()}, strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(v, model.state_dict()[k]), k


def test_single_decoder_and_ignored_arguments():
    m = tatt_amd.MORAN(1, 37, 256, 32, 100, BidirDecoder=False, inputDataType="torch.FloatTensor", maxBatch=4, CUDA=False)
    keys = list(m.state_dict())
    assert any(k.startswith("ASRN.attention.") for k in keys) and not any("attentionL2R" in k or "attentionR2L" in k for k in keys)
    assert len(keys) == 416 and m.MORN.maxBatch == 4
    with pytest.raises(ValueError, match="BidirDecoder"):
        m._attention(reverse=True)


def test_modes_raise(model):
    x, length = torch.zeros(1, 1, 32, 100), torch.tensor([20], dtype=torch.int32)
    model.train()
    with pytest.raises(NotImplementedError, match="evaluation"):
        model(x, length, None, None, test=True)
    model.eval()
    with pytest.raises(NotImplementedError, match="evaluation"):
        model(x, length, None, None)
    with pytest.raises(NotImplementedError, match="evaluation"):
        model(x, length, None, None, test=False)


def test_no_cpu_fallback(model):
    model.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.read(torch.zeros(1, 1, 32, 100))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model(torch.zeros(1, 1, 32, 100), torch.tensor([20]), None, None, test=True)


def test_sessions_refuse_moran(model):
    from tatt_amd import infer
    gen = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=1, hidden_units=32)
    with pytest.raises(TypeError, match="io.evaluate"):
        infer.evaluate_session(gen, [], recognizer=model)
    with pytest.raises(TypeError, match="io.evaluate"):
        infer.InferenceSession(gen, recognizer=model, batch_size=1)
    with pytest.raises(TypeError, match="io.evaluate"):
        infer.SuperResolver(gen, recognizer=model)


def test_helpers(e2e):
    assert moran.ALPHABET == "0123456789abcdefghijklmnopqrstuvwxyz$" and len(moran.ALPHABET) == 37
    # '$' first, in the middle (twice) and absent; recorded through the reference's converter and split
    assert moran.get_string_moran(e2e["id_cases"]) == [str(s) for s in e2e["id_strings"]]
    assert moran.get_string_moran(torch.from_numpy(e2e["id_cases"])) == [str(s) for s in e2e["id_strings"]]
    assert moran.get_string_moran(e2e["ids_l2r"]) == [str(s) for s in e2e["strings"]]
    with pytest.raises(RuntimeError, match="AMD GPU"):
        moran.parse_moran_data(torch.zeros(2, 3, 16, 64))


def test_parse_moran_data_length_and_text(monkeypatch):
    from tatt_amd import crnn
    monkeypatch.setattr(crnn, "parse_crnn_data", lambda img, w=100: ("luma", tuple(img.shape), w))
    t, length, text, text_rev = moran.parse_moran_data(torch.zeros(3, 4, 16, 64))
    assert t == ("luma", (3, 4, 16, 64), 100)
    assert length.dtype == torch.int32 and length.tolist() == [20, 20, 20] and not length.is_cuda
    assert text.dtype == torch.int64 and text.shape == (60,) and not text.any() and text_rev is text


def test_specification_reproduces_the_recorded_stages(e2e, spec):
    """Every recorded fp32 stage is within err_<stage> + 1e-9 x max |value| of the float64 restatement: err_<stage> is the distance of
    exactly that array from the reference's own float64 run (tools/gen_golden_moran.py), and a correct restatement is that run."""
    worst = []
    for name in ("offsets", "offsets_grid", "rect", "feats"):
        want = e2e[name].astype(np.float64)
        got = spec[name]
        dist = float(np.abs(got.reshape(want.shape) - want).max())
        bound = float(e2e["err_" + name]) * (1 + 1e-6) + 1e-9 * float(np.abs(want).max())
        print("restatement vs recorded fp32 %-12s: distance %.6e, bound %.6e" % (name, dist, bound))
        worst.append((name, dist, bound))
    for dn in ("l2r", "r2l"):
        want = e2e["logits_" + dn].astype(np.float64)
        got = R.rows(spec["logits_" + dn], [20] * R.E2E_B)
        assert got.shape == want.shape == (R.E2E_B * 20, 37)
        dist = float(np.abs(got - want).max())
        bound = float(e2e["err_logits_" + dn]) * (1 + 1e-6) + 1e-9 * float(np.abs(want).max())
        print("restatement vs recorded fp32 logits_%s: distance %.6e, bound %.6e" % (dn, dist, bound))
        worst.append(("logits_" + dn, dist, bound))
    for name, dist, bound in worst:
        assert dist <= bound, (name, dist, bound)
    # the fixture exercises the rectifier: the offsets move pixels, some of them beyond the image's edge
    assert np.abs(e2e["offsets_grid"]).max() > 0.25 and np.abs(e2e["rect"] - e2e["images"]).mean() > 0.05


def _compare_ids(got, want, margin, need):
    keep = margin > need
    assert (~keep).sum() * 4 <= len(keep), "more than a quarter of the rows are below the margin bound: %s" % margin
    for i in np.nonzero(keep)[0]:
        assert np.array_equal(got[i], want[i]), (i, got[i], want[i])
    return int(keep.sum())


def test_ids_equal_the_recorded_ones(e2e, spec):
    for dn in ("l2r", "r2l"):
        _, need = R.margin_bound(e2e["err_logits_" + dn], e2e["max_logits_" + dn])
        assert np.allclose(spec["margin_" + dn], e2e["margin_" + dn], rtol=1e-6, atol=1e-9)
        assert _compare_ids(spec["ids_" + dn], e2e["ids_" + dn], spec["margin_" + dn], need) == R.E2E_B


def test_decoder_specification_reproduces_the_reference_greedy(dec):
    _, need = R.margin_bound(dec["forced_ref_err"].max(), dec["forced_maxabs"].max())
    for name, seed, scale in R.GREEDY_CASES:
        x = R.features(R.GREEDY_B, R.GREEDY_T, seed).numpy()
        for d, dn in enumerate(("l2r", "r2l")):
            P = R.decoder_params(R.make_attention(R.HEAD_SEED + d, 37, scale).state_dict(), "")
            ids, lg, margin = R.greedy(P, x, R.GREEDY_L)
            key = "greedy_%s_%s_" % (name, dn)
            assert np.allclose(margin, dec[key + "margin"], rtol=1e-6, atol=1e-9)
            _compare_ids(ids, dec[key + "ids"], margin, need)
            changes = (ids[:, 1:] != ids[:, :-1]).sum(1)
            assert (changes <= 5).any() if name == "repeat" else (changes == R.GREEDY_L - 1).any(), changes


def test_rows_layout():
    lg = np.arange(3 * 4 * 2, dtype=np.float64).reshape(3, 4, 2)
    out = R.rows(lg, [4, 1, 3])
    assert out.shape == (8, 2) and np.array_equal(out[4], lg[1, 0]) and np.array_equal(out[5:], lg[2, :3])
