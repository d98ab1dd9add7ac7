"""The ASTER attention decoder on the GPU: the one-launch kernel (tatt_attn_decode) and the step-by-step route (`decode_eager`) against
the float64 specification of tests/aster_ref.py.

Error bar of the forced-mode logits (per case): 4 x the error of the reference's own fp32 torch decoder against float64 on the same
inputs (recorded in tests/golden/aster_decode.npz when the fixture was generated) + 1e-7 x the largest |logit|.  Ids of greedy and beam
decoding are compared up to and including a row's first EOS, on every row whose float64 decision margin exceeds 100 x the largest of
those bars; at most a quarter of a batch's rows may fall below it."""
import os

import numpy as np
import pytest
import torch

import tatt_amd
from tatt_amd import aster, ops
from tatt_amd._lib import LIB

import aster_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
_CACHE = {}


@pytest.fixture(scope="module")
def dec():
    return np.load(os.path.join(GOLD, "aster_decode.npz"))


@pytest.fixture
def arithmetic(request):
    before = tatt_amd.get_arithmetic()
    tatt_amd.set_arithmetic(request.param)
    yield request.param
    tatt_amd.set_arithmetic(before if before != "mixed" else "split_bf16")


def _head(C, L=100, surgery=None, eos=None):
    key = (C, L, surgery, eos)
    if key not in _CACHE:
        head = R.make_head(R.HEAD_SEED, C, L=L)
        if surgery == "noeos":
            with torch.no_grad():
                head.decoder.fc.bias[eos] = -100.0
        elif surgery == "end":
            R.end_all_beams(head, eos)
        P = R.decoder_params(head.state_dict(), "decoder.")
        _CACHE[key] = (head.to(DEV), P)
    return _CACHE[key]


def _forced_want(i):
    if ("forced", i) not in _CACHE:
        B, L, C, T = R.FORCED_CASES[i]
        x, tg = R.forced_inputs(i)
        _CACHE[("forced", i)] = (x, tg, R.forced(_head(C)[1], x.numpy(), tg.numpy()))
    return _CACHE[("forced", i)]


@pytest.mark.parametrize("arithmetic", ["split_bf16", "fp32"], indirect=True)
@pytest.mark.parametrize("i", range(len(R.FORCED_CASES)))
def test_forced_logits(i, arithmetic, dec):
    B, L, C, T = R.FORCED_CASES[i]
    x, tg, want = _forced_want(i)
    head, _ = _head(C)
    got = aster.attn_decode(head, x.to(DEV), 0, targets=tg.to(DEV))
    assert got is not None and tuple(got.shape) == (B, L, C)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    bar, _ = R.margin_bound(dec["forced_ref_err"][i], dec["forced_maxabs"][i])
    eager = aster.decode_eager(head, x.to(DEV), 0, targets=tg.to(DEV))
    err_eager = float(np.abs(eager.cpu().numpy().astype(np.float64) - want).max())
    print("forced %s %s: one launch %.3e, step by step %.3e, reference fp32 %.3e, bar %.3e, max |logit| %.1f"
          % (R.FORCED_CASES[i], arithmetic, err, err_eager, dec["forced_ref_err"][i], bar, dec["forced_maxabs"][i]))
    assert err <= bar
    assert err_eager <= bar
    tatt_amd.sync_check()


# name: (B, L, C, eos, surgery, feature seed) -- seeds: the first at which at most a quarter of the rows are below the margin bound
DECODE_CASES = {
    "b1": (1, 100, 39, 36, None, 1),                 # five beam rows
    "b3": (3, 100, 39, 36, None, 9),
    "b17": (17, 40, 97, 94, None, 19),               # crosses 16 rows; both class counts
    "fixture": (8, 100, 39, 36, None, R.DECODE_FEATURE_SEED),      # short rows, long rows and rows without EOS in one batch
    "no_eos": (3, 12, 39, 36, "noeos", 1),           # no row ever emits EOS
    "all_ended": (3, 100, 39, 36, "end", 1),         # every beam of every image has ended at step 4 of 100
    "eos_class_0": (3, 100, 39, 0, "end", 1),        # ... and the ended beams' slots then hold class 0 = EOS: the tie rule among dead beams
}


def _decode_want(name):
    if ("decode", name) not in _CACHE:
        B, L, C, eos, surgery, seed = DECODE_CASES[name]
        head, P = _head(C, L, surgery, eos)
        x = R.features(B, seed=seed)
        _CACHE[("decode", name)] = (head, x, R.greedy(P, x.numpy(), L, eos), R.beam(P, x.numpy(), L, eos))
    return _CACHE[("decode", name)]


def _kept(margin, need):
    keep = margin > need
    assert (~keep).sum() * 4 <= len(keep), "more than a quarter of the rows are below the margin bound %.3e: %s" % (need, margin)
    return np.nonzero(keep)[0]


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_greedy_and_beam(name, dec):
    B, L, C, eos, surgery, seed = DECODE_CASES[name]
    head, x, (g_ids, g_scores, g_margin), (b_ids, b_margin) = _decode_want(name)
    bar, need = R.margin_bound(dec["forced_ref_err"].max(), dec["forced_maxabs"].max())
    xd = x.to(DEV)
    for route in (aster.attn_decode, aster.decode_eager):
        ids, scores = route(head, xd, 1, eos)
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, L) and tuple(scores.shape) == (B, L)
        ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        got, want = R.upto_eos(ids, eos), R.upto_eos(g_ids, eos)
        for r in _kept(g_margin, need):
            assert got[r] == want[r], (route.__name__, "greedy", r, got[r], want[r])
            n = len(want[r])
            assert np.abs(scores[r, :n] - g_scores[r, :n]).max() <= bar, (route.__name__, r)
            assert (ids[r, n:] == eos).all() and (scores[r, n:] == 0).all()          # beyond the first EOS: EOS / 0
        ids, scores = route(head, xd, 2, eos)
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, L)
        assert bool((scores == 1).all())
        got, want = R.upto_eos(ids.cpu().numpy(), eos), R.upto_eos(b_ids, eos)
        for r in _kept(b_margin, need):
            assert got[r] == want[r], (route.__name__, "beam", r, got[r], want[r])
    lens = [len(r) for r in R.upto_eos(b_ids, eos)]
    if name == "no_eos":
        assert lens == [L] * B and (g_ids != eos).all()
    if surgery == "end":
        assert lens == [4] * B
    tatt_amd.sync_check()


REFUSED_SEEDS = (2, 1)         # feature seeds of test_refused_geometries: the first at which both rows' beam margins exceed the bound


def _raw_decode(sDim, C):
    z = torch.zeros(4, device=DEV)
    zi = torch.zeros(4, dtype=torch.int32, device=DEV)
    p = ops.P(z)
    return LIB.tatt_attn_decode(p, p, p, p, p, p, p, p, p, p, p, p, ops.P(zi), p, ops.P(zi), p, 1, 25, C, 4, sDim, sDim, sDim, 0, 1, 5,
                                ops.stream())


def test_refused_geometries(dec):
    assert _raw_decode(256, 39) == 1
    assert _raw_decode(512, 200) == 1
    for kw, seed in ((dict(sDim=256, attDim=256, rec_num_classes=39, eos=36), REFUSED_SEEDS[0]), (dict(rec_num_classes=200, eos=197), REFUSED_SEEDS[1])):
        torch.manual_seed(3)
        m = R.scale_fc(tatt_amd.ASTER(max_len_labels=6, **kw)).to(DEV).eval()
        before = dict(aster.LAUNCHES)
        feats = R.features(2, seed=seed).to(DEV)
        assert aster.attn_decode(m.decoder, feats, 2, m.eos) is None
        ids, scores = m.decode(feats, "beam")
        assert tuple(ids.shape) == (2, 6) and aster.LAUNCHES["eager"] == before["eager"] + 1
        assert aster.LAUNCHES["one_launch"] == before["one_launch"]
        ids2, _ = m.read(torch.rand(2, 3, 32, 128, generator=torch.Generator().manual_seed(2)).to(DEV) * 2 - 1)      # ASTER.read as well
        assert tuple(ids2.shape) == (2, 6) and aster.LAUNCHES == {"one_launch": before["one_launch"], "eager": before["eager"] + 2}
        P = R.decoder_params(m.state_dict())
        want, margin = R.beam(P, feats.cpu().numpy(), 6, m.eos)
        _, need = R.margin_bound(dec["forced_ref_err"].max(), dec["forced_maxabs"].max())
        assert (margin > need).all(), margin                        # (feature seeds chosen so that both rows are compared)
        assert R.upto_eos(ids.cpu().numpy(), m.eos) == R.upto_eos(want, m.eos)
    torch.cuda.synchronize()
    tatt_amd.sync_check()


def test_beam_backtrack_kernel():
    """tatt_beam_backtrack (the step-by-step route's) against the specification's backtracking, on histories with many EOS, with all beams
    ended, and with EOS as class 0"""
    for eos, surgery, C in ((36, None, 39), (36, "end", 39), (0, "end", 39), (3, None, 5)):
        head = R.make_head(R.HEAD_SEED, C)
        if surgery:
            R.end_all_beams(head, eos)
        P = R.decoder_params(head.state_dict(), "decoder.")
        want, _, (sym, pred, score) = R.beam(P, R.features(17, seed=18).numpy(), 30, eos, want_history=True)
        assert np.array_equal(aster.beam_backtrack(sym, pred, score, eos), want)
        L, B, K = sym.shape
        ids = torch.empty(B, L, dtype=torch.int32, device=DEV)
        ws = torch.empty(B, L, K, dtype=torch.int32, device=DEV)
        dsym, dpred, dscore = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype=t)
                               for a, t in ((sym, torch.int32), (pred, torch.int32), (score, torch.float32)))
        ops.call("tatt_beam_backtrack", ops.P(dsym), ops.P(dpred), ops.P(dscore), ops.P(ids), ops.P(ws), L, B, K, eos, ops.stream())
        assert np.array_equal(ids.cpu().numpy(), want), (eos, surgery, C)


# ---- the widest geometry the one launch takes: T = 32 fills the softmax wave, C = 128 both classes of every lane of the arg-max and all
# 640 candidates of the beam.  Error bars as above, from this geometry's own numbers (tests/golden/attn_decode_limits.npz).
LIMIT_FORCED = (2, 3, 128, 32, 1)              # (B, L, C, T, feature seed)
# (B, L, C, T, feature seed, eos) -- seed: the first at which both rows' greedy and beam margins exceed the bound, found by
# tools/gen_golden_aster.py with the float64 specification on the CPU and recorded in the fixture
LIMIT_DECODE = (2, 6, 128, 32, 1, 125)


@pytest.fixture(scope="module")
def lim():
    lim = np.load(os.path.join(GOLD, "attn_decode_limits.npz"))
    assert tuple(lim["aster_forced_case"]) == LIMIT_FORCED and tuple(lim["aster_decode_case"]) == LIMIT_DECODE
    return lim


def _limit_inputs(case):
    B, L, C, T, seed = case[:5]
    return R.features(B, T, seed), torch.randint(0, C, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("arithmetic", ["split_bf16", "fp32"], indirect=True)
def test_forced_logits_at_the_limits(arithmetic, lim):
    B, L, C, T, _ = LIMIT_FORCED
    head, P = _head(C)
    if "limit_forced" not in _CACHE:
        x, tg = _limit_inputs(LIMIT_FORCED)
        _CACHE["limit_forced"] = (x, tg, R.forced(P, x.numpy(), tg.numpy()))
    x, tg, want = _CACHE["limit_forced"]
    bar, _ = R.margin_bound(lim["aster_forced_ref_err"], lim["aster_forced_maxabs"])
    before = aster.LAUNCHES["one_launch"]
    for route in (aster.attn_decode, aster.decode_eager):
        got = route(head, x.to(DEV), 0, targets=tg.to(DEV))
        assert got is not None and tuple(got.shape) == (B, L, C)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print("forced at the limits %s %s: error %.3e, reference fp32 %.3e, bar %.3e" % (arithmetic, route.__name__, err,
                                                                                        lim["aster_forced_ref_err"], bar))
        assert err <= bar, (route.__name__, err, bar)
    assert aster.LAUNCHES["one_launch"] == before + 1
    tatt_amd.sync_check()


def test_greedy_and_beam_at_the_limits(lim):
    B, L, C, T, _, eos = LIMIT_DECODE
    head, P = _head(C, L)
    x = _limit_inputs(LIMIT_DECODE)[0]
    g_ids, g_scores, g_margin = R.greedy(P, x.numpy(), L, eos)
    b_ids, b_margin = R.beam(P, x.numpy(), L, eos)
    bar, need = R.margin_bound(max(lim["aster_forced_ref_err"], lim["aster_decode_ref_err"]),
                               max(lim["aster_forced_maxabs"], lim["aster_decode_maxabs"]))
    assert (g_margin > need).all() and (b_margin > need).all(), (g_margin, b_margin, need)      # (the seed: every row is compared)
    xd = x.to(DEV)
    before = aster.LAUNCHES["one_launch"]
    for route in (aster.attn_decode, aster.decode_eager):
        ids, scores = route(head, xd, 1, eos)
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, L) and tuple(scores.shape) == (B, L)
        ids, scores = ids.cpu().numpy(), scores.cpu().numpy()
        got, want = R.upto_eos(ids, eos), R.upto_eos(g_ids, eos)
        for r in range(B):
            assert got[r] == want[r], (route.__name__, "greedy", r, got[r], want[r])
            n = len(want[r])
            err = np.abs(scores[r, :n] - g_scores[r, :n]).max()
            print("greedy at the limits %s row %d: score error %.3e, bar %.3e" % (route.__name__, r, err, bar))
            assert err <= bar, (route.__name__, r)
            assert (ids[r, n:] == eos).all() and (scores[r, n:] == 0).all()          # beyond the first EOS: EOS / 0
        ids, scores = route(head, xd, 2, eos)
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, L)
        assert bool((scores == 1).all())
        assert R.upto_eos(ids.cpu().numpy(), eos) == R.upto_eos(b_ids, eos), (route.__name__, "beam")
    assert aster.LAUNCHES["one_launch"] == before + 2
    tatt_amd.sync_check()
