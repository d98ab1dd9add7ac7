"""The MORAN attention decoder on the GPU: the one-launch kernel (tatt_moran_decode) and the step-by-step route (`decode_eager`)
against the float64 specification of tests/moran_ref.py, with the weights of both directions (two seeded heads).

Error bar of the forced-mode logits (per case and direction): 4 x the error of the reference's own fp32 AttentionCell against float64 on
the same inputs (recorded in tests/golden/moran_decode.npz when the fixture was generated) + 1e-7 x the largest |logit|.  Greedy ids are
compared on every row whose float64 decision margin exceeds 100 x the largest of those bars; at most a quarter of a batch's rows may
fall below it."""
import os

import numpy as np
import pytest
import torch

from tatt_amd import moran, ops
from tatt_amd._lib import LIB

import moran_ref as R

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = "cuda:0"
DIRS = ("l2r", "r2l")
_CACHE = {}


@pytest.fixture(scope="module")
def dec():
    return np.load(os.path.join(GOLD, "moran_decode.npz"))


def _head(d, C, scale=1.0):
    key = (d, C, scale)
    if key not in _CACHE:
        att = R.make_attention(R.HEAD_SEED + d, C, scale)
        P = R.decoder_params(att.state_dict(), "")
        _CACHE[key] = (att.to(DEV), P)
    return _CACHE[key]


def _forced_want(i, d):
    if ("forced", i, d) not in _CACHE:
        B, L, C, T = R.FORCED_CASES[i]
        x, tg = R.forced_inputs(i)
        _CACHE[("forced", i, d)] = (x, tg, R.forced(_head(d, C)[1], x.numpy(), tg.numpy()))
    return _CACHE[("forced", i, d)]


@pytest.mark.parametrize("route", ["one_launch", "eager"])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("i", range(len(R.FORCED_CASES)))
def test_forced_logits(i, d, route, dec):
    B, L, C, T = R.FORCED_CASES[i]
    x, tg, want = _forced_want(i, d)
    att, _ = _head(d, C)
    before = dict(moran.LAUNCHES)
    if route == "one_launch":
        got = moran.attn_decode(att, x.to(DEV), 0, targets=tg.to(DEV))
        assert got is not None
    else:
        got = moran.decode_eager(att, x.to(DEV), 0, targets=tg.to(DEV))
    assert moran.LAUNCHES[route] == before[route] + 1
    assert tuple(got.shape) == (B, L, C)
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
    bar, _ = R.margin_bound(dec["forced_ref_err"][i, d], dec["forced_maxabs"][i, d])
    print("forced case %d %s %s %s: error %.3e, bar %.3e (reference fp32 error %.3e, max |logit| %.2f)"
          % (i, (B, L, C, T), DIRS[d], route, err, bar, dec["forced_ref_err"][i, d], dec["forced_maxabs"][i, d]))
    assert err <= bar, (err, bar)


@pytest.mark.parametrize("route", ["one_launch", "eager"])
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("case", range(len(R.GREEDY_CASES)))
def test_greedy(case, d, route, dec):
    name, seed, scale = R.GREEDY_CASES[case]
    att, P = _head(d, 37, scale)
    x = R.features(R.GREEDY_B, R.GREEDY_T, seed)
    if ("greedy", case, d) not in _CACHE:
        _CACHE[("greedy", case, d)] = R.greedy(P, x.numpy(), R.GREEDY_L)
    want_ids, want_lg, margin = _CACHE[("greedy", case, d)]
    changes = (want_ids[:, 1:] != want_ids[:, :-1]).sum(1)
    assert (changes <= 5).any() if name == "repeat" else (changes == R.GREEDY_L - 1).any(), changes
    fn = moran.attn_decode if route == "one_launch" else moran.decode_eager
    ids, lg = fn(att, x.to(DEV), 1, steps=R.GREEDY_L)
    assert ids.dtype == torch.int32 and tuple(ids.shape) == (R.GREEDY_B, R.GREEDY_L) and tuple(lg.shape) == (R.GREEDY_B, R.GREEDY_L, 37)
    ids, lg = ids.cpu().numpy(), lg.cpu().numpy().astype(np.float64)
    bar, need = R.margin_bound(dec["forced_ref_err"].max(), dec["forced_maxabs"].max())
    keep = margin > need
    assert (~keep).sum() * 4 <= len(keep), margin
    key = "greedy_%s_%s_" % (name, DIRS[d])
    errs = []
    for r in np.nonzero(keep)[0]:
        assert np.array_equal(ids[r], want_ids[r]), (r, ids[r], want_ids[r])
        assert np.array_equal(ids[r], dec[key + "ids"][r])                      # ... which are the ids the reference decoded
        errs.append(np.abs(lg[r] - want_lg[r]).max())
    print("greedy %s %s %s: %d rows compared, logits error %.3e, bar %.3e" % (name, DIRS[d], route, keep.sum(), max(errs), bar))
    assert max(errs) <= bar
    assert np.array_equal(lg.argmax(2), ids)                                     # the ids are the arg-max of the logits returned


def _model(C):
    if ("model", C) not in _CACHE:
        torch.manual_seed(R.HEAD_SEED)
        m = moran.MORAN(1, C, 256, 32, 100)
        with torch.no_grad():
            m.ASRN.attention.generator.weight.mul_(R.GEN_SCALE)
        P = R.decoder_params(m.state_dict(), "ASRN.attention.")
        _CACHE[("model", C)] = (m.to(DEV).eval(), P)
    return _CACHE[("model", C)]


@pytest.mark.parametrize("T,C,L", [(33, 37, 20), (25, 65, 20), (25, 37, 65)])
def test_refused_geometries_take_the_eager_route(T, C, L, dec):
    m, P = _model(C)
    x = R.features(2, T, 9)
    dummy = torch.zeros(8, device=DEV)
    p = ops.P(dummy)
    # (the entry refuses before it reads an operand or launches)
    assert LIB.tatt_moran_decode(p, p, p, p, p, p, p, p, p, p, p, None, p, p, 2, T, C, L, 256, 1, ops.stream()) == 1
    assert LIB.tatt_moran_decode(p, p, p, p, p, p, p, p, p, p, p, None, p, p, 2, 25, 37, 20, 512, 1, ops.stream()) == 1
    assert moran.attn_decode(m.ASRN.attention, x.to(DEV), 1, steps=L) is None
    before = dict(moran.LAUNCHES)
    got_ids, got_lg = m.decode(x.to(DEV), L)
    assert moran.LAUNCHES["eager"] == before["eager"] + 1 and moran.LAUNCHES["one_launch"] == before["one_launch"]
    assert tuple(got_ids.shape) == (2, L) and tuple(got_lg.shape) == (2, L, C)
    want_ids, want_lg, margin = R.greedy(P, x.numpy(), L)
    bar, need = R.margin_bound(dec["forced_ref_err"].max(), dec["forced_maxabs"].max())
    lg = got_lg.cpu().numpy().astype(np.float64)
    assert np.abs(lg[:, 0] - want_lg[:, 0]).max() <= bar                           # the first step depends on no decision
    for r in np.nonzero(margin > need)[0]:
        assert np.array_equal(got_ids[r].cpu().numpy(), want_ids[r]) and np.abs(lg[r] - want_lg[r]).max() <= bar


# ---- the widest geometry the one launch takes: T = 32 fills the softmax wave and the LDS staging, C = 64 every lane of the arg-max.
# Error bars as above, from this geometry's own numbers (tests/golden/attn_decode_limits.npz).
LIMIT_FORCED = (2, 2, 64, 32, 1)               # (B, L, C, T, feature seed)
# seed: the first at which both rows' greedy margins exceed the bound in both directions, found by tools/gen_golden_moran.py with the
# float64 specification on the CPU and recorded in the fixture
LIMIT_GREEDY = (2, 4, 64, 32, 1)


@pytest.fixture(scope="module")
def lim():
    lim = np.load(os.path.join(GOLD, "attn_decode_limits.npz"))
    assert tuple(lim["moran_forced_case"]) == LIMIT_FORCED and tuple(lim["moran_greedy_case"]) == LIMIT_GREEDY
    return lim


def _limit_inputs(case):
    B, L, C, T, seed = case
    return R.features(B, T, seed), torch.randint(0, C + 1, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("d", [0, 1])
def test_forced_logits_at_the_limits(d, lim):
    B, L, C, T, _ = LIMIT_FORCED
    att, P = _head(d, C)
    x, tg = _limit_inputs(LIMIT_FORCED)
    want = R.forced(P, x.numpy(), tg.numpy())
    bar, _ = R.margin_bound(lim["moran_forced_ref_err"][d], lim["moran_forced_maxabs"][d])
    before = moran.LAUNCHES["one_launch"]
    for route in (moran.attn_decode, moran.decode_eager):
        got = route(att, x.to(DEV), 0, targets=tg.to(DEV))
        assert got is not None and tuple(got.shape) == (B, L, C)
        err = float(np.abs(got.cpu().numpy().astype(np.float64) - want).max())
        print("forced at the limits %s %s: error %.3e, reference fp32 %.3e, bar %.3e" % (DIRS[d], route.__name__, err,
                                                                                        lim["moran_forced_ref_err"][d], bar))
        assert err <= bar, (route.__name__, err, bar)
    assert moran.LAUNCHES["one_launch"] == before + 1


@pytest.mark.parametrize("d", [0, 1])
def test_greedy_at_the_limits(d, lim):
    B, L, C, T, _ = LIMIT_GREEDY
    att, P = _head(d, C)
    x = _limit_inputs(LIMIT_GREEDY)[0]
    want_ids, want_lg, margin = R.greedy(P, x.numpy(), L)
    bar, need = R.margin_bound(max(lim["moran_forced_ref_err"].max(), lim["moran_greedy_ref_err"].max()),
                               max(lim["moran_forced_maxabs"].max(), lim["moran_greedy_maxabs"].max()))
    assert (margin > need).all(), (margin, need)                                  # (the seed: every row is compared)
    before = moran.LAUNCHES["one_launch"]
    for route in (moran.attn_decode, moran.decode_eager):
        ids, lg = route(att, x.to(DEV), 1, steps=L)
        assert ids.dtype == torch.int32 and tuple(ids.shape) == (B, L) and tuple(lg.shape) == (B, L, C)
        ids, lg = ids.cpu().numpy(), lg.cpu().numpy().astype(np.float64)
        assert np.array_equal(ids, want_ids), (route.__name__, ids, want_ids)
        err = np.abs(lg - want_lg).max()
        print("greedy at the limits %s %s: logits error %.3e, bar %.3e" % (DIRS[d], route.__name__, err, bar))
        assert err <= bar
        assert np.array_equal(lg.argmax(2), ids)                                  # the ids are the arg-max of the logits returned
    assert moran.LAUNCHES["one_launch"] == before + 1
