"""bn2 and the residual sum of a residual block applied by the GruBlocks' own kernels on the way in (functional.SRB_IN_FOLD:
tatt_tokgemm_sb_in, tatt_gru_wgrad_frag_in) instead of being written out by tatt_bn_apply / tatt_axpby in front of them.

The transform is per element and rounds as the stand-alone kernels round (common.h bn_affine_f; a + b is a + b), and every kernel
downstream is the same one on the same values, so the folded operator is compared with its own unfolded form by torch.equal: the
output, the gradient of every input and all ten parameter gradients.  Against float64 the bounds are test_gru_block_fused's."""
import functools

import pytest
import torch

from oracle import tatt_oracle as O
from oracle.fixtures import make_inputs
from tests.util import check_close

pytestmark = pytest.mark.gpu
STD = dict(scale_factor=2, width=128, height=32, STN=True, mask=True, srb_nums=5, hidden_units=32)
# (1, 8, 32): the smallest geometry both kernels take -- M = 256 = 4 token tiles, T = 8 (vertical) and 32, 8 fragment chunks.
# (17, 16, 64): 272 token tiles on 256 persistent work-groups (some stage a second tile through the prefetch path) and 544 fragment
# chunks on 128 groups (an uneven split).
SHAPES = [(1, 8, 32), (17, 16, 64)]
CASES = ["gru1", "gru2"]            # gru1: BatchNorm form, text-prior half, vertical;  gru2: sum form, horizontal


def R(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.randn(*shape, generator=g) * scale


def _block(dev):
    from tatt_amd.tsrn import RecurrentResidualBlock
    torch.manual_seed(5)
    blk = RecurrentResidualBlock(64, 64).to(dev).train()
    with torch.no_grad():
        blk.bn2.weight.add_(0.3 * R(64).to(dev))
        blk.bn2.bias.add_(0.3 * R(64, seed=1).to(dev))
        blk.conv2.bias.add_(R(64, seed=4).to(dev))          # y2 with a non-zero per-channel mean
    return blk


def _y2_stats(blk, B, H, W, dev):
    """the pre-BatchNorm map and bn2's batch statistics over it: from conv_bn (ConvBnFn) where it takes the geometry; for a width its
    convolution does not take, the unfused convolution and the statistics in torch (the fold does not care where they come from)"""
    from tatt_amd import functional as Fh, ops
    x = (R(B, H, W, 64, seed=2) + 0.5).to(dev)
    with torch.no_grad():
        if ops.conv3_bn_fusable(x, blk.conv2.weight, blk.bn2):
            y2, st = Fh.conv_bn(x, blk.conv2, blk.bn2)
            return y2.detach(), st[0].detach(), st[1].detach()
        y2 = Fh.conv2d(x, blk.conv2.weight, blk.conv2.bias)
        f = y2.reshape(-1, 64).double()
        return y2, f.mean(0).float(), (1.0 / torch.sqrt(f.var(0, unbiased=False) + blk.bn2.eps)).float()


def _inputs(which, B, H, W, dev):
    blk = _block(dev)
    if which == "gru1":
        y2, mean, rstd = _y2_stats(blk, B, H, W, dev)
        return blk, dict(y2=y2, mean=mean, rstd=rstd, xb=R(B, H, W, 64, seed=7).to(dev))
    return blk, dict(a=(R(B, H, W, 64, seed=8) + 0.25).to(dev), b=R(B, H, W, 64, seed=9).to(dev))


def _run_once(dev, which, shape, fold):
    """the GruBlock on a folded-form input with the switch as given -> {name: tensor on the CPU} (output, input and parameter gradients)"""
    from tatt_amd import functional as Fh
    B, H, W = shape
    blk, t = _inputs(which, B, H, W, dev)
    for p in blk.parameters():
        p.grad = None
    leaves = {k: v.clone().requires_grad_(True) for k, v in t.items() if k not in ("mean", "rstd")}
    old = Fh.SRB_IN_FOLD
    Fh.SRB_IN_FOLD = fold
    try:
        if which == "gru1":
            gb = blk.gru1
            out = Fh.gru_block((leaves["y2"], t["mean"], t["rstd"], blk.bn2.weight, blk.bn2.bias), gb, True, xb=leaves["xb"])
        else:
            gb = blk.gru2
            out = Fh.gru_block((leaves["a"], leaves["b"]), gb, False)
        (out * R(B, H, W, 64, seed=3).to(dev)).sum().backward()
    finally:
        Fh.SRB_IN_FOLD = old
    torch.cuda.synchronize()
    d = {"out": out}
    d.update({"d." + k: v.grad for k, v in leaves.items()})
    if which == "gru1":
        d["d.gamma"], d["d.beta"] = blk.bn2.weight.grad, blk.bn2.bias.grad
    params = list(gb.named_parameters())
    assert len(params) == 10
    d.update({"g." + n: p.grad for n, p in params})
    assert all(v is not None for v in d.values()), [k for k, v in d.items() if v is None]
    return {k: v.detach().cpu().clone() for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def _run(dev, which, shape, fold):
    """computed once, shared by the tests, never modified"""
    return _run_once(dev, which, shape, fold)


@functools.lru_cache(maxsize=None)
def _oracle(dev, which, shape):
    """float64: O.gru_block on the train-mode BatchNorm of y2 (batch statistics of y2 itself, so the gradient of y2 carries their
    dependence on it), respectively on a + b"""
    B, H, W = shape
    blk, t = _inputs(which, B, H, W, dev)
    gb = blk.gru1 if which == "gru1" else blk.gru2
    ps = {n: p.detach().cpu().double().requires_grad_(True) for n, p in gb.named_parameters()}
    sd = {"b." + n: p for n, p in ps.items()}
    lv = {k: v.detach().cpu().double().requires_grad_(True) for k, v in t.items() if k not in ("mean", "rstd")}
    if which == "gru1":
        lv["gamma"] = blk.bn2.weight.detach().cpu().double().requires_grad_(True)
        lv["beta"] = blk.bn2.bias.detach().cpu().double().requires_grad_(True)
        f = lv["y2"].reshape(-1, 64)
        xhat = (lv["y2"] - f.mean(0)) / torch.sqrt(f.var(0, unbiased=False) + blk.bn2.eps)
        inp = torch.cat([xhat * lv["gamma"] + lv["beta"], lv["xb"]], -1).permute(0, 3, 1, 2)
        out = O.gru_block(inp.transpose(-1, -2), sd, "b").transpose(-1, -2).permute(0, 2, 3, 1)          # vertical
    else:
        out = O.gru_block((lv["a"] + lv["b"]).permute(0, 3, 1, 2), sd, "b").permute(0, 2, 3, 1)
    (out * R(B, H, W, 64, seed=3).double()).sum().backward()
    d = {"out": out.detach()}
    d.update({"d." + k: v.grad for k, v in lv.items()})
    d.update({"g." + n: p.grad for n, p in ps.items()})
    return d


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("which", CASES)
def test_fold_equals_unfolded_bitwise(dev, which, shape):
    """1. the operator against its own unfolded form: torch.equal on the output, the gradients of y2 / a, b, xb, gamma, beta and the ten
    parameter gradients; and the folded run did take the two new entries."""
    from tatt_amd import ops
    calls = []
    real = ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        on = _run_once(dev, which, shape, True)
    finally:
        ops.call = real
    assert "tatt_tokgemm_sb_in" in calls and "tatt_gru_wgrad_frag_in" in calls, calls
    assert "tatt_bn_apply" not in calls and "tatt_axpby" not in calls, calls
    off = _run(dev, which, shape, False)
    assert on.keys() == off.keys()
    bad = []
    for k in on:
        diff = float((on[k].double() - off[k].double()).abs().max())
        print("%s %s %-28s max|on - off| = %.3e of %.3e" % (which, shape, k, diff, float(off[k].abs().max())))
        if not torch.equal(on[k], off[k]):
            bad.append("%s: %.3e" % (k, diff))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("which", CASES)
def test_fold_against_float64(dev, which, shape):
    """2. the folded operator against the float64 composition, with the bounds of test_gru_block_fused: output rtol 2e-4 / atol 2e-5;
    gradients of the input maps rtol 1e-3 / atol 5e-5 max(1, max|g|); parameter gradients (gamma and beta are parameters too)
    rtol 2e-3 / atol 2e-4 max|g|."""
    on, ref = _run(dev, which, shape, True), _oracle(dev, which, shape)
    assert on.keys() == ref.keys()
    for k, g in on.items():
        r = ref[k].float()
        if k == "out":
            check_close(k, g, r)
        elif k in ("d.gamma", "d.beta") or k.startswith("g."):
            check_close(k, g, r, rtol=2e-3, atol=2e-4 * float(r.abs().max()))
        else:
            check_close(k, g, r, rtol=1e-3, atol=5e-5 * max(1.0, float(r.abs().max())))


@pytest.mark.parametrize("which", CASES)
def test_fallback_routing(dev, which):
    """3. (3, 5, 7): M = 105 tokens, neither kernel applies -- the map is written out, the switch changes nothing and no new entry runs"""
    from tatt_amd import ops
    calls = []
    real = ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        on = _run_once(dev, which, (3, 5, 7), True)
    finally:
        ops.call = real
    off = _run(dev, which, (3, 5, 7), False)
    assert not [c for c in calls if c.endswith("_in")], calls
    assert ("tatt_bn_apply" if which == "gru1" else "tatt_axpby") in calls
    for k in on:
        assert torch.equal(on[k], off[k]), k


def test_whole_step_bitwise(dev):
    """4. one TATT training step (B = 2, 16x64, STN on, dropout on, same seed) with the switch on and off: the loss, the gradient norm,
    every parameter and every BatchNorm buffer after the step are equal"""
    import tatt_amd
    from tatt_amd import functional as Fh
    from tatt_amd.train import Trainer
    from oracle.fixtures import randomize_state_dict
    from tatt_amd import ops
    res, calls = [], []
    old, real = Fh.SRB_IN_FOLD, ops.call
    ops.call = lambda name, *a: (calls.append((Fh.SRB_IN_FOLD, name)), real(name, *a))[1]
    try:
        for fold in (True, False):
            Fh.SRB_IN_FOLD = fold
            torch.manual_seed(1234)
            m = tatt_amd.TSRN_TL_TRANS(**STD)
            m.load_state_dict(randomize_state_dict(m.state_dict()))
            m = m.to(dev).train()
            m.infoGen.dropout_on = True
            Fh.set_seed(dev, 99)
            tr = Trainer(m, use_graph=False)
            x, tp, hr = make_inputs(2, seed=41)
            loss = tr.step(x.to(dev), tp.to(dev), hr.to(dev))
            torch.cuda.synchronize()
            d = {"loss": torch.as_tensor(loss).detach().reshape(-1), "grad_norm": torch.as_tensor(tr.last_grad_norm).detach().reshape(-1)}
            d.update({k: v for k, v in m.state_dict().items()})
            res.append({k: v.detach().cpu().clone() for k, v in d.items()})
    finally:
        Fh.SRB_IN_FOLD, ops.call = old, real
    # five residual blocks: gru1 and gru2 of each take the folded entries with the switch on, none with it off
    assert calls.count((True, "tatt_tokgemm_sb_in")) == 10 and calls.count((True, "tatt_gru_wgrad_frag_in")) == 10
    assert not [c for c in calls if c[0] is False and c[1].endswith("_in")]
    print("loss %.9g / %.9g, grad norm %.9g / %.9g" % (float(res[0]["loss"]), float(res[1]["loss"]), float(res[0]["grad_norm"]),
                                                     float(res[1]["grad_norm"])))
    assert res[0].keys() == res[1].keys()
    bad = [k for k in res[0] if not torch.equal(res[0][k], res[1][k])]
    assert not bad, bad


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("K", [64, 128])
def test_gru_tail(dev, K, compact):
    """5. tatt_gru_tail / tatt_gru_tail_c (the gradients of the composed projection mapped back; dW_hh given as the (192, 64) product or
    compact (192, 32)) against float64 matrix products, with the bounds test_gru_block_fused uses for these gradients"""
    from tatt_amd import ops
    dWp, dbp, Wc, bc = R(192, K, seed=1), R(192, seed=2), R(64, K, seed=3, scale=0.2), R(64, seed=4, scale=0.2)
    wih = [R(96, 64, seed=5, scale=0.2), R(96, 64, seed=6, scale=0.2)]
    dWhh = R(192, 32 if compact else 64, seed=7)
    g = [t.to(dev) for t in (dWp, dbp, Wc, bc, wih[0], wih[1], dWhh)]
    dwih = [torch.empty(96, 64, device=dev) for _ in range(2)]
    dwhh = [torch.empty(96, 32, device=dev) for _ in range(2)]
    dWc, dbc = torch.empty(64, K, device=dev), torch.empty(64, device=dev)
    P = ops.P
    ops.call("tatt_gru_tail_c" if compact else "tatt_gru_tail", P(g[0]), P(g[1]), P(g[2]), P(g[3]), P(g[4]), P(g[5]), P(dwih[0]),
             P(dwih[1]), P(dWc), P(dbc), K, P(g[6]), P(dwhh[0]), P(dwhh[1]), ops.stream())
    D = lambda t: t.double()
    want = {"dWc": D(wih[0]).t() @ D(dWp[:96]) + D(wih[1]).t() @ D(dWp[96:]),
            "dbc": D(wih[0]).t() @ D(dbp[:96]) + D(wih[1]).t() @ D(dbp[96:])}
    got = {"dWc": dWc, "dbc": dbc}
    for d in range(2):
        rows = slice(96 * d, 96 * d + 96)
        want["dwih%d" % d] = D(dWp[rows]) @ D(Wc).t() + torch.outer(D(dbp[rows]), D(bc))
        want["dwhh%d" % d] = D(dWhh[rows]) if compact else D(dWhh[rows, 32 * d:32 * d + 32])
        got["dwih%d" % d], got["dwhh%d" % d] = dwih[d], dwhh[d]
    for k, w in want.items():
        check_close(k, got[k], w.float(), rtol=2e-3, atol=2e-4 * float(w.abs().max()))
