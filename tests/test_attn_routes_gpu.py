"""The short-key attention core (tatt_attn_fwd / tatt_attn_bwd) and the row softmax (tatt_softmax_rows_*) of csrc/attn.hip against the
float64 specifications of tests/norm_attn_ref.py, at the edges of their geometry: S = 1 .. 32 keys (no padding lanes at 32; 17 .. 31: the
second MFMA accumulator's row mask), a clamped last block of 64 queries (Lq = 1, 63, 65, 130), every combination of the two upstream
gradients, dropout with the mask recovered from tatt_dropout; row lengths round the wave (64), the work-group (256) and the limit (4096).
Backward references: float64 autograd of the specification.  Outputs of the direct C-ABI calls lie inside canaries.

Error bars: NR.judge, 4 x unit + k x EPS32 x max|reference|; k = fp32 roundings on the longest dependent chain (a chain counts its length):
  attention  probabilities   22 + S    16 fused multiply-adds of a score, the max subtraction, __expf (2), the sum over S, 1 / sum, the product
             ctx             24 + 2S   the dropout scale, S fused multiply-adds
             wavg            27 + S    the dropout scale, two cross-lane adds, 0.25 (exact)
             dQ              44 + 3S   d = 16 fused multiply-adds + dwavg (2) + the scale, dot over S, p (d - dot) (2), S fused multiply-adds
             dV              88 + S + blocks    the dropped probability, 64 queries on the matrix core, the per-block partials in a chain
             dK              108 + 2S + blocks  the score gradient (44 + 2S), 64 queries, the partials
  softmax    P, Pd           31        max (exact), subtraction, __expf (2), 16 per thread + log2 64 + 3 across the group, 1 / sum, the product,
                                       the dropout scale
             dS              60        the kernel's own P (31), the scale, the dot product (25), g - dot, the product

Measured on the MI355X (unit / bar / error; gradients with both upstream gradients given):
  attention B=3 Lq=65 S=17 p=0.1   ctx 1.768e-06 / 3.057e-05 / 1.708e-06   wavg 1.425e-07 / 3.967e-06 / 1.475e-07   dQ 8.625e-06 / 2.062e-04 / 6.718e-06
                                   dK 5.607e-06 / 3.203e-04 / 7.013e-06    dV 2.701e-06 / 1.372e-04 / 2.701e-06
  attention B=3 Lq=65 S=32 p=0.1   ctx 2.451e-06 / 4.865e-05 / 2.481e-06   wavg 1.816e-07 / 4.673e-06 / 1.912e-07   dQ 6.112e-06 / 2.526e-04 / 1.074e-05
                                   dK 5.688e-06 / 3.180e-04 / 6.476e-06    dV 1.986e-06 / 9.852e-05 / 2.034e-06
  attention B=3 Lq=130 S=1 p=0     dV 9.040e-06 / 3.887e-04 / 6.561e-06 (dQ, dK exactly zero, as in float64)
  scores of +-60, p=0.1            ctx 4.864e-06 / 5.721e-05 / 4.864e-06   dQ 1.739e-05 / 2.841e-04 / 1.739e-05   dK 2.960e-05 / 7.421e-04 / 3.226e-05
  all scores equal, p=0            wavg 2.191e-10 / 3.094e-07 / 2.191e-10  dK 2.488e-06 / 1.542e-04 / 1.341e-06
  softmax rows=3 L=257  p=0.1      P 3.339e-08 / 1.059e-06 / 5.992e-09     Pd 1.205e-08 / 1.076e-06 / 9.496e-09     dS 4.627e-08 / 1.972e-06 / 1.512e-08
  softmax rows=3 L=4096 p=0.1      P 1.489e-08 / 1.665e-06 / 7.104e-09     Pd 1.817e-08 / 1.856e-06 / 5.702e-09     dS 5.180e-08 / 1.468e-06 / 2.200e-08
What this file found: no wrong value -- all 67 tests pass on the kernels as they were, and no canary changed.
"""
import pytest
import torch

from tests import norm_attn_ref as NR

pytestmark = pytest.mark.gpu
P_DROP = 0.1
AT_SMAX, AT_QPB, SM_MAX = 32, 64, 4096

# ---- attention -----------------------------------------------------------------------------------------------------------------------
ALL_LQ, ALL_S = (1, 63, 64, 65, 130), (1, 2, 15, 16, 17, 26, 31, 32)
LQ_S = sorted({(65, S) for S in ALL_S} | {(Lq, 26) for Lq in ALL_LQ} | {(1, 1), (1, 32), (130, 1), (130, 32)})
ATTN_CASES = [(B, Lq, S) for B in (1, 3) for Lq, S in LQ_S]


def _check_attn_cases():
    rows = [{"second accumulator holds rows": S > 16, "padding lanes": S < AT_SMAX, "row mask s1 < S cuts": 16 < S < AT_SMAX,
             "clamped tail block": Lq % AT_QPB != 0, "more than one block": Lq > AT_QPB, "one key": S == 1, "one query": Lq == 1,
             "batch > 1": B > 1} for B, Lq, S in ATTN_CASES]
    for name in rows[0]:
        assert {r[name] for r in rows} == {True, False}, name
    assert {S for _, _, S in ATTN_CASES} == set(ALL_S) and {Lq for _, Lq, _ in ATTN_CASES} == set(ALL_LQ)


_check_attn_cases()


def _seed(dev, value=0x0BADC0DE12345 & 0x7FFFFFFFFFFFFFFF):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _attn_inputs(B, Lq, S, seed=0):
    gen = torch.Generator().manual_seed(500 + 7 * B + 131 * Lq + S + seed)
    Q, K, V = torch.randn(B, Lq, 64, generator=gen), torch.randn(B, S, 64, generator=gen), torch.randn(B, S, 64, generator=gen)
    dctx, dwavg = torch.randn(B, Lq, 64, generator=gen), torch.randn(B, Lq, S, generator=gen)
    return Q, K, V, dctx, dwavg


GRADS = ("both", "dctx", "dwavg")


def _attn_reference(Q, K, V, dctx, dwavg, mask):
    """-> {dtype: {"ctx", "wavg", ("dQ", which), ...}} by autograd of the specification in that dtype"""
    out = {}
    for dt in (torch.float64, torch.float32):
        q, k, v = (t.to(dt).clone().requires_grad_() for t in (Q, K, V))
        ctx, wavg = NR.attn_core(q, k, v, None if mask is None else mask.to(dt))
        r = {"ctx": ctx.detach(), "wavg": wavg.detach()}
        for which in GRADS:
            loss = 0.0
            if which != "dwavg":
                loss = loss + (ctx * dctx.to(dt)).sum()
            if which != "dctx":
                loss = loss + (wavg * dwavg.to(dt)).sum()
            gs = torch.autograd.grad(loss, [q, k, v], retain_graph=True, allow_unused=True)      # (wavg alone does not depend on V)
            for name, g, leaf in zip(("dQ", "dK", "dV"), gs, (q, k, v)):
                r[(name, which)] = g if g is not None else torch.zeros_like(leaf)
        out[dt] = r
    return out[torch.float64], out[torch.float32]


def _k_attn(name, S, Lq):
    blocks = -(-Lq // AT_QPB)
    return {"ctx": 24 + 2 * S, "wavg": 27 + S, "dQ": 44 + 3 * S, "dV": 88 + S + blocks, "dK": 108 + 2 * S + blocks}[name]


def _attn_direct(ops, dev, Q, K, V, dctx, dwavg, p, seed, site):
    """both launches through the C ABI into canaried buffers -> ctx, wavg, dQ, dK, dV, canaries intact"""
    B, Lq, _ = Q.shape
    S = K.shape[1]
    flat = lambda n: NR.box2d(None, 1, n, "contig", dev)
    cb, wb, qb, kb, vb = flat(B * Lq * 64), flat(B * Lq * S), flat(B * Lq * 64), flat(B * S * 64), flat(B * S * 64)
    ops.call("tatt_attn_fwd", ops.P(Q), ops.P(K), ops.P(V), ops.P(cb.v), ops.P(wb.v), B, Lq, S, p, ops.P(seed), site, ops.stream())
    part = NR.box2d(None, 1, B * (-(-Lq // AT_QPB)) * 2 * S * 64, "contig", dev)
    ops.call("tatt_attn_bwd", ops.P(Q), ops.P(K), ops.P(V), ops.P(dctx), ops.P(dwavg), ops.P(qb.v), ops.P(kb.v), ops.P(vb.v), ops.P(part.v),
             B, Lq, S, p, ops.P(seed), site, ops.stream())
    boxes = [cb, wb, qb, kb, vb, part]
    return [t.v.reshape(-1) for t in boxes[:5]], all(t.intact() for t in boxes)


def _run_attention(dev, case, Q, K, V, dctx, dwavg, drops=(0.0, P_DROP)):
    from tatt_amd import ops
    B, Lq, S = Q.shape[0], Q.shape[1], K.shape[1]
    seed, site = _seed(dev), 11
    Qd, Kd, Vd, dcd, dwd = (t.to(dev) for t in (Q, K, V, dctx, dwavg))
    failed = []
    for p in drops:
        mask = NR.recover_mask((B, 4, Lq, S), p, seed, site, dev) if p > 0 else None
        r64, r32 = _attn_reference(Q, K, V, dctx, dwavg, mask)
        assert all(bool(torch.isfinite(t).all()) for t in r64.values())
        tag = "%s p=%.1f" % (case, p)
        ctx, wavg = ops.attn_fwd(Qd, Kd, Vd, p, seed, site)
        ctx_only, none = ops.attn_fwd(Qd, Kd, Vd, p, seed, site, need_weights=False)
        assert none is None and torch.equal(ctx_only, ctx), tag + ": ctx differs without the weights"
        for name, t in (("ctx", ctx), ("wavg", wavg)):
            failed.append(NR.judge(tag, name, t, r64[name], r32[name], _k_attn(name, S, Lq)))
        grads = {}
        for which in GRADS:
            dc = dcd if which != "dwavg" else torch.zeros_like(dcd)
            dw = dwd if which != "dctx" else None
            grads[which] = ops.attn_bwd(Qd, Kd, Vd, dc, dw, p, seed, site)
            for name, t in zip(("dQ", "dK", "dV"), grads[which]):
                failed.append(NR.judge(tag, "%s(%s)" % (name, which), t, r64[(name, which)], r32[(name, which)], _k_attn(name, S, Lq),
                                       grad=True))
        direct, intact = _attn_direct(ops, dev, Qd, Kd, Vd, dcd, dwd, p, seed, site)
        same = [torch.equal(a, b.reshape(-1)) for a, b in zip(direct, (ctx, wavg) + tuple(grads["both"]))]
        if not all(same):
            failed.append((tag, "the call into canaried buffers differs", same))
        if not intact:
            failed.append((tag, "a canary changed"))
    return [f for f in failed if f]


@pytest.mark.parametrize("B,Lq,S", ATTN_CASES)
def test_attention_core_against_float64(dev, B, Lq, S):
    failed = _run_attention(dev, "attn B=%d Lq=%d S=%d" % (B, Lq, S), *_attn_inputs(B, Lq, S))
    assert not failed, failed[:8]


def test_attention_scores_of_plus_minus_60(dev):
    """the max subtraction: Q scaled so that the scores span about +-60 (exp(60) squared is beyond fp32)"""
    B, Lq, S = 3, 65, 26
    Q, K, V, dctx, dwavg = _attn_inputs(B, Lq, S, seed=1)
    sc = torch.einsum("bqhd,bshd->bhqs", Q.view(B, Lq, 4, 16).double(), K.view(B, S, 4, 16).double())
    Q = Q * float(60.0 / sc.abs().max())
    sc = torch.einsum("bqhd,bshd->bhqs", Q.view(B, Lq, 4, 16).double(), K.view(B, S, 4, 16).double())
    assert 59.0 < float(sc.max()) < 61.0 or 59.0 < float(-sc.min()) < 61.0
    assert float(sc.max()) > 40.0 and float(sc.min()) < -40.0
    ctx, wavg = NR.attn_core(Q.double(), K.double(), V.double(), None)
    assert bool(torch.isfinite(ctx).all()) and bool(torch.isfinite(wavg).all())          # (the float64 reference, on the CPU)
    failed = _run_attention(dev, "attn scores +-60", Q, K, V, dctx, dwavg)
    assert not failed, failed[:8]


def test_attention_all_scores_equal(dev):
    B, Lq, S = 1, 65, 17
    Q, K, V, dctx, dwavg = _attn_inputs(B, Lq, S, seed=2)
    K = K[:, :1].expand(B, S, 64).contiguous()                # every key the same: every probability 1 / S
    w = NR.attn_core(Q.double(), K.double(), V.double(), None)[1]
    assert float((w - 1.0 / S).abs().max()) < 1e-15
    failed = _run_attention(dev, "attn equal scores", Q, K, V, dctx, dwavg)
    assert not failed, failed[:8]


@pytest.mark.parametrize("S", [0, 33])
def test_attention_refuses_key_counts_outside_1_to_32(dev, S):
    from tatt_amd import ops
    Q, K = torch.randn(1, 5, 64, device=dev), torch.randn(1, max(S, 1), 64, device=dev)[:, :S]
    with pytest.raises(RuntimeError, match="tatt_attn_fwd failed with code 1"):
        ops.attn_fwd(Q, K, K, 0.0, _seed(dev), 0)
    with pytest.raises(RuntimeError, match="tatt_attn_bwd failed with code 1"):
        ops.attn_bwd(Q, K, K, Q, None, 0.0, _seed(dev), 0)


@pytest.mark.parametrize("which", ["dctx", "dwavg"])
@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_attention_function_with_one_gradient_missing(dev, which, p):
    """functional.AttnCoreFn when autograd hands over no gradient for one of the two outputs (dc is None / dw is None)"""
    from tatt_amd import functional as Fh
    B, Lq, S = 3, 65, 26
    Q, K, V, dctx, dwavg = _attn_inputs(B, Lq, S, seed=3)
    Fh.set_seed(dev, 4242)
    site = 6
    mask = NR.recover_mask((B, 4, Lq, S), p, Fh.current_seed(dev), site, dev) if p > 0 else None
    r64, r32 = _attn_reference(Q, K, V, dctx, dwavg, mask)
    q, k, v = (t.to(dev).requires_grad_() for t in (Q, K, V))
    ctx, wavg = Fh.AttnCoreFn.apply(q, k, v, p, site)
    loss = (ctx * dctx.to(dev)).sum() if which == "dctx" else (wavg * dwavg.to(dev)).sum()
    loss.backward()
    tag = "AttnCoreFn %s alone p=%.1f" % (which, p)
    failed = [NR.judge(tag, "ctx", ctx, r64["ctx"], r32["ctx"], _k_attn("ctx", S, Lq)),
              NR.judge(tag, "wavg", wavg, r64["wavg"], r32["wavg"], _k_attn("wavg", S, Lq))]
    for name, t in (("dQ", q.grad), ("dK", k.grad), ("dV", v.grad)):
        failed.append(NR.judge(tag, name, t, r64[(name, which)], r32[(name, which)], _k_attn(name, S, Lq), grad=True))
    failed = [f for f in failed if f]
    assert not failed, failed


# ---- row softmax ---------------------------------------------------------------------------------------------------------------------
SM_L = (1, 2, 37, 63, 64, 65, 255, 256, 257, 1024, 4095, 4096)
SM_CASES = [(rows, L) for rows in (1, 3) for L in SM_L]
K_SM = {"P": 31, "Pd": 31, "dS": 60}


def _check_softmax_cases():
    rows = [{"beyond one wave": L > 64, "beyond one element per thread": L > 256, "threads without an element": L < 256,
             "a ragged last round": L % 256 != 0, "the limit": L == SM_MAX, "more than one row": r > 1} for r, L in SM_CASES]
    for name in rows[0]:
        assert {r[name] for r in rows} == {True, False}, name


_check_softmax_cases()


def _softmax_inputs(rows, L):
    gen = torch.Generator().manual_seed(300 + 5 * rows + L)
    S = 3.0 * torch.randn(rows, L, generator=gen)
    if rows == 3:                                             # one row shifted up, one down, one of equal values
        S[0] += 80.0
        S[1] -= 80.0
        S[2] = 0.7
    return S, torch.randn(rows, L, generator=gen)


def _softmax_reference(S, dPd, mask):
    out = {}
    for dt in (torch.float64, torch.float32):
        s = S.to(dt).clone().requires_grad_()
        P, Pd = NR.softmax_rows(s, None if mask is None else mask.to(dt))
        (dS,) = torch.autograd.grad((Pd * dPd.to(dt)).sum(), s)
        out[dt] = {"P": P.detach(), "Pd": Pd.detach(), "dS": dS}
    return out[torch.float64], out[torch.float32]


@pytest.mark.parametrize("rows,L", SM_CASES)
def test_softmax_rows_against_float64(dev, rows, L):
    from tatt_amd import ops
    S, dPd = _softmax_inputs(rows, L)
    seed, site = _seed(dev), 9
    failed = []
    for p, with_pd in ((0.0, False), (0.0, True), (P_DROP, True)):
        mask = NR.recover_mask((rows, L), p, seed, site, dev) if p > 0 else None
        r64, r32 = _softmax_reference(S, dPd, mask)
        tag = "softmax rows=%d L=%d p=%.1f %s" % (rows, L, p, "Pd" if with_pd else "no Pd")
        sb = NR.box2d(S, 1, rows * L, "contig", dev)                                  # overwritten in place by P
        pb = NR.box2d(None, 1, rows * L, "contig", dev) if with_pd else None
        ops.call("tatt_softmax_rows_fwd", ops.P(sb.v), ops.P(pb.v) if with_pd else None, rows, L, p, ops.P(seed), site, ops.stream())
        P = sb.v.reshape(rows, L)
        failed.append(NR.judge(tag, "P", P, r64["P"], r32["P"], K_SM["P"]))
        if with_pd:
            Pd = pb.v.reshape(rows, L)
            failed.append(NR.judge(tag, "Pd", Pd, r64["Pd"], r32["Pd"], K_SM["Pd"]))
            if p <= 0:
                assert torch.equal(Pd, P)
            else:
                assert torch.equal(Pd == 0, (mask.to(dev) == 0) | (P == 0))
        db = NR.box2d(dPd, 1, rows * L, "contig", dev)                                # overwritten in place by dS
        ops.call("tatt_softmax_rows_bwd", ops.P(sb.v), ops.P(db.v), rows, L, p, ops.P(seed), site, ops.stream())
        failed.append(NR.judge(tag, "dS", db.v.reshape(rows, L), r64["dS"], r32["dS"], K_SM["dS"], grad=True))
        if not all(b.intact() for b in (sb, pb, db) if b is not None):
            failed.append((tag, "a canary changed"))
    failed = [f for f in failed if f]
    assert not failed, failed[:8]


@pytest.mark.parametrize("rows,L", [(3, 37), (3, 4096)])
def test_softmax_rows_function(dev, rows, L):
    from tatt_amd import functional as Fh
    S, dP = _softmax_inputs(rows, L)
    r64, r32 = _softmax_reference(S, dP, None)
    s = S.to(dev).requires_grad_()
    P = Fh.SoftmaxRowsFn.apply(s)
    P.backward(dP.to(dev))
    assert torch.equal(s.detach(), S.to(dev))                 # (the function works on a copy)
    tag = "SoftmaxRowsFn rows=%d L=%d" % (rows, L)
    failed = [f for f in (NR.judge(tag, "P", P, r64["P"], r32["P"], K_SM["P"]),
                          NR.judge(tag, "dS", s.grad, r64["dS"], r32["dS"], K_SM["dS"], grad=True)) if f]
    assert not failed, failed


def test_softmax_rows_refuses_4097(dev):
    from tatt_amd import ops
    S = torch.randn(2, SM_MAX + 1, device=dev)
    for name in ("tatt_softmax_rows_fwd", "tatt_softmax_rows_bwd"):
        with pytest.raises(RuntimeError, match=name + " failed with code 1"):
            ops.call(name, ops.P(S), ops.P(S.clone()), 2, SM_MAX + 1, 0.0, ops.P(_seed(dev)), 0, ops.stream())
