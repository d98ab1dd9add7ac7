"""BatchNorm and LayerNorm (csrc/norm.hip) against the float64 specifications of tests/norm_attn_ref.py at every route their host code can
take.  The operators are called through tatt_amd.ops on maps with chosen strides and alignment, every output inside canaries
(tests/step_tail_ref.py), every input inside NaNs; one pass per family goes through functional.BatchNormActFn / LayerNormFn.

The host predicates are restated below (`v4_ok`, `apply_v4`, `bwd_v4`, `cs_groups`) ONLY to label the cases: at collection time the case
lists must hold a case on each side of every clause, so that a later edit of a list cannot silently lose a route.

Error bars: NR.judge, 4 x unit + k x EPS32 x max|reference|, unit = the float32 CPU run of the specification against its float64 run on
the same inputs (and mask), measured inside the test.  k = fp32 roundings on the kernel's longest dependent chain for that output:
  BatchNorm   mean, rstd     2   sums, mean, variance and 1 / sqrt in fp64 (bn_stats_stage1 / _stage2), rounded once; +1 for the constant
              rstd (eval)    3   bn_rstd_kernel: add, sqrtf, divide in fp32
              running stats  3   fp64 blend of the fp32 old value, rounded once; the blend's operands carry a rounding each
              y              5   bn_apply: subtract, two products, add (a fused multiply-add or not), the activation's select;
                                 +7 for mish (x log2 e, v_exp, e (e + 2): 2, n + 2, v_rcp, two products less one shared)
              dx            13   xhat 2, pre-activation 2, du 1, two means times 1 / M: 4, two subtractions, gamma rstd v: 2;
                                 +10 for mish' (the 7 of mish, a second v_rcp, 1 - t t, two products)
              dgamma, dbeta  6   per term xhat 2, du 1 (+10 mish'), product 1, then fp64 sums rounded once
              coef           7   a: 1; b = -a rstd (q / M): 4; c = -a (s / M) - b mean: 3 more
              dx (affine)    9   two fused multiply-adds on coefficients of up to 7
  LayerNorm   y             30   row sum: 4 per lane in a chain + log2 64 across the wave = 10, / C, x - mu, the sum of squares: 12,
                                 / C + eps, sqrtf, reciprocal: 4, (x - mu) rs gamma + beta: 3
              dx, dB        34   xhat 2, dy gamma 1, two row sums of C: 10 and 12, c2: 3, rs (g - s1) - xhat c2: 4, the dropout scale 1
              dgamma, dbeta 24   per term 3, 16 rows per wave in an fp32 chain, 4 waves, then fp64 column sums rounded once
ReLU: dy is set to zero where the float64 pre-activation lies within 1e-4 of 0 -- fp32 and float64 may take different sides of the kink
there and the derivative jumps; below 1 % of the elements (asserted).

Small cases are drawn well-conditioned (`_bn_inputs`, `_ln_inputs`): with two nearly equal samples in a channel, or two nearly equal
entries in a LayerNorm row of C = 2, the float32 specification itself misses the earlier tolerance (a first run showed bars of 1.1e-4
against 1.1e-4 allowed for the affine backward at C = 16, M = 2, and of up to 25 for LayerNorm mode 1 at C = 2).

Measured on the MI355X, one case per route (unit, bar, error as above; [stats / apply / backward route], v4 = the 16-byte kernels):
  BatchNorm, train, mish                                     y: unit      bar        error      dx: unit     bar        error      dgamma: unit bar        error
  C=37   M=16385 contiguous          [sc / sc / sc]          9.949e-07  1.315e-05  9.796e-07    1.113e-06  1.937e-05  1.457e-06    3.456e-05  6.108e-04  3.152e-05
  C=64   M=16385 contiguous          [v4 / v4 / v4]          1.340e-06  1.411e-05  9.797e-07    1.053e-06  1.703e-05  1.269e-06    4.966e-05  5.482e-04  3.515e-05
  C=48   M=65    contiguous          [sc / v4 / sc]          5.945e-07  9.414e-06  4.280e-07    4.757e-07  9.592e-06  4.686e-07    1.967e-06  3.971e-05  1.996e-06
  C=64   M=257   gamma.. at offset 1 [v4 / sc / sc]          8.614e-07  1.169e-05  8.541e-07    8.132e-07  1.329e-05  1.038e-06    8.870e-06  1.045e-04  3.520e-06
  C=2048 M=65    column slice, relu  [sc / v4 / sc]          8.480e-07  7.078e-06  6.091e-07    6.142e-07  8.867e-06  4.089e-07    5.637e-06  3.826e-05  1.366e-06
  C=1    M=257   eval, column offset 1 [sc / sc / sc]        6.284e-07  1.089e-05  6.284e-07    5.395e-07  9.705e-06  5.395e-07    3.135e-06  6.249e-05  5.043e-06
  statistics at C=64 M=16385 (256 groups of 65 rows): mean 5.195e-08 / 2.842e-07 / 1.462e-08, rstd 7.612e-08 / 4.657e-07 / 2.880e-08,
  running_var 1.523e-07 / 1.148e-06 / 5.846e-08
  three pieces, C=64 M=16385 mish [v4]: coef 5.897e-08 / 1.108e-06 / 5.897e-08, dx = a du + b x + c 5.274e-07 / 7.125e-06 / 4.301e-07;
  C=1028 M=65 [sc]: coef 8.106e-08 / 1.585e-06 / 5.804e-08, dx 4.064e-07 / 6.464e-06 / 4.064e-07
  LayerNorm                                                  y: unit      bar        error      dx: unit     bar        error      dgamma: unit bar        error
  C=128 M=4160  mode 1, residual       [c128, G 65, G2 2]    1.292e-06  2.758e-05  9.750e-07    7.796e-07  2.682e-05  6.614e-07    2.381e-05  6.376e-04  1.643e-05
  C=128 M=4160  mode 1, dropout 0.1    [generic, G2 2]       1.073e-06  2.722e-05  1.027e-06    8.091e-07  2.638e-05  6.576e-07    2.818e-05  6.571e-04  2.411e-05
  C=64  M=16385 mode 0, dropout 0.1    [generic, G 257, G2 5] 1.298e-06 3.301e-05  1.126e-06    7.388e-07  2.521e-05  6.209e-07    5.133e-05  1.604e-03  2.623e-05
  C=255 M=4160  mode 0, residual       [generic, G2 2]       1.138e-06  3.319e-05  1.119e-06    7.649e-07  2.686e-05  7.279e-07    3.274e-05  6.264e-04  2.255e-05
  C=2   M=65    mode 1, no residual    [generic]             2.526e-07  4.927e-06  1.690e-07    5.581e-07  2.232e-06  6.633e-07    6.122e-07  2.269e-05  4.401e-07
  dB with dropout at C=64 M=16385: 1.034e-06 / 2.885e-05 / 8.093e-07
What this file found: no wrong value -- all 193 tests pass on the kernels as they were; every scalar route, tail row, group edge and
second-level reduction agrees with float64 within its bar, and no canary changed.  The comment in bn_stats_stage1 that restricted C to
powers of two is corrected (C = 1, 3, 37, 48, 1028 and 2048 run it here).
"""
import pytest
import torch

from tests import norm_attn_ref as NR
from tests.step_tail_ref import f32

pytestmark = pytest.mark.gpu
EPS_BN, MOMENTUM = f32(1e-5), f32(0.1)                   # as the C floats the kernels receive
LN_EPS = {0: f32(1e-5), 1: f32(1e-6)}
P_DROP = 0.1
CS_MAXG, BA_R, V4_U, LN_BWD_ROWS = 256, 4, 12, 64


# ---- the host predicates of csrc/norm.hip, restated to label the cases ---------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def v4_clauses(aligned, ld, C):
    return {"C%4": C % 4 == 0, "C<=1024": C <= 1024, "ld%4": ld % 4 == 0, "base16": aligned,
            "rows": C % 4 == 0 and (256 % (C // 4) == 0 or (C // 4) % 256 == 0)}


def v4_ok(aligned, ld, C):
    return all(v4_clauses(aligned, ld, C).values())


def apply_clauses(aligned, ld, C, vec_aligned):
    """tatt_bn_apply's own predicate (X and Y have the same layout here)"""
    return {"C%4": C % 4 == 0, "ld%4": ld % 4 == 0, "maps16": aligned, "vectors16": vec_aligned}


def apply_v4(aligned, ld, C, vec_aligned):
    return all(apply_clauses(aligned, ld, C, vec_aligned).values())


def bwd_v4(aligned, ld, C, vec_aligned):
    """tatt_bn_bwd: all three maps v4_ok and the five vectors aligned"""
    return v4_ok(aligned, ld, C) and vec_aligned


def cs_groups(M):
    g = cdiv(M, 64)
    return CS_MAXG if g > CS_MAXG else max(g, 1)


def geometry(C, layout):
    extra, off = NR.LAYOUTS[layout]
    return off % 4 == 0, C + extra


# ---- BatchNorm cases -----------------------------------------------------------------------------------------------------------------
BN_C = (1, 3, 16, 37, 48, 64, 1024, 1028, 2048)
BN_M = (1, 2, 3, 4, 5, 63, 65, 257)
BN_CM = [(C, M) for C in BN_C for M in BN_M if C < 1024 or M <= 65] + [(C, M) for C in (37, 64) for M in (16384, 16385)]
BN_INNER = [(layout, odd) for layout in NR.LAYOUTS for odd in (False, True)]
WANT_ROUTE = {1: "scalar", 3: "scalar", 16: "vector", 37: "scalar", 48: "scalar stats, vector apply", 64: "vector",
              1024: "vector", 1028: "scalar stats, vector apply", 2048: "scalar stats, vector apply"}


def _route(C):
    """the route of the contiguous layout with aligned vectors"""
    stats, app = v4_ok(True, C, C), apply_v4(True, C, C, True)
    return {(True, True): "vector", (False, False): "scalar", (False, True): "scalar stats, vector apply"}[(stats, app)]


def _both_sides(rows, what):
    for name in rows[0]:
        seen = {r[name] for r in rows}
        assert seen == {True, False}, "%s: clause %s has only the side %s in the case list" % (what, name, seen)


def _check_bn_cases():
    assert {C: _route(C) for C in BN_C} == WANT_ROUTE
    assert (1024 // 4) % 256 == 0 and v4_ok(True, 1024, 1024) and 256 % (48 // 4) != 0
    geo = [(C, M) + geometry(C, layout) + (odd,) for C, M in BN_CM for layout, odd in BN_INNER]
    _both_sides([v4_clauses(al, ld, C) for C, M, al, ld, odd in geo], "v4_ok")
    _both_sides([apply_clauses(al, ld, C, not odd) for C, M, al, ld, odd in geo], "tatt_bn_apply")
    _both_sides([{"maps": v4_ok(al, ld, C), "vectors16": not odd} for C, M, al, ld, odd in geo], "tatt_bn_bwd")
    # every combination of the three routes that the code can produce, the odd-offset gamma that flips the apply route alone included
    combos = {(v4_ok(al, ld, C), apply_v4(al, ld, C, not odd), bwd_v4(al, ld, C, not odd)) for C, M, al, ld, odd in geo}
    assert combos == {(True, True, True), (True, False, False), (False, True, False), (False, False, False)}, combos
    Ms = {M for _, M in BN_CM}
    _both_sides([{"groups saturate": cdiv(M, 64) > CS_MAXG, "rpb 65": cdiv(M, cs_groups(M)) == 65} for M in Ms], "cs_groups")
    assert cs_groups(16384) == 256 and cdiv(16384, 256) == 64 and cs_groups(16385) == 256 and cs_groups(1) == 1
    # the row edges of the vector kernels: BA_R rows per thread (a full group, a clamped tail of every length) and V4_U loads in flight
    # (a block's rows per row lane below and above V4_U, with a remainder)
    assert {M % BA_R for M in Ms} == {0, 1, 2, 3}
    per_lane = {cdiv(cdiv(M, cs_groups(M)), 256 // (C // 4)) for C, M in BN_CM if v4_ok(True, C, C) and C <= 1024 and C // 4 <= 256}
    for U in (V4_U, V4_U // 2):                               # (v4_rows, and v4_rows2 over two maps)
        assert min(per_lane) < U < max(per_lane) and any(n % U for n in per_lane if n > U), per_lane
    assert all(M <= 65 for C, M in BN_CM if C >= 1024) and max(M * C for C, M in BN_CM) <= 16385 * 64


_check_bn_cases()


MAX_MEAN_OVER_STD = 8.0


def _bn_inputs(C, M):
    """x = 1.5 randn + 0.3.  A case of fewer than 1024 elements is redrawn until |batch mean| <= 8 batch std in every channel: two nearly
    equal samples make a channel's backward cancel (the affine form b x + c by |mean| rstd), the float32 specification itself then misses
    the earlier tolerance, and the largest error of so few elements says little about the error level.  Decided on the inputs alone."""
    for draw in range(1000):
        gen = torch.Generator().manual_seed(7000 + 31 * C + M + 100000 * draw)
        x = 1.5 * torch.randn(M, C, generator=gen) + 0.3
        gamma, beta = 1 + 0.3 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
        rm, rv = 0.4 * torch.randn(C, generator=gen), 0.5 + torch.rand(C, generator=gen)
        dy = torch.randn(M, C, generator=gen)
        if M == 1 or M * C >= 1024:
            break
        xd = x.double()
        if float((xd.mean(0).abs() / torch.sqrt(xd.var(0, unbiased=False) + EPS_BN)).max()) <= MAX_MEAN_OVER_STD:
            break
    else:
        raise AssertionError("no well-conditioned draw for C=%d M=%d" % (C, M))
    return x, gamma, beta, rm, rv, dy


def _bn_reference(x, gamma, beta, rm, rv, dy, training, act):
    """-> the specification in float64 and in float32, and the dy both ran on"""
    out = {}
    for dt in (torch.float64, torch.float32):
        c = lambda t: t.to(dt)
        y, mean, rstd, nrm, nrv = NR.bn_forward(c(x), c(gamma), c(beta), c(rm), c(rv), training, MOMENTUM, EPS_BN, act)
        if dt == torch.float64 and act == NR.ACT_RELU:
            u = (x.double() - mean) * rstd * gamma.double() + beta.double()
            near = u.abs() < 1e-4
            assert float(near.double().mean()) < 0.01
            dy = torch.where(near, torch.zeros_like(dy), dy)
        dx, dg, db = NR.bn_backward(c(x), c(dy), mean, rstd, c(gamma), c(beta), act, training)
        du, xh, s, q = NR.bn_partial_sums(c(x), c(dy), mean, rstd, c(gamma), c(beta), act)
        out[dt] = {"y": y, "mean": mean, "rstd": rstd, "running_mean": nrm, "running_var": nrv, "dx": dx, "dgamma": dg, "dbeta": db,
                   "coef": NR.bn_backward_finish(s, q, x.shape[0], mean, rstd, c(gamma))[2], "du": du}
    return out[torch.float64], out[torch.float32], dy


def _k(name, act, training):
    mish = act == NR.ACT_MISH
    return {"mean": 2, "rstd": 2 if training else 3, "running_mean": 3, "running_var": 3, "y": 12 if mish else 5,
            "dx": 23 if mish else 13, "dgamma": 16 if mish else 6, "dbeta": 16 if mish else 6, "coef": 7, "dx3": 9}[name]


@pytest.mark.parametrize("C,M", BN_CM)
def test_batchnorm_routes_against_float64(dev, C, M):
    from tatt_amd import ops
    x, gamma, beta, rm, rv, dy0 = _bn_inputs(C, M)
    failed = []
    for training in ((True, False) if M > 1 else (False,)):
        for act in (0, 1, 2):
            r64, r32, dy = _bn_reference(x, gamma, beta, rm, rv, dy0, training, act)
            for layout, odd in BN_INNER:
                aligned, ld = geometry(C, layout)
                case = "bn C=%d M=%d %s act%d %s %s [stats %s apply %s bwd %s]" % (
                    C, M, "train" if training else "eval", act, layout, "vec+1" if odd else "vec", "v4" if v4_ok(aligned, ld, C) else "sc",
                    "v4" if apply_v4(aligned, ld, C, not odd) else "sc", "v4" if bwd_v4(aligned, ld, C, not odd) else "sc")
                got, boxes = {}, []

                def box(t, vec=None):
                    b = NR.boxvec(t, vec, odd, dev) if vec is not None else NR.box2d(t, M, C, layout, dev)
                    boxes.append(b)
                    return b

                xb, gb, bb = box(x), box(gamma, vec=C), box(beta, vec=C)
                rmb, rvb = box(rm, vec=C), box(rv, vec=C)
                if training:
                    mean, rstd = ops.bn_stats(xb.v, EPS_BN, MOMENTUM, rmb.v, rvb.v)
                    got["running_mean"], got["running_var"] = rmb.v, rvb.v
                    mb, rb = box(mean.cpu(), vec=C), box(rstd.cpu(), vec=C)
                else:
                    mb, rb = rmb, box(ops.bn_rstd(rvb.v, EPS_BN).cpu(), vec=C)
                got["mean"], got["rstd"] = mb.v, rb.v
                yb = box(None)
                assert ops.bn_apply(xb.v, mb.v, rb.v, gb.v, bb.v, act, out=yb.v) is yb.v
                got["y"] = yb.v
                dyb, dxb = box(dy), box(None)
                dgb, dbb, sums = box(None, vec=C), box(None, vec=C), box(None, vec=2 * C)
                ws = torch.empty(CS_MAXG * 2 * C, device=dev, dtype=torch.float64)
                ops.call("tatt_bn_bwd", ops.P(xb.v), xb.v.stride(0), ops.P(dyb.v), dyb.v.stride(0), ops.P(dxb.v), dxb.v.stride(0), M, C,
                         ops.P(mb.v), ops.P(rb.v), ops.P(gb.v), ops.P(bb.v), act, int(training), ops.P(dgb.v), ops.P(dbb.v), ops.P(sums.v),
                         ops.P(ws), ops.stream())
                got["dx"], got["dgamma"], got["dbeta"] = dxb.v, dgb.v, dbb.v
                if layout == "contig" and not odd:             # the launcher the operators use allocates its own outputs: same bits
                    for a, b in zip(ops.bn_bwd(xb.v, dyb.v, mb.v, rb.v, gb.v, bb.v, act, training), (dxb.v, dgb.v, dbb.v)):
                        assert torch.equal(a, b)
                for name, t in got.items():
                    bad = NR.judge(case, name, t, r64[name], r32[name], _k(name, act, training), grad=name.startswith("d"))
                    if bad:
                        failed.append(bad)
                if not all(b.intact() for b in boxes):
                    failed.append((case, "a canary changed"))
    assert not failed, failed[:8]


# ---- the backward in three pieces ---------------------------------------------------------------------------------------------------
BN3_CM = [(C, M) for C, M in BN_CM if C % 4 == 0 and M > 1]


@pytest.mark.parametrize("C,M", BN3_CM)
def test_batchnorm_backward_in_three_pieces(dev, C, M):
    """tatt_bn_bwd_partials -> tatt_bn_bwd_finish -> tatt_bn_bwd_affine: dgamma, dbeta, coef and dx = a du + b x + c (train mode)"""
    from tatt_amd import ops
    x, gamma, beta, rm, rv, dy0 = _bn_inputs(C, M)
    failed = []
    for act in (0, 1, 2):
        r64, r32, dy = _bn_reference(x, gamma, beta, rm, rv, dy0, True, act)
        for layout, odd in BN_INNER:
            aligned, ld = geometry(C, layout)
            case = "bn3 C=%d M=%d act%d %s %s [partials %s]" % (C, M, act, layout, "vec+1" if odd else "vec",
                                                                "v4" if bwd_v4(aligned, ld, C, not odd) else "sc")
            xb, dyb = NR.box2d(x, M, C, layout, dev), NR.box2d(dy, M, C, layout, dev)
            vecs = [NR.boxvec(t, C, odd, dev) for t in (r32["mean"], r32["rstd"], gamma, beta)]
            mean, rstd, g, b = (v.v for v in vecs)
            part, G = ops.bn_bwd_partials(xb.v, dyb.v, mean, rstd, g, b, act)
            assert G == cs_groups(M) and part.numel() == G * 2 * C
            dg, db, coef = ops.bn_bwd_finish(part, G, C, M, mean, rstd, g)
            # the statistics handed over are the float32 specification's: the reference of this test takes the same ones
            w = {}
            for dt in (torch.float64, torch.float32):
                c = lambda t: t.to(dt)
                du, xh, s, q = NR.bn_partial_sums(c(x), c(dy), c(r32["mean"]), c(r32["rstd"]), c(gamma), c(beta), act)
                wg, wb, wc = NR.bn_backward_finish(s, q, M, c(r32["mean"]), c(r32["rstd"]), c(gamma))
                w[dt] = {"dgamma": wg, "dbeta": wb, "coef": wc, "du": du}
            w64, w32 = w[torch.float64], w[torch.float32]
            got = {"dgamma": dg, "dbeta": db, "coef": coef}
            if layout == "contig":
                du32 = w64["du"].float()                       # the gradient in front of the BatchNorm, as a producer would hand it over
                w64["dx3"] = NR.bn_backward_affine(x.double(), du32.double(), w64["coef"])
                w32["dx3"] = NR.bn_backward_affine(x, du32, w32["coef"])
                dub, dxb = NR.box2d(du32, M, C, "contig", dev), NR.box2d(None, M, C, "contig", dev)
                ops.call("tatt_bn_bwd_affine", ops.P(xb.v), ops.P(dub.v), ops.P(dxb.v), M, C, ops.P(coef), ops.stream())
                assert torch.equal(ops.bn_bwd_affine(xb.v, dub.v, coef), dxb.v)
                got["dx3"] = dxb.v
                if not dxb.intact():
                    failed.append((case, "a canary changed"))
            for name, t in got.items():
                bad = NR.judge(case, name, t, w64[name], w32[name], _k(name, act, True), grad=True)
                if bad:
                    failed.append(bad)
    assert not failed, failed[:8]


def test_batchnorm_affine_refuses_c37(dev):
    from tatt_amd import ops
    x = torch.randn(5, 37, device=dev)
    with pytest.raises(RuntimeError, match="tatt_bn_bwd_affine failed with code 1"):
        ops.bn_bwd_affine(x, x.clone(), torch.zeros(3, 37, device=dev))


@pytest.mark.parametrize("C,M", [(37, 65), (64, 257)])
def test_batchnorm_function_wiring(dev, C, M):
    """functional.BatchNormActFn: forward, running statistics and the three gradients through autograd, train and eval, mish"""
    from tatt_amd import functional as Fh
    x, gamma, beta, rm, rv, dy = _bn_inputs(C, M)
    failed = []
    for training in (True, False):
        r64, r32, _ = _bn_reference(x, gamma, beta, rm, rv, dy, training, NR.ACT_MISH)
        xd, g, b = (t.to(dev).requires_grad_() for t in (x, gamma, beta))
        rmd, rvd = rm.to(dev), rv.to(dev)
        y = Fh.BatchNormActFn.apply(xd.view(1, M, C), g, b, rmd, rvd, training, MOMENTUM, EPS_BN, NR.ACT_MISH)
        y.backward(dy.to(dev).view(1, M, C))
        got = {"y": y[0], "running_mean": rmd, "running_var": rvd, "dx": xd.grad, "dgamma": g.grad, "dbeta": b.grad}
        for name, t in got.items():
            bad = NR.judge("BatchNormActFn C=%d M=%d %s" % (C, M, "train" if training else "eval"), name, t, r64[name], r32[name],
                           _k(name, NR.ACT_MISH, training), grad=name.startswith("d"))
            if bad:
                failed.append(bad)
    assert not failed, failed


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------
LN_C = (2, 37, 63, 64, 65, 128, 255, 256)
LN_M = (1, 3, 4, 5, 63, 64, 65, 4096, 4160)
LN_CM = [(C, M) for C in LN_C for M in LN_M] + [(64, 16385)]
LN_DROP_C = (37, 64, 128)
K_LN = {"y": 30, "dx": 34, "dB": 34, "dgamma": 24, "dbeta": 24}


def _ln_kernel(C, p):
    return "c128" if C == 128 and p <= 0.0 else "generic"


def _check_ln_cases():
    runs = [(C, M, p) for C, M in LN_CM for p in ((0.0, P_DROP) if C in LN_DROP_C else (0.0,))]
    assert {_ln_kernel(C, p) for C, M, p in runs if C == 128} == {"c128", "generic"}
    _both_sides([{"C == 128": C == 128, "dropout": p > 0.0, "second-level groups > 1": cs_groups(cdiv(M, LN_BWD_ROWS)) > 1,
                  "ragged last block": M % LN_BWD_ROWS != 0, "lanes beyond C": C % 64 != 0} for C, M, p in runs], "tatt_ln_bwd")
    assert cdiv(4160, LN_BWD_ROWS) == 65 and cs_groups(65) == 2 and cs_groups(cdiv(4096, LN_BWD_ROWS)) == 1
    assert cs_groups(cdiv(16385, LN_BWD_ROWS)) == 5 and {cdiv(C, 64) for C in LN_C} == {1, 2, 4}


_check_ln_cases()


def _ln_inputs(C, M):
    """C = 2: the two entries of a row lie at least 1 apart and the residual is small -- LayerNorm of two nearly equal values is
    ill-conditioned (dx grows as 1 / |x0 - x1|), and the float32 specification itself then misses the earlier tolerance"""
    gen = torch.Generator().manual_seed(9000 + 17 * C + M)
    a, b = torch.randn(M, C, generator=gen), torch.randn(M, C, generator=gen)
    if C == 2:
        sign = torch.where(torch.rand(M, generator=gen) < 0.5, -1.0, 1.0)
        a[:, 1] = a[:, 0] + sign * (1.0 + torch.rand(M, generator=gen))
        b *= 0.1
    gamma, beta = 1 + 0.3 * torch.randn(C, generator=gen), 0.2 * torch.randn(C, generator=gen)
    dy = torch.randn(M, C, generator=gen)
    return a, b, gamma, beta, dy


def _ln_reference(a, b, gamma, beta, dy, mode, mask):
    out = {}
    if a.shape[1] == 2:
        x = a if b is None else a + (b if mask is None else b * mask)
        assert float((x[:, 0] - x[:, 1]).abs().min()) >= 0.25
    for dt in (torch.float64, torch.float32):
        c = lambda t: None if t is None else t.to(dt)
        y = NR.layer_norm(c(a), c(b), c(gamma), c(beta), LN_EPS[mode], mode, c(mask))
        dx, db, dg, dbeta = NR.layer_norm_backward(c(a), c(b), c(dy), c(gamma), LN_EPS[mode], mode, c(mask))
        out[dt] = {"y": y, "dx": dx, "dB": db, "dgamma": dg, "dbeta": dbeta}
    return out[torch.float64], out[torch.float32]


def _seed(dev, value=0x1234ABCD5678EF01 & 0x7FFFFFFFFFFFFFFF):
    return torch.tensor([value], dtype=torch.int64, device=dev)


def _ln_direct(ops, dev, a, b, dy, gamma, beta, mode, p, seed, site):
    """tatt_ln_fwd / tatt_ln_bwd through the C ABI into canaried buffers, dgamma and dbeta allocated apart (the non-adjacent branch)"""
    M, C = a.shape
    flat = lambda n: NR.box2d(None, 1, n, "contig", dev)
    yb, sb, dxb, dBb, dgb, dbb = flat(M * C), flat(2 * M), flat(M * C), flat(M * C), flat(C), flat(C)
    assert dbb.v.data_ptr() != dgb.v.data_ptr() + 4 * C
    ops.call("tatt_ln_fwd", ops.P(a), ops.P(b), ops.P(yb.v), ops.P(sb.v), M, C, ops.P(gamma), ops.P(beta), LN_EPS[mode], mode, float(p),
             ops.P(seed), site, ops.stream())
    part = torch.empty(cdiv(M, LN_BWD_ROWS) * 2 * C, device=dev)
    # (the workspace holds NaNs: a second-level reduction that reads more groups than the first level wrote shows)
    ws = torch.full((CS_MAXG * 2 * C,), float("nan"), device=dev, dtype=torch.float64)
    ops.call("tatt_ln_bwd", ops.P(a), ops.P(b), ops.P(dy), ops.P(sb.v), ops.P(dxb.v), ops.P(dBb.v) if p > 0 else None, M, C, ops.P(gamma),
             ops.P(dgb.v), ops.P(dbb.v), ops.P(part), ops.P(ws), LN_EPS[mode], mode, float(p), ops.P(seed), site, ops.stream())
    boxes = [yb, sb, dxb, dBb, dgb, dbb]
    return [t.v.reshape(-1) for t in boxes], all(t.intact() for t in boxes)


@pytest.mark.parametrize("C,M", LN_CM)
def test_layernorm_routes_against_float64(dev, C, M):
    from tatt_amd import ops
    a, b, gamma, beta, dy = _ln_inputs(C, M)
    ad, bd, gd, betad, dyd = (t.to(dev) for t in (a, b, gamma, beta, dy))
    seed, site = _seed(dev), 5
    mask = NR.recover_mask((M, C), P_DROP, seed, site, dev) if C in LN_DROP_C else None
    if mask is not None and M * C >= 64:
        assert bool((mask == 0).any())
    failed = []
    for mode in (0, 1):
        for residual in ("none", "plain") + (("dropped",) if mask is not None else ()):
            p = P_DROP if residual == "dropped" else 0.0
            case = "ln C=%d M=%d mode%d %s [%s, G %d, G2 %d]" % (C, M, mode, residual, _ln_kernel(C, p), cdiv(M, LN_BWD_ROWS),
                                                               cs_groups(cdiv(M, LN_BWD_ROWS)))
            bb = bd if residual != "none" else None
            r64, r32 = _ln_reference(a, b if residual != "none" else None, gamma, beta, dy, mode, mask if residual == "dropped" else None)
            y, stats = ops.ln_fwd(ad, bb, gd, betad, LN_EPS[mode], mode, p, seed, site)
            dx, dB, dg, dbeta = ops.ln_bwd(ad, bb, dyd, stats, gd, LN_EPS[mode], mode, p, seed, site)
            assert dbeta.data_ptr() == dg.data_ptr() + 4 * C                       # the adjacent branch
            assert (dB is None) == (residual == "none") and (dB is dx) == (residual == "plain")
            got = {"y": y, "dx": dx, "dgamma": dg, "dbeta": dbeta}
            if residual != "none":
                got["dB"] = dB
            for name, t in got.items():
                bad = NR.judge(case, name, t, r64[name], r32[name], K_LN[name], grad=name.startswith("d"))
                if bad:
                    failed.append(bad)
            if residual == "dropped":                                             # dB = Dropout'(dx) with the forward's mask, exactly
                assert torch.equal(dB == 0, (mask.to(dev) == 0) | (dx == 0))
            # the same through the C ABI with dgamma and dbeta allocated apart: bit for bit, and no canary touched
            (y2, s2, dx2, dB2, dg2, db2), intact = _ln_direct(ops, dev, ad, bb, dyd, gd, betad, mode, p, seed, site)
            same = [torch.equal(y2, y.reshape(-1)), torch.equal(s2, stats.reshape(-1)), torch.equal(dx2, dx.reshape(-1)),
                    torch.equal(dg2, dg), torch.equal(db2, dbeta), p <= 0 or torch.equal(dB2, dB.reshape(-1))]
            if not all(same):
                failed.append((case, "the non-adjacent dgamma / dbeta call differs", same))
            if not intact:
                failed.append((case, "a canary changed"))
    assert not failed, failed[:8]


def test_layernorm_refusals(dev):
    from tatt_amd import ops
    a = torch.randn(3, 257, device=dev)
    g = torch.ones(257, device=dev)
    with pytest.raises(RuntimeError, match="tatt_ln_fwd failed with code 1"):
        ops.ln_fwd(a, None, g, g)
    with pytest.raises(RuntimeError, match="tatt_ln_bwd failed with code 1"):
        ops.ln_bwd(a, None, a, torch.zeros(3, 2, device=dev), g)
    a, g = torch.randn(3, 64, device=dev), torch.ones(64, device=dev)
    with pytest.raises(RuntimeError, match="tatt_ln_fwd failed with code 2"):
        ops.ln_fwd(a, None, g, g, pdrop=P_DROP, seed=_seed(dev), site=1)
    with pytest.raises(RuntimeError, match="tatt_ln_bwd failed with code 2"):
        ops.call("tatt_ln_bwd", ops.P(a), None, ops.P(a), ops.P(a), ops.P(a), ops.P(a), 3, 64, ops.P(g), ops.P(g), ops.P(g), ops.P(a),
                 None, 1e-5, 0, P_DROP, ops.P(_seed(dev)), 1, ops.stream())


@pytest.mark.parametrize("C,M,mode", [(64, 65, 0), (128, 130, 1)])
def test_layernorm_function_wiring(dev, C, M, mode):
    """functional.LayerNormFn with dropout on the residual: the mask of the seed word the function reads, recovered"""
    from tatt_amd import functional as Fh
    a, b, gamma, beta, dy = _ln_inputs(C, M)
    Fh.set_seed(dev, 77)
    site = 3
    mask = NR.recover_mask((M, C), P_DROP, Fh.current_seed(dev), site, dev)
    r64, r32 = _ln_reference(a, b, gamma, beta, dy, mode, mask)
    ad, bd, gd, betad = (t.to(dev).requires_grad_() for t in (a, b, gamma, beta))
    y = Fh.LayerNormFn.apply(ad.view(1, M, C), bd.view(1, M, C), gd, betad, LN_EPS[mode], mode, P_DROP, site)
    y.backward(dy.to(dev).view(1, M, C))
    got = {"y": y[0], "dx": ad.grad, "dB": bd.grad, "dgamma": gd.grad, "dbeta": betad.grad}
    failed = [bad for bad in (NR.judge("LayerNormFn C=%d M=%d mode%d" % (C, M, mode), name, t, r64[name], r32[name], K_LN[name],
                                       grad=name.startswith("d")) for name, t in got.items()) if bad]
    assert not failed, failed
