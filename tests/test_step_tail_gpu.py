"""The small launches that end every training step, each against a plain float64 reference of the same operation: the global norm
(tatt_l2norm), clip + Adam (tatt_adam_step), the optimiser chain as the Trainer issues and captures it, the gradient gather
(tatt_gather_grads), the counters and clears (tatt_inc_i64, tatt_zero_f32), tatt_colsum, tatt_copy4d, the split-K reduction
(tatt_splitk_reduce) and its deferred, batched form (tatt_reduce_defer / tatt_reduce_flush).  They are called the way the product
calls them (tatt_amd.train.HipStepKernels, tatt_amd.ops).  References, case lists and bound checks: tests/step_tail_ref.py; that
they can fail: tests/test_step_tail_ref.py."""
import numpy as np
import pytest
import torch

from tests import step_tail_ref as R

pytestmark = pytest.mark.gpu
STD = dict(scale_factor=2, width=128, height=32, STN=True, mask=True, srb_nums=5, hidden_units=32)


def _kernels():
    from tatt_amd.train import HipStepKernels
    return HipStepKernels()


def _randn(n, seed, scale=1.0):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)) * scale


# ---- tatt_l2norm --------------------------------------------------------------------------------------------------------------------
def _l2(dev, g_dev):
    out = torch.full((1,), -1.0, device=dev)
    _kernels().l2norm(g_dev, out, torch.empty(1024, dtype=torch.float64, device=dev))
    return out.cpu()[0]


@pytest.mark.parametrize("n", R.L2_SIZES + ("flat",))
def test_l2norm_within_one_ulp_of_float64(dev, n):
    """One block per 256 elements up to 1024 blocks (262,144 elements), a grid-stride loop above; double accumulation, one rounding.
    1e20 and 1e-30 per element: the squares leave the fp32 range, the answer does not."""
    if n == "flat":
        import tatt_amd
        from tatt_amd.train import Trainer
        torch.manual_seed(1234)
        n = Trainer(tatt_amd.TSRN_TL_TRANS(**STD).to(dev)).n
    for scale in (1.0, 1e20, 1e-30):
        g = _randn(n, n % 1000 + 1, scale)
        got = _l2(dev, g.to(dev))
        ok, ref = R.l2_within_one_ulp(got, g)
        assert ok, (n, scale, float(got), ref)
    assert float(_l2(dev, torch.zeros(n, device=dev))) == 0.0


def test_l2norm_of_a_slice_leaves_its_surroundings(dev):
    g = _randn(5000, 3)
    buf0 = torch.cat([R.canary(5), g, R.canary(7)])
    outbuf0 = R.canary(8).clone()
    buf, outbuf = buf0.to(dev), outbuf0.to(dev)
    _kernels().l2norm(buf[5:5005], outbuf[3:4], torch.empty(1024, dtype=torch.float64, device=dev))
    assert R.same_bits(buf, buf0)
    got = outbuf.cpu()
    assert R.same_bits(got[:3], outbuf0[:3]) and R.same_bits(got[4:], outbuf0[4:])
    assert R.l2_within_one_ulp(got[3], g)[0]


# ---- tatt_adam_step -----------------------------------------------------------------------------------------------------------------
def _hip_adam(P, G, M, V, off, n, lr, b1, b2, eps, gnorm, max_norm, gscale, step):
    _kernels().adam(P[off:off + n], G[off:off + n], M[off:off + n], V[off:off + n], lr, b1, b2, eps, gnorm, max_norm, gscale, step)


@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_step_vs_float64(dev, n):
    """Every case of step_tail_ref.adam_cases(n): steps 1, 2, 7, 1000 and 2**32 + 3, a norm on both sides of max_norm, max_norm 0, a
    zero gradient with a zero norm, a (max_norm, gnorm) pair of order 1e-6, gscale 1 and 1/8, non-zero m and v unrelated to g, segment
    offsets 0, 4 and 16 inside larger buffers whose other elements are compared bitwise.  m, v and p element-wise, u = 2^-24:

        |m - m64| <= Km u (b1 |m0| + (1 - b1) |g coef64|)
        |v - v64| <= Kv u v64
        |p - p64| <= u |p64| + Kp u a1 (b1 |m0| + (1 - b1) |g coef64|) / den64

    Worst ratio to each shape with K = 1       m        v        p
      fp32 emulation of adam_kernel, CPU     2.178    4.066    4.629
      tatt_adam_step, MI355X                 2.178    3.991    3.889
    K = 4 x the emulation's ratio rounded up to a power of two: Km 16, Kv 32, Kp 32 (tests/step_tail_ref.py::ADAM_K)."""
    worst = dict(m=0.0, v=0.0, p=0.0)
    for case in R.adam_cases(n):
        r = R.run_adam_case(_hip_adam, case, dev=dev)
        worst = {k: max(worst[k], r[k]) for k in worst}
    print("tatt_adam_step n=%d worst ratios: m %.3f v %.3f p %.3f" % (n, worst["m"], worst["v"], worst["p"]))


def test_adam_step_refuses_a_misaligned_segment(dev):
    case = dict(R.adam_cases(1025)[0], off=1)
    bufs0 = R.adam_buffers(case)
    bufs = [b.to(dev) for b in bufs0]
    gnorm, step = torch.ones(1, device=dev), torch.ones(1, dtype=torch.int64, device=dev)
    with pytest.raises(RuntimeError, match="1001"):
        _hip_adam(bufs[0], bufs[1], bufs[2], bufs[3], 1, 1025, R.LR, R.B1, R.B2, R.EPS, gnorm, R.CLIP, 1.0, step)
    torch.cuda.synchronize()
    for b0, b in zip(bufs0, bufs):
        assert R.same_bits(b0, b)


# ---- the optimiser chain, captured and replayed -------------------------------------------------------------------------------------
def test_optimiser_chain_replays_from_device_scalars(dev):
    """guard, inc, l2norm, adam as Trainer._optim issues them, captured once on one stream and replayed four times over a new
    gradient each: the step count and the norm are read from device memory at replay, or steps 2..4 would repeat step 1's
    bias corrections and clip coefficient.  Gradient norms 0.1, 3, 0.2 and 10 around max_norm = 0.25.  Each replay is compared
    with one float64 step from the state before it (bounds of test_adam_step_vs_float64), the norm with its own reference."""
    from tatt_amd import functional as Fh
    Fh.sticky_word(dev)
    K = _kernels()
    n, off = 4099, 16
    case = dict(n=n, off=off, seed=77, zero_grad=False)
    bufs0 = R.adam_buffers(case)
    P, G, M, V = (b.to(dev) for b in bufs0)
    p, g, m, v = (X[off:off + n] for X in (P, G, M, V))
    step_count = torch.zeros(1, dtype=torch.int64, device=dev)
    gnorm = torch.zeros(1, device=dev)
    ws = torch.empty(1024, dtype=torch.float64, device=dev)
    grads = [_randn(n, 10 + k) * (t / n ** 0.5) for k, t in enumerate((0.1, 3.0, 0.2, 10.0))]

    def chain():
        K.guard()
        K.inc(step_count)
        K.l2norm(g, gnorm, ws)
        K.adam(p, g, m, v, R.LR, R.B1, R.B2, R.EPS, gnorm, R.CLIP, 1.0, step_count)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        chain()                                        # (warm-up outside the capture; its effects are undone below)
    torch.cuda.current_stream(dev).wait_stream(side)
    for X, X0 in zip((P, G, M, V), bufs0):
        X.copy_(X0)
    step_count.zero_()
    gnorm.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        chain()
    torch.cuda.synchronize()
    assert int(step_count) == 0 and R.same_bits(P, bufs0[0])          # capturing runs nothing
    state = [bufs0[0][off:off + n].clone(), bufs0[2][off:off + n].clone(), bufs0[3][off:off + n].clone()]
    coefs = []
    for k in range(4):
        g.copy_(grads[k].to(dev))
        graph.replay()
        torch.cuda.synchronize()
        assert int(step_count) == k + 1
        ok, ref = R.l2_within_one_ulp(gnorm.cpu()[0], grads[k])
        assert ok, (k, float(gnorm), ref)
        coefs.append(min(1.0, R.CLIP / (ref + 1e-6)))
        ref64 = R.adam64(state[0], grads[k], state[1], state[2], R.LR, R.B1, R.B2, R.EPS, float(gnorm), R.CLIP, 1.0, k + 1)
        got = (p.cpu(), m.cpu(), v.cpu())
        r = R.adam_ratios(got, ref64)
        print("replay %d: norm %.4f ratios m %.3f v %.3f p %.3f" % (k + 1, float(gnorm), r["m"], r["v"], r["p"]))
        for key in "mvp":
            assert r[key] <= R.ADAM_K[key], (k, key, r[key])
        state = [t.clone() for t in got]
    assert coefs[0] == 1.0 and coefs[2] == 1.0 and coefs[1] < 0.1 and coefs[3] < 0.03      # the replays did differ in their clip
    for X, X0 in zip((P, G, M, V), bufs0):
        got = X.cpu()
        assert R.same_bits(got[:off], X0[:off]) and R.same_bits(got[off + n:], X0[off + n:])


# ---- tatt_gather_grads --------------------------------------------------------------------------------------------------------------
def _to_dev_keeping_offset(src, dev):
    if src is None:
        return None
    if src.storage_offset() == 1:
        d = torch.empty(src.numel() + 1, device=dev)
        d[1:].copy_(src)
        return d[1:]
    return src.to(dev)


@pytest.mark.parametrize("count,zero_edges", R.gather_cases())
def test_gather_grads_bitwise(dev, count, zero_edges):
    """Tables of 112 entries (count 1, 111, 112, 113, 225), entry sizes from 0 to 4097 with zero-length entries first, last and
    adjacent, missing sources that must write zeros over the stale (here: NaN-pattern) content, sources at element offset 1 (the
    scalar path), destination offsets that are not multiples of 4; every element between and around the entries stays as it was."""
    from tatt_amd import ops
    entries, dst0 = R.gather_case(count, zero_edges)
    assert all(0 <= o and o + n <= dst0.numel() for _, o, n in entries)
    dst = dst0.to(dev)
    ops.gather_grads(dst, [(_to_dev_keeping_offset(s, dev), o, n) for s, o, n in entries])
    exp = R.gather_expected(dst0, entries)
    got = dst.cpu()
    if not R.same_bits(got, exp):
        bad = (R.bits(got) != R.bits(exp)).nonzero().reshape(-1)
        raise AssertionError("%d elements differ, first at %d" % (bad.numel(), int(bad[0])))


# ---- tatt_inc_i64, tatt_zero_f32 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_inc_i64_and_zero_f32(dev, n):
    from tatt_amd import ops
    pat = 0x5555AAAA5555AAAA
    buf0 = torch.full((3 + n + 5,), pat, dtype=torch.int64)
    vals = torch.randint(-2 ** 40, 2 ** 40, (n,), generator=torch.Generator().manual_seed(n))
    vals[0] = 2 ** 32 - 1                               # must carry into the upper word
    vals[-1] = 2 ** 32 - 1 if n > 1 else vals[-1]
    buf0[3:3 + n] = vals
    buf = buf0.to(dev)
    ops.inc_i64(buf[3:3 + n])
    exp = buf0.clone()
    exp[3:3 + n] += 1
    assert torch.equal(buf.cpu(), exp)
    assert int(buf[3]) == 2 ** 32
    f0 = R.canary(3 + n + 5).clone()
    f0[3:3 + n] = _randn(n, n) + 2.0
    f = f0.to(dev)
    ops.zero_f32(f[3:3 + n])
    expf = f0.clone()
    expf[3:3 + n] = 0.0
    assert R.same_bits(f, expf)


# ---- tatt_colsum --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 255, 256, 257, 49152])
@pytest.mark.parametrize("C", [1, 37, 64, 192, 513])
def test_colsum_vs_float64(dev, M, C):
    """out[c] = scale * sum_m x[m, c] + beta * out[c] over a contiguous map, over a 16-byte aligned column slice of a wider map
    (ld != C: the vector kernel where C allows it) and over a slice at column offset 1 (never the vector kernel).  The sum is
    formed in double; rounding it (times scale) to fp32 and accumulating beta * out in fp32 cost at most one unit in the last place
    of the larger of |scale * sum| and |result|: asserted within 2."""
    from tatt_amd import ops
    gen = torch.Generator().manual_seed(M * 1000 + C)
    layouts = []
    layouts.append(torch.randn(M, C, generator=gen))
    layouts.append(torch.randn(M, C + 8, generator=gen)[:, 4:4 + C])
    layouts.append(torch.randn(M, C + 3, generator=gen)[:, 1:1 + C])
    for li, x in enumerate(layouts):
        base = x._base if x._base is not None else x
        xd = base.to(dev)
        if x._base is not None:
            xd = xd[:, x.storage_offset():x.storage_offset() + C]
        assert xd.stride() == x.stride()
        s64 = x.double().sum(0)
        for scale, beta in ((1.0, 0.0), (0.37, 1.0), (-2.5, 0.0)):
            out0 = torch.cat([R.canary(4), torch.randn(C, generator=gen), R.canary(4)])
            outd = out0.to(dev)
            ops.colsum(xd, out=outd[4:4 + C], scale=scale, beta=beta)
            got = outd.cpu()
            assert R.same_bits(got[:4], out0[:4]) and R.same_bits(got[4 + C:], out0[4 + C:])
            scaled = R.f32(scale) * s64
            ref = scaled + R.f32(beta) * out0[4:4 + C].double() if beta != 0.0 else scaled
            mag = torch.maximum(scaled.abs(), ref.abs())
            ulp = torch.from_numpy(np.spacing(mag.numpy().astype(np.float32)).astype(np.float64))
            err = (got[4:4 + C].double() - ref).abs()
            assert bool((err <= 2.0 * ulp).all()), (M, C, li, scale, beta, float((err / ulp).max()))


# ---- tatt_copy4d --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ext", [(1, 1, 1, 1), (3, 5, 7, 11)])
@pytest.mark.parametrize("beta", [0.0, 0.5])
def test_copy4d_layouts_bitwise(dev, ext, beta):
    """NCHW -> NHWC and back, and a permuted parameter gather whose source has a zero stride (a broadcast axis).  beta = 0.5:
    0.5 * dst is exact, so v + 0.5 * dst has one rounding, fused or not -- bitwise against the same expression in fp32 torch."""
    from tatt_amd import ops
    n, c, h, w = ext
    gen = torch.Generator().manual_seed(sum(ext))
    total = n * c * h * w

    def run(src, sizes, sstr, dstr, expect_view):
        dst0 = torch.cat([torch.randn(total, generator=gen), R.canary(6)])
        dst = dst0.to(dev)
        ops.copy4d(src.to(dev), dst, sizes, sstr, dstr, beta=beta)
        exp = dst0.clone()
        v = expect_view.contiguous().reshape(-1)
        exp[:total] = v + beta * dst0[:total] if beta != 0.0 else v
        assert R.same_bits(dst, exp)

    nchw = torch.randn(n, c, h, w, generator=gen)
    run(nchw, (n, h, w, c), (c * h * w, w, 1, h * w), (h * w * c, w * c, c, 1), nchw.permute(0, 2, 3, 1))
    nhwc = torch.randn(n, h, w, c, generator=gen)
    run(nhwc, (n, c, h, w), (h * w * c, 1, w * c, c), (c * h * w, h * w, w, 1), nhwc.permute(0, 3, 1, 2))
    # dst[i0, i1, i2, i3] = par[i3, i1]: axes 0 and 2 broadcast (stride 0), the other two permuted
    par = torch.randn(w, c, generator=gen)
    run(par, (n, c, h, w), (0, 1, 0, c), (c * h * w, h * w, w, 1), par.t()[None, :, None, :].expand(n, c, h, w))


# ---- tatt_splitk_reduce, direct -----------------------------------------------------------------------------------------------------
def _hip_reduce(case, partial, C, vec):
    from tatt_amd import ops
    S, M, N, cin, taps, vec_len, remap, beta = case
    ops.call("tatt_splitk_reduce", ops.P(partial), ops.P(C), M, N, S, cin if remap else 0, taps if remap else 0, beta, ops.P(vec),
             vec_len, ops.stream())


@pytest.mark.parametrize("S", R.RED_S)
def test_splitk_reduce_vs_float64(dev, S):
    """S slabs the test writes itself: the loop unrolled by 16 (from S = 13), its stride-4 tail, M * N on both sides of a block of
    64, the trailing row-sum blocks behind the 64-aligned total with vec_len == M and vec_len != M (the conv bias gradient), the OIHW
    scatter, beta 0 and 1, and vec overwritten whatever beta is.  |err| <= S u sum_s |partial_s| per element (S + 1 terms with
    beta)."""
    worst = 0.0
    for case in R.reduce_cases():
        if case[0] == S:
            worst = max(worst, R.run_reduce_case(_hip_reduce, case, dev=dev))
    print("tatt_splitk_reduce S=%d worst ratio to the bound %.3f" % (S, worst))


# ---- deferred reductions ------------------------------------------------------------------------------------------------------------
PAT = 0x7FC0BEEF


def _pattern(n, dev):
    return torch.full((n,), PAT, dtype=torch.int32, device=dev).view(torch.float32)


def _untouched(t):
    return bool((t.reshape(-1).view(torch.int32) == PAT).all())


class _Item:
    """One reduction of a mixed list: kind 0 plain, 1 with vec (vec_len != M), 2 OIHW scatter, 3 tatt_gemm split-K with Z = 2,
    4 tatt_gemm split-K with the row sums riding along.  issue(outs) launches it into the given output tensors."""

    def __init__(self, k, dev):
        self.kind = k % 5
        gen = torch.Generator().manual_seed(500 + k)
        r = lambda *s: torch.randn(*s, generator=gen).to(dev)
        if self.kind == 0:
            self.case, self.sizes = (5 + k % 3, 37, 5, 37, 1, 0, False, 0.0), (37 * 5,)
        elif self.kind == 1:
            self.case, self.sizes = (13 + k % 4, 18, 4, 2, 9, 4, False, 0.0), (18 * 4, 4)
        elif self.kind == 2:
            self.case, self.sizes = (4 + k % 2, 63, 1, 7, 9, 0, True, 0.0), (63,)
        elif self.kind == 3:
            self.A, self.B, self.sizes = r(2, 40, 64), r(2, 64, 24), (2 * 40 * 24,)
        else:
            self.A, self.B, self.sizes = r(48, 80), r(80, 20), (48 * 20, 48)
        if self.kind < 3:
            S, M, N, _, _, vl = self.case[:6]
            self.partial = r(S * M * N + S * vl)

    def outputs(self, dev):
        return [_pattern(n, dev) for n in self.sizes]

    def issue(self, outs):
        from tatt_amd import ops
        if self.kind < 3:
            _hip_reduce(self.case, self.partial, outs[0], outs[1] if len(outs) > 1 else None)
        elif self.kind == 3:
            ops.gemm(self.A, 64, 1, self.B, 24, 1, outs[0], 24, 1, 40, 24, 64, Z=2, bsA=40 * 64, bsB=64 * 24, bsC=40 * 24, splitk=3)
        else:
            ops.gemm(self.A, 80, 1, self.B, 20, 1, outs[0], 20, 1, 48, 20, 80, alpha=0.5, splitk=2, rowsum=outs[1])


@pytest.mark.parametrize("K", [1, 35, 36, 37, 72, 73])
def test_deferred_reductions_equal_immediate_ones_bitwise(dev, K):
    """K registrations of mixed shapes around the 36-entry table: nothing is written before the flush except by the automatic
    flush of a full table; afterwards every output equals, bit for bit, the same reduction issued un-deferred (both run
    splitk_reduce_body)."""
    from tatt_amd import ops
    items = [_Item(k, dev) for k in range(K)]
    ref = []
    for it in items:
        o = it.outputs(dev)
        it.issue(o)
        ref.append(o)
    torch.cuda.synchronize()
    assert not any(_untouched(t) for o in ref for t in o)
    outs = [it.outputs(dev) for it in items]
    ops.reduce_defer(True)
    try:
        for it, o in zip(items, outs):
            it.issue(o)
        torch.cuda.synchronize()
        flushed = K // 36 * 36
        for k, (o, r) in enumerate(zip(outs, ref)):
            for t, rt in zip(o, r):
                if k < flushed:
                    assert R.same_bits(t, rt), ("entry %d of a full table" % k)
                else:
                    assert _untouched(t), ("entry %d was written before the flush" % k)
        ops.reduce_flush()
        torch.cuda.synchronize()
        for k, (o, r) in enumerate(zip(outs, ref)):
            for t, rt in zip(o, r):
                assert R.same_bits(t, rt), k
    finally:
        ops.reduce_defer(False)


def test_deferral_order_streams_and_switching_off(dev):
    """An accumulating reduction sees the pending ones to the same C; another stream is not held back; after reduce_defer(False)
    a reduction runs at once."""
    from tatt_amd import ops
    a, b = _Item(0, dev), _Item(5, dev)
    acc = (a.case[:7] + (1.0,))
    ref = a.outputs(dev)
    a.issue(ref)
    _hip_reduce(acc, b.partial[:a.partial.numel()], ref[0], None)
    other_ref = b.outputs(dev)
    b.issue(other_ref)
    torch.cuda.synchronize()
    out, other, late = a.outputs(dev), b.outputs(dev), b.outputs(dev)
    s2 = torch.cuda.Stream(device=dev)
    ops.reduce_defer(True)
    try:
        a.issue(out)
        torch.cuda.synchronize()
        assert _untouched(out[0])
        with torch.cuda.stream(s2):
            b.issue(other)
        s2.synchronize()
        assert R.same_bits(other[0], other_ref[0]) and _untouched(out[0])
        _hip_reduce(acc, b.partial[:a.partial.numel()], out[0], None)        # beta = 1: flushes the pending one first, then runs
        torch.cuda.synchronize()
        assert R.same_bits(out[0], ref[0])
    finally:
        ops.reduce_defer(False)
    b.issue(late)
    torch.cuda.synchronize()
    assert R.same_bits(late[0], other_ref[0])


WG = dict(n=40, M=512, N=48, K=40)


def _wgrad_inputs(dev, seed):
    gen = torch.Generator().manual_seed(seed)
    return [(torch.randn(WG["M"], WG["N"], generator=gen).to(dev), torch.randn(WG["M"], WG["K"], generator=gen).to(dev))
            for _ in range(WG["n"])]


def _wgrad_outputs(dev):
    return [(_pattern(WG["N"] * WG["K"], dev).view(WG["N"], WG["K"]), _pattern(WG["N"], dev)) for _ in range(WG["n"])]


def test_deferred_workspaces_survive_until_the_flush(dev):
    """40 linear_bwd_weight calls (split-K 4, bias row sums) under deferral with every reference to their temporaries dropped and
    garbage of the workspaces' size allocated and written in between: a workspace freed early would be handed out again and
    overwritten before the flush reads it."""
    from tatt_amd import ops
    assert ops._auto_split(WG["N"], WG["K"], WG["M"]) == 4
    ws_numel = 4 * WG["N"] * WG["K"] + 4 * WG["N"]
    ins = _wgrad_inputs(dev, 1)
    ref = _wgrad_outputs(dev)
    for (dy, x), (dW, db) in zip(ins, ref):
        ops.linear_bwd_weight(dy, x, out=dW, rowsum=db)
    torch.cuda.synchronize()
    outs = _wgrad_outputs(dev)
    ops.reduce_defer(True)
    try:
        for k in range(WG["n"]):
            dy, x = ins[k]
            ops.linear_bwd_weight(dy.clone(), x.clone(), out=outs[k][0], rowsum=outs[k][1])
            for _ in range(3):
                junk = torch.full((ws_numel,), 1e30, device=dev)
                del junk
        ops.reduce_flush()
        torch.cuda.synchronize()
    finally:
        ops.reduce_defer(False)
    for k in range(WG["n"]):
        assert R.same_bits(outs[k][0], ref[k][0]) and R.same_bits(outs[k][1], ref[k][1]), k
    assert rel_to_float64(ref[0][0], ins[0]) < 1e-5


def rel_to_float64(dW, pair):
    dy, x = pair
    want = dy.double().cpu().t() @ x.double().cpu()
    return float((dW.double().cpu() - want).norm() / want.norm())


def test_deferred_reductions_in_a_captured_graph(dev):
    """The same 40 calls, deferred and flushed inside one captured graph (one stream), replayed twice on changed inputs."""
    from tatt_amd import ops
    ins = _wgrad_inputs(dev, 2)
    outs = _wgrad_outputs(dev)

    def body():
        ops.reduce_defer(True)
        try:
            for (dy, x), (dW, db) in zip(ins, outs):
                ops.linear_bwd_weight(dy, x, out=dW, rowsum=db)
            ops.reduce_flush()
        finally:
            ops.reduce_defer(False)

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        body()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        body()
    for seed in (3, 4):
        for (dy, x), (ndy, nx) in zip(ins, _wgrad_inputs(dev, seed)):
            dy.copy_(ndy)
            x.copy_(nx)
        for dW, db in outs:
            dW.view(torch.int32).fill_(PAT)
            db.view(torch.int32).fill_(PAT)
        graph.replay()
        torch.cuda.synchronize()
        ref = _wgrad_outputs(dev)
        for (dy, x), (dW, db) in zip(ins, ref):
            ops.linear_bwd_weight(dy, x, out=dW, rowsum=db)
        torch.cuda.synchronize()
        for k in range(WG["n"]):
            assert R.same_bits(outs[k][0], ref[k][0]) and R.same_bits(outs[k][1], ref[k][1]), (seed, k)
