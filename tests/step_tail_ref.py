"""TEST INFRASTRUCTURE for the launches that end a training step (tatt_l2norm, tatt_adam_step, tatt_gather_grads,
tatt_splitk_reduce): float64 references, an fp32 emulation of adam_kernel's operation order with its mutants, the case lists and the
bound checks.  tests/test_step_tail_gpu.py runs the HIP kernels through these checks; tests/test_step_tail_ref.py proves on the CPU
that the checks accept the emulation and reject every mutant.

Every implementation under test -- kernel, emulation, mutant -- has the same call shape and works in place on the buffers it is
handed, canaries included, so that one checker serves them all.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24                      # unit round-off of fp32
CANARY_BITS = 0x7FC0DEAD            # a quiet NaN with a payload: compared bitwise, never by value


def f32(x):
    """The value a C `float` argument takes."""
    return float(np.float32(x))


def canary(n):
    return torch.full((n,), CANARY_BITS, dtype=torch.int32).view(torch.float32)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return bool(torch.equal(bits(a), bits(b)))


# ---------------------------------------------------------------------------------------------------------------------------------
# l2norm
# ---------------------------------------------------------------------------------------------------------------------------------
L2_SIZES = (1, 3, 255, 256, 257, 262144, 262145, 1000003)


def l2norm64(g):
    return float(torch.sqrt((g.double() ** 2).sum()))


def l2_within_one_ulp(got, g):
    """got: the fp32 result.  The kernel sums in double and rounds once: the neighbours of the rounded float64 norm are allowed."""
    ref = l2norm64(g)
    r32 = np.float32(ref)
    lo, hi = np.nextafter(r32, np.float32(-np.inf)), np.nextafter(r32, np.float32(np.inf))
    return float(lo) <= float(got) <= float(hi), ref


# ---------------------------------------------------------------------------------------------------------------------------------
# Adam
# ---------------------------------------------------------------------------------------------------------------------------------
ADAM_SIZES = (1, 3, 4, 5, 7, 1023, 1024, 1025, 1000003)
ADAM_OFFSETS = (0, 4, 16)
ADAM_STEPS = (1, 2, 7, 1000, 2 ** 32 + 3)
ADAM_PAD = 24                       # canary elements behind every segment
ADAM_CANARY = 7.25                  # finite, so that an update applied to a canary changes its bits (arithmetic on a NaN keeps them)
LR, B1, B2, EPS, CLIP = 1e-3, 0.5, 0.999, 1e-8, 0.25
# (max_norm, gnorm, zero_grad): clipping, not clipping, no clip at all (gnorm ignored), a zero gradient with a zero norm, and a pair
# of order 1e-6 where the +1e-6 of the clip denominator decides the coefficient
ADAM_CLIPS = ((CLIP, 16.0, False), (CLIP, 0.1, False), (0.0, 5.0, False), (CLIP, 0.0, True), (2e-6, 3e-6, False))
ADAM_GSCALES = (1.0, 0.125)


def adam_configs():
    return [dict(step=s, max_norm=mn, gnorm=gn, zero_grad=z, gscale=gs)
            for s in ADAM_STEPS for (mn, gn, z) in ADAM_CLIPS for gs in ADAM_GSCALES]


def adam_cases(n):
    """Every configuration at every offset for the small sizes; the million-element size takes a spread of the configurations
    (every clip setting, every step, both scales), the offsets in rotation."""
    cfgs = adam_configs()
    if n <= 2048:
        return [dict(c, n=n, off=o, seed=1000 * n + 7 * i + o) for i, c in enumerate(cfgs) for o in ADAM_OFFSETS]
    pick = [c for i, c in enumerate(cfgs) if i % 3 == 0]
    return [dict(c, n=n, off=ADAM_OFFSETS[i % 3], seed=n + i) for i, c in enumerate(pick)]


def adam_buffers(case):
    """-> p, g, m, v of off + n + ADAM_PAD elements: canaries outside [off, off + n); m and v non-zero and unrelated to g."""
    n, off = case["n"], case["off"]
    gen = torch.Generator().manual_seed(case["seed"])
    out = []
    for kind in "pgmv":
        buf = torch.full((off + n + ADAM_PAD,), ADAM_CANARY)
        if kind == "p":
            val = torch.randn(n, generator=gen)
        elif kind == "g":
            val = torch.randn(n, generator=gen) * 10.0 ** (-3.0 * torch.rand(n, generator=gen))
            if case["zero_grad"]:
                val = torch.zeros(n)
        elif kind == "m":
            val = 0.1 * torch.randn(n, generator=gen)
        else:
            val = 10.0 ** (-1.0 - 6.0 * torch.rand(n, generator=gen))
        buf[off:off + n] = val
        out.append(buf)
    return out


def adam64(p, g, m, v, lr, b1, b2, eps, gnorm, max_norm, gscale, step):
    """float64 Adam of the formula in include/tatt_hip.h on fp32 inputs; scalars as the C floats the kernel receives.
    -> p1, m1, v1, and the pieces the bounds are made of."""
    lr, b1, b2, eps, max_norm, gscale, gnorm = (f32(x) for x in (lr, b1, b2, eps, max_norm, gscale, gnorm))
    p, g, m, v = (t.double() for t in (p, g, m, v))
    coef = gscale
    if max_norm > 0.0:
        coef *= min(1.0, max_norm / (gnorm * gscale + f32(1e-6)))
    bc1, bc2 = 1.0 - b1 ** float(step), 1.0 - b2 ** float(step)
    gi = g * coef
    m1 = b1 * m + (1.0 - b1) * gi
    v1 = b2 * v + (1.0 - b2) * gi * gi
    a1 = lr / bc1
    den = torch.sqrt(v1) / math.sqrt(bc2) + eps
    p1 = p - a1 * m1 / den
    mabs = b1 * m.abs() + (1.0 - b1) * gi.abs()
    return p1, m1, v1, dict(mabs=mabs, a1=a1, den=den)


def adam_emulation(P, G, M, V, off, n, lr, b1, b2, eps, gnorm, max_norm, gscale, step, mutant=None):
    """adam_kernel's operation order in fp32 torch on the CPU, in place on [off, off + n) of the four buffers.  gnorm: fp32 tensor
    of one element, step: int64 tensor of one element (the kernel reads both from device memory).
    `mutant` names one deliberate mistake (ADAM_MUTANTS)."""
    F = torch.float32
    s = lambda x: torch.tensor(x, dtype=F)
    t = int(step.reshape(-1)[0])
    if mutant == "step_int32":
        t = int(np.array([t], dtype=np.int64).astype(np.int32)[0])
    if mutant == "step_off_by_one":
        t += 1
    b1f, b2f = f32(b1), f32(b2)
    bc1, bc2 = s(1.0 - b1f ** float(t)), s(1.0 - b2f ** float(t))
    if mutant == "bc1_missing":
        bc1 = s(1.0)
    if mutant == "bc2_missing":
        bc2 = s(1.0)
    gs = s(gscale)
    coef = gs.clone()
    if max_norm > 0.0 and mutant != "clip_removed":
        gn = gnorm.reshape(-1)[0].to(F)
        den = gn if mutant == "gscale_dropped" else gn * gs
        if mutant != "no_1e-6":
            den = den + s(1e-6)
        c = s(max_norm) / den
        if mutant == "clip_doubled":
            c = c * 2.0
        coef = coef * torch.minimum(c, s(1.0))
    if mutant in ("gscale_dropped", "gscale_norm_only"):
        coef = coef / gs
    a1 = s(lr) / bc1
    rs2 = s(1.0) / torch.sqrt(bc2)
    b1t, b2t, epst = s(b1), s(b2), s(eps)
    end = off + n
    if mutant == "tail_skipped":
        end = off + (n // 4) * 4
    if mutant == "one_past_n":
        end = off + n + 1
    p, g, m, v = (X[off:end] for X in (P, G, M, V))
    gi = g * coef
    mi = b1t * m + (s(1.0) - b1t) * gi
    vi = b2t * v + (s(1.0) - b2t) * gi * gi
    if mutant == "eps_in_sqrt":
        d = torch.sqrt(vi * rs2 * rs2 + epst)
    else:
        d = torch.sqrt(vi) * rs2 + epst
    p1 = p - a1 * mi / d
    m.copy_(mi), v.copy_(vi), p.copy_(p1)


ADAM_MUTANTS = ("clip_doubled", "clip_removed", "gscale_dropped", "gscale_norm_only", "no_1e-6", "step_off_by_one", "bc1_missing",
                "bc2_missing", "eps_in_sqrt", "step_int32", "tail_skipped", "one_past_n")

# Constants of the three bound shapes: 4 x the worst ratio of adam_emulation over every case of adam_cases(n), n in ADAM_SIZES,
# rounded up to a power of two (test_step_tail_ref.py::test_adam_bound_constants measures the ratios and asserts this derivation).
# Measured on the CPU: m 2.178, v 4.066, p 4.629 -> 4 x = 8.7, 16.3, 18.5 -> 16, 32, 32.
ADAM_K = dict(m=16.0, v=32.0, p=32.0)


def k_from_ratio(r):
    return 2.0 ** math.ceil(math.log2(4.0 * r))


def adam_ratios(got, ref):
    """Worst ratio of |got - ref64| to each bound shape with K = 1 -> dict(m=, v=, p=).  A zero bound with a zero error counts 0,
    with a non-zero error (or a NaN) inf."""
    (p, m, v), (p64, m64, v64, x) = got, ref

    def worst(err, bound):
        if not err.numel():
            return 0.0
        r = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf),
                                                                              torch.zeros_like(err)))
        r = torch.where(torch.isnan(r), torch.full_like(r, math.inf), r)
        return float(r.max())
    upd = x["a1"] * x["mabs"] / x["den"]
    return dict(m=worst((m.double() - m64).abs(), U * x["mabs"]),
                v=worst((v.double() - v64).abs(), U * v64),
                p=worst(((p.double() - p64).abs() - U * p64.abs()).clamp_min(0.0), U * upd))


def run_adam_case(impl, case, dev="cpu", K=None):
    """Run `impl` (call shape of adam_emulation without `mutant`) on the case; assert canaries bitwise and m, v, p within the
    bounds; -> ratios to the bound shapes."""
    K = ADAM_K if K is None else K
    n, off = case["n"], case["off"]
    bufs0 = adam_buffers(case)
    bufs = [b.clone().to(dev) for b in bufs0]
    gnorm = torch.tensor([case["gnorm"]], dtype=torch.float32, device=dev)
    step = torch.tensor([case["step"]], dtype=torch.int64, device=dev)
    impl(bufs[0], bufs[1], bufs[2], bufs[3], off, n, LR, B1, B2, EPS, gnorm, case["max_norm"], case["gscale"], step)
    got = [b.cpu() for b in bufs]
    for name, b0, b1 in zip("pgmv", bufs0, got):
        assert same_bits(b0[:off], b1[:off]) and same_bits(b0[off + n:], b1[off + n:]), ("canary of %s overwritten" % name, case)
    assert same_bits(bufs0[1], got[1]), ("the gradient was written", case)
    assert int(step.cpu()) == case["step"] and same_bits(gnorm, torch.tensor([case["gnorm"]])), ("scalars written", case)
    seg = lambda b: b[off:off + n]
    ref = adam64(seg(bufs0[0]), seg(bufs0[1]), seg(bufs0[2]), seg(bufs0[3]), LR, B1, B2, EPS, case["gnorm"], case["max_norm"],
                 case["gscale"], case["step"])
    r = adam_ratios((seg(got[0]), seg(got[2]), seg(got[3])), ref)
    for k in "mvp":
        assert r[k] <= K[k], ("%s outside its bound: ratio %.3g > K %.3g" % (k, r[k], K[k]), case)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
# gradient gather
# ---------------------------------------------------------------------------------------------------------------------------------
GG_MAX = 112
GG_COUNTS = (1, 111, 112, 113, 225)
GG_SIZES = (0, 1, 3, 4, 5, 37, 1023, 1024, 1025, 4097)


def gather_case(count, zero_edges, seed=0):
    """-> (entries, dst0): entries = [(src or None, off, n)] over a destination pre-filled with NaN-pattern canaries; gaps of
    0..7 elements between entries (offsets not multiples of 4), a quarter of the sources missing, a quarter views at element
    offset 1 (16-byte misaligned).  zero_edges: zero-length entries first, last and adjacent in the middle."""
    rng = np.random.RandomState(100 * count + seed + (1 if zero_edges else 0))
    ns = [int(GG_SIZES[rng.randint(len(GG_SIZES))]) for _ in range(count)]
    if zero_edges:
        ns[0] = ns[-1] = 0
        if count >= 5:
            ns[count // 2] = ns[count // 2 + 1] = 0
            ns[count // 2 + 2] = 1025
    else:
        ns[0], ns[-1] = 37, 1025
    entries, off = [], int(rng.randint(1, 8))
    for k, n in enumerate(ns):
        kind = k % 4 if count > 1 else 0
        if not zero_edges and k == count - 1:
            kind = 0
        if kind == 1:
            src = None
        elif kind == 3:
            src = torch.from_numpy(rng.standard_normal(n + 1).astype(np.float32))[1:]
        else:
            src = torch.from_numpy(rng.standard_normal(n).astype(np.float32))
        entries.append((src, off, n))
        off += n + int(rng.randint(0, 8))
    return entries, canary(off + 8).clone()


def gather_cases():
    return [(c, z) for c in GG_COUNTS for z in (True, False)]


def gather_expected(dst0, entries):
    exp = dst0.clone()
    for src, off, n in entries:
        exp[off:off + n] = 0.0 if src is None else src
    return exp


def gather_emulation(dst, entries, mutant=None):
    """What tatt_gather_grads writes, in torch; `mutant` in GATHER_MUTANTS."""
    count = len(entries)
    if mutant == "last_table_dropped" and count > GG_MAX:
        entries = entries[:(count - 1) // GG_MAX * GG_MAX]
    prev_n = None
    for src, off, n in entries:
        lo = 0
        if mutant == "zero_length_shifts" and prev_n == 0:
            lo = min(n, 1024)                 # the successor's first block is taken for the empty entry's and returns early
        prev_n = n
        if src is None:
            if mutant != "none_keeps_old":
                dst[off + lo:off + n] = 0.0
        else:
            dst[off + lo:off + n] = src[lo:]


GATHER_MUTANTS = ("none_keeps_old", "last_table_dropped", "zero_length_shifts")


# ---------------------------------------------------------------------------------------------------------------------------------
# split-K reduction
# ---------------------------------------------------------------------------------------------------------------------------------
RED_S = (1, 2, 3, 4, 5, 12, 13, 16, 17, 29, 128, 256)
# (M, N, remap_cin, remap_taps): M*N = 1, 63, 63, 64, 65, 192*64, 37*5 and a conv-like 9*Cin x Cout
RED_SHAPES = ((1, 1, 1, 1), (63, 1, 7, 9), (9, 7, 1, 9), (8, 8, 4, 2), (5, 13, 5, 1), (192, 64, 64, 3), (37, 5, 37, 1), (18, 4, 2, 9))


def reduce_cases():
    """(S, M, N, cin, taps, vec_len, remap, beta); vec_len: 0 = no vec, M, or a length other than M (N, the conv bias gradient's
    Cout; M + 5 for the square shape)."""
    cases = []
    for S in RED_S:
        for (M, N, cin, taps) in RED_SHAPES:
            for vec_len in (0, M, N if N != M else M + 5):
                for remap in (False, True):
                    for beta in (0.0, 1.0):
                        cases.append((S, M, N, cin, taps, vec_len, remap, beta))
    return cases


def reduce_inputs(case):
    """-> partial (flat: S slabs of M x N, then S vectors of vec_len), C0 (M*N, the prior content of the output), vec0 (vec_len)"""
    S, M, N, cin, taps, vec_len, remap, beta = case
    gen = torch.Generator().manual_seed((S * 7919 + M * 131 + N * 17 + vec_len * 3 + int(remap) * 2 + int(beta)) % (2 ** 31))
    partial = torch.randn(S * M * N + S * vec_len, generator=gen)
    return partial, torch.randn(M * N, generator=gen), torch.randn(vec_len + 1, generator=gen)[:vec_len]


def _scatter(t_mn, case):
    """(M, N) result -> the flat layout of C: row-major, or OIHW dW[co][ci][tap] with i = tap*cin + ci, j = co."""
    S, M, N, cin, taps, vec_len, remap, beta = case
    if not remap:
        return t_mn.reshape(-1)
    return t_mn.reshape(taps, cin, N).permute(2, 1, 0).reshape(-1)


def reduce64(case, partial, C0):
    """-> C64, boundC, vec64, boundV.  |err| <= S u sum_s |partial_s| for an fp32 sum of S terms in any order; beta adds one term
    (beta C0) and one rounding, hence S + 1 there.  vec is overwritten whatever beta is."""
    S, M, N, cin, taps, vec_len, remap, beta = case
    slabs = partial[:S * M * N].double().reshape(S, M, N)
    C = _scatter(slabs.sum(0), case)
    A = _scatter(slabs.abs().sum(0), case)
    terms = S
    if beta != 0.0:
        C = C + beta * C0.double()
        A = A + abs(beta) * C0.double().abs()
        terms += 1
    pv = partial[S * M * N:].double().reshape(S, vec_len)
    return C, terms * U * A, pv.sum(0), S * U * pv.abs().sum(0)


def reduce_emulation(case, partial, C, vec, mutant=None):
    """splitk_reduce in fp32 torch (in place on C / vec); `mutant` in REDUCE_MUTANTS."""
    S, M, N, cin, taps, vec_len, remap, beta = case
    keep = S - S % 4 if mutant == "slab_tail_dropped" else S
    slabs = partial[:S * M * N].reshape(S, M, N)[:keep]
    R = _scatter(slabs.sum(0), case)
    C.copy_(R + beta * C if beta != 0.0 else R)
    if vec_len:
        tail = partial[S * M * N:]
        if mutant == "vec_stride_M":
            tail = torch.cat([tail, torch.zeros(S * max(M, vec_len))])       # (the kernel would read out of bounds here)
            idx = torch.arange(S)[:, None] * M + torch.arange(vec_len)[None, :]
            vec.copy_(tail[idx].sum(0))
        else:
            vec.copy_(tail.reshape(S, vec_len).sum(0))


REDUCE_MUTANTS = ("slab_tail_dropped", "vec_stride_M")


def run_reduce_case(impl, case, dev="cpu"):
    """impl(case, partial, C, vec) in place; asserts C and vec within their bounds -> worst ratio to the bound."""
    S, M, N, cin, taps, vec_len, remap, beta = case
    partial, C0, vec0 = reduce_inputs(case)
    C, vec = C0.clone().to(dev), vec0.clone().to(dev)
    impl(case, partial.to(dev), C, vec if vec_len else None)
    C64, bC, v64, bV = reduce64(case, partial, C0)
    eC = (C.cpu().double() - C64).abs()
    worst = float((eC / bC.clamp_min(1e-300)).max())
    assert bool((eC <= bC).all()), ("C outside S u sum|partial|", case, worst)
    if vec_len:
        eV = (vec.cpu().double() - v64).abs()
        wv = float((eV / bV.clamp_min(1e-300)).max())
        assert bool((eV <= bV).all()), ("vec outside its bound (accumulated, or read at the wrong stride)", case, wv)
        worst = max(worst, wv)
    return worst
