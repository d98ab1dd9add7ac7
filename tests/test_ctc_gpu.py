"""CTC label supervision on the GPU (csrc/ctc.hip, functional.CtcLossFn, losses.CTCLoss / ctc_loss_from_logits, TextPriorSR.set_labels).
Yardstick: torch.nn.functional.ctc_loss on the CPU in float64 (the operator the reference calls, interfaces/super_resolution.py:51) on
`logits.double().log_softmax(2)`; tolerances are multiples of the distance of torch's own CPU float32 evaluation from that yardstick
on the same inputs, measured inside the test."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.fixtures import randomize_state_dict
from tests.util import rel_err

pytestmark = pytest.mark.gpu

# how many times further from float64 than torch's CPU float32 evaluation the HIP result may be (plus the floors below): 4 x, the factor
# test_split_bf16_training_drift_against_the_fp64_yardstick grants a second fp32-width evaluation; the gradients measured below 2 x in
# every case (see test_parity_with_torch_cpu_float64), so theirs is 2
K_F32 = 4.0
K_F32_GRAD = 2.0


# ---- label batches ------------------------------------------------------------------------------------------------------------
def _word(rng, C, L, repeats=0):
    """L codes in 1..C-1 with exactly `repeats` adjacent equal pairs (doubled letters)."""
    w = []
    for i in range(L):
        if i > 0 and i <= repeats:
            w.append(w[-1])
        else:
            c = int(rng.randint(1, C))
            while w and c == w[-1]:
                c = 1 + c % (C - 1)
            w.append(c)
    return w


def _needed(w):
    return len(w) + sum(1 for a, b in zip(w, w[1:]) if a == b)


def make_labels(T, B, C, seed, vary_in_len, with_ignored=True):
    """-> codes (B, T) long padded with 0, tgt_len (B) (-1 = ignored), in_len (B).  One batch holds: length 0, length 1, length in_len,
    doubled letters, a word exactly feasible (L + repeats == in_len) and one infeasible by one, the single [blank] target the
    reference's collate emits for an empty word, an ignored sample; the rest random."""
    rng = np.random.RandomState(seed)
    codes = np.zeros((B, T), dtype=np.int64)
    tl, il = np.zeros(B, dtype=np.int64), np.full(B, T, dtype=np.int64)
    for b in range(B):
        Tb = int(rng.randint(max(2, T // 2), T + 1)) if vary_in_len else T
        kind = (b + (3 if B == 1 else 0)) % 12
        rep = min(2, Tb // 3)
        if kind == 0:
            w = []
        elif kind == 1:
            w = _word(rng, C, 1)
        elif kind == 2:
            w = _word(rng, C, Tb)                                   # every step emits a character
        elif kind == 3:
            w = _word(rng, C, max(2, Tb // 3), repeats=1)
        elif kind == 4:
            w = _word(rng, C, Tb - rep, repeats=rep)                # exactly feasible
            assert _needed(w) == Tb
        elif kind == 5:
            w = _word(rng, C, Tb - rep + 1, repeats=rep) if Tb - rep + 1 <= T else _word(rng, C, Tb, repeats=1)
            assert _needed(w) == Tb + 1                             # infeasible by one
        elif kind == 6:
            w = [0]                                                 # the blank itself as the only target
        elif kind == 7 and with_ignored:
            w = _word(rng, C, 3)
        else:
            w = _word(rng, C, int(rng.randint(0, max(1, Tb // 2) + 1)), repeats=int(rng.randint(0, 2)))
        codes[b, :len(w)] = w
        tl[b] = -1 if (kind == 7 and with_ignored) else len(w)
        il[b] = Tb
    return torch.from_numpy(codes), torch.from_numpy(tl), torch.from_numpy(il)


def yardstick(logits, codes, tl, il, dtype, w=None):
    """torch's CPU operator in `dtype` -> (nll (B), gradient w.r.t. the logits of sum_b w_b nll_b over the finite, non-ignored samples).
    Ignored samples (tl < 0) get nll 0."""
    x = logits.detach().cpu().to(dtype).requires_grad_(True)
    live = tl >= 0
    nll = F.ctc_loss(x.log_softmax(2), codes, il, tl.clamp_min(0), blank=0, reduction="none", zero_infinity=False)
    nll = torch.where(live, nll, torch.zeros_like(nll))
    fin = torch.isfinite(nll) & live
    w = torch.ones(nll.shape[0], dtype=torch.float64) if w is None else w
    (nll[fin] * w[fin].to(dtype)).sum().backward()
    return nll.detach(), x.grad.detach(), fin


def ulp32(v):
    """one fp32 ulp at the magnitude of each element of v"""
    return torch.from_numpy(np.asarray(np.spacing(np.abs(v.double().numpy()).astype(np.float32)), dtype=np.float64)).reshape(v.shape)


def _hip(dev, logits, codes, tl, il, w, normalized, layout, zero_infinity=False, concat=False, vary_in_len=True):
    """-> (nll, gradient w.r.t. the logits of sum over the finite samples of w_b nll_b) by the HIP path."""
    from tatt_amd.losses import CTCLoss, ctc_loss_from_logits
    T, B, C = logits.shape
    if layout == "btc":                                              # a (B, T, C)-major buffer viewed as (T, B, C)
        base = logits.permute(1, 0, 2).contiguous().to(dev).requires_grad_(True)
        x = base.permute(1, 0, 2)
        assert not x.is_contiguous() or B == 1
    else:
        base = logits.clone().to(dev).requires_grad_(True)
        x = base
    if normalized:
        if concat:                                                   # torch's concatenated 1-D targets, everything from the host
            tg = torch.cat([codes[b, :max(int(tl[b]), 0)] for b in range(B)])
            nll = CTCLoss(reduction="none", zero_infinity=zero_infinity)(x.log_softmax(2), tg, il.tolist(), tl.tolist())
        else:
            nll = CTCLoss(reduction="none", zero_infinity=zero_infinity)(x.log_softmax(2), codes.to(dev), il.to(dev), tl.to(dev))
    else:
        nll = ctc_loss_from_logits(x, codes.to(dev).int(), tl.to(dev).int(), il.to(dev).int() if vary_in_len else None,
                                   zero_infinity=zero_infinity)
    fin = torch.isfinite(nll)
    (nll[fin] * w.to(dev).float()[fin]).sum().backward()
    g = base.grad.permute(1, 0, 2) if layout == "btc" else base.grad
    return nll.detach().cpu(), g.detach().cpu()


CASES = [(26, 48, 37), (64, 16, 128), (7, 1, 5)]


@pytest.mark.parametrize("scale", [1.0, 3.0, 10.0])
@pytest.mark.parametrize("T,B,C", CASES)
def test_parity_with_torch_cpu_float64(dev, T, B, C, scale):
    """Losses and gradients of the HIP operator against torch's CPU float64 operator; the bound is K_F32 x the distance of torch's own
    CPU float32 evaluation from float64 on the same inputs (largest distance over the batch), plus 8 fp32 ulps of the yardstick for
    the losses and 8 * 2^-24 absolute for the gradients.  Variants: raw logits (fused log-softmax) and log-probabilities (drop-in
    module), in_len = T for all and varying in_len < T, padded device targets and concatenated host targets, a (B, T, C)-major
    strided view of x.

    Measured on an MI355X, largest ratio of the HIP distance to the float32-CPU distance over the variants of a case, (loss, gradient):
      (26, 48, 37)   scale 1: 1.00, 1.21   scale 3: 1.00, 1.20   scale 10: 1.00, 1.15
      (64, 16, 128)  scale 1: 1.74, 0.83   scale 3: 1.00, 1.06   scale 10: 1.00, 1.06
      (7, 1, 5)      scale 1: 1.00, 1.20   scale 3: 7.83, 0.47   scale 10: 1.00, 1.39
    Absolute: losses 1.4e-5 .. 1.3e-4 from float64 at B = 48 / 16 (torch's float32: the same figures), gradients 2e-5 .. 2e-4.  The 7.83
    is one sample whose float32-CPU loss happens to land 2.2e-7 from float64 while the kernel's is 1.7e-6 away, 2 ulps of the loss: inside
    the 8-ulp floor.  Every gradient ratio is below 2, so the gradient factor is 2; the loss factor stays 4."""
    g = torch.Generator().manual_seed(1000 + T + int(scale))
    logits = torch.randn(T, B, C, generator=g) * scale
    w = torch.randn(B, generator=g, dtype=torch.float64)
    worst = [0.0, 0.0]
    for vary in (False, True):
        codes, tl, il = make_labels(T, B, C, seed=T * 7 + B, vary_in_len=vary)
        n64, g64, fin64 = yardstick(logits, codes, tl, il, torch.float64, w)
        n32, g32, fin32 = yardstick(logits, codes, tl, il, torch.float32, w)
        assert torch.equal(fin64, fin32)
        if B > 1:
            assert bool((~fin64 & (tl >= 0)).any()) and bool(fin64.any()) and bool((tl < 0).any())
        d_l32 = float((n32.double()[fin64] - n64[fin64]).abs().max())
        d_g32 = float((g32.double() - g64)[:, fin64].abs().max())
        variants = [(0, "tbc", False)] if not vary else [(0, "tbc", False), (0, "btc", False), (1, "tbc", False), (1, "btc", True)]
        for normalized, layout, concat in variants:
            nh, gh = _hip(dev, logits, codes, tl, il, w, normalized, layout, concat=concat, vary_in_len=vary)
            finh = torch.isfinite(nh)
            assert torch.equal(finh, fin64 | (tl < 0)), "the infeasible samples differ from torch's"
            assert bool((nh[~finh] == float("inf")).all()) and bool((nh[tl < 0] == 0).all())
            d_l = (nh.double() - n64)[fin64].abs()
            d_g = float((gh.double() - g64)[:, fin64].abs().max())
            lim_l = K_F32 * d_l32 + 8.0 * ulp32(n64[fin64])
            lim_g = K_F32_GRAD * d_g32 + 8.0 * 2.0 ** -24
            r_l, r_g = float(d_l.max()) / max(d_l32, 1e-300), d_g / max(d_g32, 1e-300)
            worst = [max(worst[0], r_l), max(worst[1], r_g)]
            print("ctc parity T=%d B=%d C=%d scale=%g vary=%d norm=%d %s concat=%d: loss |d| hip %.3e f32cpu %.3e (x%.2f)  "
                  "grad |d| hip %.3e f32cpu %.3e (x%.2f)" % (T, B, C, scale, vary, normalized, layout, concat, float(d_l.max()), d_l32,
                                                            r_l, d_g, d_g32, r_g))
            assert bool((d_l <= lim_l).all()), (float(d_l.max()), d_l32)
            assert d_g <= lim_g, (d_g, d_g32)
            assert bool((gh[:, tl < 0] == 0).all())
    print("ctc parity T=%d B=%d C=%d scale=%g WORST ratio loss x%.2f grad x%.2f" % (T, B, C, scale, worst[0], worst[1]))


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
def test_reductions_against_torch(dev, reduction):
    """CTCLoss(reduction=...) and ctc_loss_from_logits(reduction=...) against torch's CPU float64 value; same bound as the parity test
    (K_F32 x the float32-CPU distance + 8 ulps).  zero_infinity=True so that the sums stay finite."""
    from tatt_amd.losses import CTCLoss, ctc_loss_from_logits
    T, B, C = 26, 48, 37
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(T, B, C, generator=g) * 3.0
    codes, tl, il = make_labels(T, B, C, seed=3, vary_in_len=True, with_ignored=False)
    ref = lambda dt: F.ctc_loss(logits.to(dt).log_softmax(2), codes, il, tl, blank=0, reduction=reduction, zero_infinity=True)
    r64, r32 = ref(torch.float64), ref(torch.float32).double()
    d32 = float((r32 - r64).abs().max())
    x = logits.to(dev)
    a = CTCLoss(reduction=reduction, zero_infinity=True)(x.log_softmax(2), codes.to(dev), il.to(dev), tl.to(dev))
    b = ctc_loss_from_logits(x, codes.to(dev).int(), tl.to(dev).int(), il.to(dev).int(), reduction=reduction, zero_infinity=True)
    assert a.shape == r64.shape and b.shape == r64.shape
    for got in (a, b):
        d = (got.cpu().double() - r64).abs()
        print("ctc reduction %s: |d| hip %.3e f32cpu %.3e" % (reduction, float(d.max()), d32))
        assert bool((d <= K_F32 * d32 + 8.0 * ulp32(r64)).all()), (reduction, float(d.max()), d32)


@pytest.mark.parametrize("scale", [3.0, 10.0])
def test_exact_properties(dev, scale):
    """What must hold exactly: the infeasible set is torch's; those samples are +inf with a non-finite gradient (zero_infinity=False) or
    0.0 with a zero gradient (True); ignored samples and rows t >= in_len have zero gradient; the unit gradient's rows sum to 0 up to
    K_F32 x the largest row sum of torch's CPU float32 gradient + C * 2^-22; two runs are bitwise equal."""
    from tatt_amd.losses import ctc_loss_from_logits
    T, B, C = 26, 48, 37
    g = torch.Generator().manual_seed(77)
    logits = torch.randn(T, B, C, generator=g) * scale
    codes, tl, il = make_labels(T, B, C, seed=9, vary_in_len=True)
    n64, _, fin64 = yardstick(logits, codes, tl, il, torch.float64)
    _, g32, _ = yardstick(logits, codes, tl, il, torch.float32)
    infeasible = ~fin64 & (tl >= 0)
    assert bool(infeasible.any())
    cd, td, idv = codes.to(dev).int(), tl.to(dev).int(), il.to(dev).int()
    live_rows = (torch.arange(T)[:, None] < il[None, :]) & fin64[None, :] & (tl >= 0)[None, :]          # (T, B)
    rs32 = float(g32.sum(2)[live_rows].abs().max())
    # torch's CPU gradient for a target EQUAL to the blank does not sum to zero in its last row (it assigns where it should add), which
    # would make the bound above vacuous: the same check again over the samples whose targets hold no blank, against torch's row sums there
    no_blank = torch.tensor([bool((codes[b, :max(int(tl[b]), 0)] != 0).all()) for b in range(B)])
    proper_rows = live_rows & no_blank[None, :]
    rs32p = float(g32.sum(2)[proper_rows].abs().max())
    assert rs32p < 1e-3 and bool((~no_blank).any())
    runs = []
    for zi in (False, True, False):
        x = logits.clone().to(dev).requires_grad_(True)
        nll = ctc_loss_from_logits(x, cd, td, idv, zero_infinity=zi)
        nll.sum().backward()
        nll, gx = nll.detach().cpu(), x.grad.detach().cpu()
        runs.append((nll, gx))
        if zi:
            assert bool(torch.isfinite(nll).all())
        else:
            assert torch.equal(~torch.isfinite(nll), infeasible), "the infeasible samples differ from torch's"
        for b in torch.nonzero(infeasible).reshape(-1).tolist():
            if zi:
                assert float(nll[b]) == 0.0 and bool((gx[:, b] == 0).all())
            else:
                assert float(nll[b]) == float("inf") and not bool(torch.isfinite(gx[:int(il[b]), b]).any())
        assert bool((nll[tl < 0] == 0).all()) and bool((gx[:, tl < 0] == 0).all())
        pad_rows = torch.arange(T)[:, None] >= il[None, :]
        assert bool((gx[pad_rows] == 0).all())
        rs = float(gx.sum(2)[live_rows].abs().max())
        print("ctc row sums scale=%g zero_infinity=%d: hip %.3e f32cpu %.3e" % (scale, zi, rs, rs32))
        assert rs <= K_F32 * rs32 + C * 2.0 ** -22, (rs, rs32)
        rsp = float(gx.sum(2)[proper_rows].abs().max())
        print("ctc row sums, targets without a blank: hip %.3e f32cpu %.3e" % (rsp, rs32p))
        assert rsp <= K_F32 * rs32p + C * 2.0 ** -22, (rsp, rs32p)
    assert torch.equal(runs[0][0].view(torch.int32), runs[2][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int32), runs[2][1].view(torch.int32))


def test_label_data_out_of_range_is_infeasible_not_a_fault(dev):
    """Codes outside [0, C), offsets / lengths that leave the codes array, input lengths outside [0, T]: the sample is infeasible; its
    neighbours are untouched.  Geometries outside the kernel's capacity raise."""
    from tatt_amd import functional as Fh
    T, B, C = 12, 6, 9
    g = torch.Generator().manual_seed(2)
    x = (torch.randn(T, B, C, generator=g) * 2).to(dev)
    i32 = lambda v: torch.tensor(v, dtype=torch.int32, device=dev)
    codes = i32([1, 2, 3, 4, 1, 2, 99, 4, 1, -5, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4, 1, 2, 3, 4])
    offs, tl, il = i32([0, 4, 8, 12, 22, 20]), i32([4, 4, 4, 4, 4, 4]), i32([12, 12, 12, 13, 12, -1])
    nll = Fh.CtcLossFn.apply(x, codes, offs, tl, il, 0, False, False).cpu()
    assert torch.isfinite(nll[0]) and bool((nll[1:] == float("inf")).all()), nll
    good = Fh.CtcLossFn.apply(x[:, :1], codes[:4].contiguous(), i32([0]), i32([4]), None, 0, False, False).cpu()
    assert torch.equal(good, nll[:1])
    nll0 = Fh.CtcLossFn.apply(x, codes, offs, tl, il, 0, True, False).cpu()
    assert bool((nll0[1:] == 0).all()) and torch.equal(nll0[:1], nll[:1])
    with pytest.raises(RuntimeError):
        Fh.CtcLossFn.apply(torch.zeros(65, 1, 8, device=dev), i32([1]), i32([0]), i32([1]), None, 0, False, False)
    with pytest.raises(RuntimeError):
        Fh.CtcLossFn.apply(torch.zeros(8, 1, 129, device=dev), i32([1]), i32([0]), i32([1]), None, 0, False, False)
    with pytest.raises(RuntimeError):
        Fh.CtcLossFn.apply(x, codes.long(), offs, tl, il, 0, False, False)


def test_captured_launches_read_new_labels_on_replay(dev):
    """ctc_loss_from_logits forward + backward captured once; codes, lengths and logits rewritten IN PLACE; the replay equals an eager
    call on the new data bit for bit and differs from the captured step's values."""
    from tatt_amd.losses import ctc_loss_from_logits
    T, B, C = 26, 48, 37
    g = torch.Generator().manual_seed(31)
    data = []
    for k in range(2):
        codes, tl, il = make_labels(T, B, C, seed=40 + k, vary_in_len=False)
        data.append(((torch.randn(T, B, C, generator=g) * 3).to(dev), codes.to(dev).int(), tl.to(dev).int()))
    w = torch.randn(B, generator=g).to(dev)
    x = data[0][0].clone()
    codes, tl = data[0][1].clone(), data[0][2].clone()

    def step():
        # a fresh leaf over the static buffer per call (as GradCuts.cut makes them): a leaf that an eager backward on another stream has
        # used keeps its AccumulateGrad node on that stream, and the engine would then tie that stream into the capture
        xv = x.detach().requires_grad_(True)
        nll = ctc_loss_from_logits(xv, codes, tl, zero_infinity=True)
        gx, = torch.autograd.grad((nll * w).sum(), xv)
        return nll.detach(), gx
    eager = []
    for xs, cs, ls in data:
        x.copy_(xs); codes.copy_(cs); tl.copy_(ls)
        n_, g_ = step()
        eager.append((n_.clone(), g_.clone()))
    x.copy_(data[0][0]); codes.copy_(data[0][1]); tl.copy_(data[0][2])
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        step()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        nll_s, gx_s = step()
    for k in (0, 1, 0):
        x.copy_(data[k][0]); codes.copy_(data[k][1]); tl.copy_(data[k][2])
        gph.replay()
        torch.cuda.synchronize()
        assert torch.equal(nll_s, eager[k][0]) and torch.equal(gx_s, eager[k][1]), k
    assert not torch.equal(eager[0][0], eager[1][0]) and not torch.equal(eager[0][1], eager[1][1])


def test_registry_op_equals_the_autograd_function(dev):
    from tatt_amd import functional as Fh
    T, B, C = 26, 48, 37
    g = torch.Generator().manual_seed(8)
    x = (torch.randn(T, B, C, generator=g) * 3).to(dev)
    codes, tl, il = make_labels(T, B, C, seed=1, vary_in_len=True)
    cd, td, idv = codes.to(dev).int().contiguous(), tl.to(dev).int(), il.to(dev).int()
    offs = (torch.arange(B, device=dev, dtype=torch.int32) * T)
    for normalized, zi, inl in ((False, False, idv), (True, True, None)):
        xin = x.log_softmax(2) if normalized else x
        a = torch.ops.tatt_hip.ctc_loss(xin, cd, offs, td, inl, 0, zi, normalized)
        b = Fh.CtcLossFn.apply(xin, cd, offs, td, inl, 0, zi, normalized)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- in the model -------------------------------------------------------------------------------------------------------------
WORDS = ["", "a", "hello", "Bookkeeper", "x" * 30, "?!", "zz9", "street", "aa", "mississippi", "q8", "the", "0123456789", "llama"]


def _words(B, step):
    return [WORDS[(3 * step + 5 * b + b // 7) % len(WORDS)] for b in range(B)]


def _crnn_sd():
    import tatt_amd
    torch.manual_seed(1234)
    return randomize_state_dict(tatt_amd.CRNN(32, 1, 37, 256).state_dict())


def _build(dev, teacher, detach, **kwargs):
    import tatt_amd
    from tatt_amd.train import TextPriorSR
    torch.manual_seed(1234)
    sr_m = tatt_amd.TSRN_TL_TRANS(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    sr_m.load_state_dict(randomize_state_dict(sr_m.state_dict()))
    tpg = tatt_amd.CRNN(32, 1, 37, 256)
    tpg.load_state_dict(_crnn_sd())
    tch = None
    if teacher:
        tch = tatt_amd.CRNN(32, 1, 37, 256)
        tch.load_state_dict(randomize_state_dict(tch.state_dict(), seed=5))
    m = TextPriorSR(sr_m, tpg, teacher=tch, detach_prior=detach, **kwargs).to(dev).train()
    sr_m.infoGen.dropout_on = False
    return m


def _term64(m, x, words, weight):
    """weight * mean_b(nll_b * tic_b) with nll from the float64 yardstick on the student's logits (infeasible and ignored words: 0)."""
    from tatt_amd.crnn import parse_crnn_data
    from tatt_amd.train import encode_label_batch
    with torch.no_grad():
        logits = m.tpg(parse_crnn_data(x[:, :3], m.in_width)).detach().cpu().double()
    codes, lens, tics = encode_label_batch(words)
    T, B, _ = logits.shape
    nll = F.ctc_loss(logits.log_softmax(2), codes.long().clamp_min(0), torch.full((B,), T, dtype=torch.long), lens.long().clamp_min(0),
                     blank=0, reduction="none", zero_infinity=True)
    nll = torch.where(lens >= 0, nll, torch.zeros_like(nll))
    return weight * float((nll * tics.double()).mean())


def _state(m):
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).cpu()


@pytest.mark.parametrize("detach", [True, False])
@pytest.mark.parametrize("teacher", [True, False])
@pytest.mark.parametrize("B", [3, 48])
def test_label_term_in_the_model(dev, B, teacher, detach):
    """TextPriorSR with label_weight: 0 is bitwise the model built without the keyword; 0.5 adds 0.5 * mean(nll * tic) of the float64
    yardstick on the student's logits (1e-6 relative on the loss); the staged backward delivers the term's gradient at stage "tpg"
    (== the single-pass gradient, 1e-5); a hipGraph-replayed Trainer fed different labels every step equals the eager Trainer (1e-6);
    one TssimRecipe step includes the term; with the label term alone driving the recogniser, 20 replayed steps lower it."""
    from oracle.fixtures import make_inputs
    from tatt_amd import functional as Fh
    from tatt_amd.train import Trainer, TssimRecipe, image_loss_mean
    x, _, hr = make_inputs(B, seed=11)
    x, hr = x.to(dev), hr.to(dev)
    # label_weight = 0: nothing differs
    res = []
    for kw in ({}, {"label_weight": 0.0}):
        m = _build(dev, teacher, detach, **kw)
        assert not hasattr(m, "_labels")
        loss = Trainer(m, use_graph=False).step(x, None, hr)
        res.append((loss.cpu(), [None if p.grad is None else p.grad.cpu() for p in m.parameters()]))
    assert torch.equal(res[0][0], res[1][0])
    for a, b in zip(res[0][1], res[1][1]):
        assert (a is None and b is None) or torch.equal(a, b)
    base = float(res[0][0])
    # label_weight = 0.5: the loss, single pass
    words = _words(B, 0)
    m = _build(dev, teacher, detach, label_weight=0.5)
    with pytest.raises(RuntimeError):
        m(x)                                                       # no labels set
    m.set_labels(words[:B - 1] if B > 1 else words + words)
    with pytest.raises(RuntimeError):
        m(x)                                                       # labels of another batch size
    term = _term64(m, x, words, 0.5)
    assert term > 0.0
    want = base + term
    m = _build(dev, teacher, detach, label_weight=0.5)
    m.set_labels(words)
    sr, _ = m(x)
    loss = image_loss_mean(sr, hr, scale=100.0) + m.extra_loss(hr)
    loss.backward()
    got1, g_ref = float(loss.detach()), m.tpg.rnn[1].embedding.weight.grad.clone()
    print("label term B=%d teacher=%d detach=%d: base %.6f term %.6f single-pass %.6f want %.6f" % (B, teacher, detach, base, term, got1, want))
    assert abs(got1 - want) < 1e-6 * abs(want), (got1, want)
    # staged Trainer
    m = _build(dev, teacher, detach, label_weight=0.5)
    m.set_labels(words)
    tr = Trainer(m, use_graph=False)
    assert tr.stages[-1] == "tpg"
    got = float(tr.step(x, None, hr))
    assert abs(got - want) < 1e-6 * abs(want), (got, want)
    assert rel_err(m.tpg.rnn[1].embedding.weight.grad, g_ref) < 1e-5
    # graph replay with different labels every step == eager
    out = []
    for use_graph in (False, True):
        m = _build(dev, teacher, detach, label_weight=0.5)
        tr = Trainer(m, use_graph=use_graph, warmup_eager=2)
        ls = []
        for k in range(6):
            m.set_labels(_words(B, k))
            ls.append(float(tr.step(x, None, hr)))
        out.append((ls, _state(m)))
    assert abs(out[0][0][0] - want) < 1e-6 * abs(want)
    for a, b in zip(*[o[0] for o in out]):
        assert abs(a - b) <= 1e-6 * abs(a), (out[0][0], out[1][0])
    assert float((out[0][1] - out[1][1]).abs().max()) <= 1e-6
    # the shipped recipe reaches the term through model.extra_loss
    rl = []
    for lw in (0.0, 0.5):
        m = _build(dev, teacher, detach, label_weight=lw)
        if lw:
            m.set_labels(words)
        rec = TssimRecipe(5.0, seed=4)
        rl.append(float(Trainer(m, use_graph=False, recipe=rec).step(x, None, hr)))
    with torch.no_grad():
        x_rot = Fh.AffineSampleFn.apply(x, rec.theta_pos)
    term_rot = _term64(_build(dev, teacher, detach, label_weight=0.5), x_rot, words, 0.5)
    assert term_rot > 0.0 and abs((rl[1] - rl[0]) - term_rot) < 2e-6 * abs(rl[1]), (rl, term_rot)
    # the label term alone trains the recogniser
    if not teacher:
        m = _build(dev, teacher, detach, label_weight=0.5)
        tr = Trainer(m, use_graph=True, warmup_eager=2)
        before = _term64(m, x, words, 0.5)
        for _ in range(20):
            m.set_labels(words)
            tr.step(x, None, hr)
        after = _term64(m, x, words, 0.5)
        print("label term over 20 replayed steps: %.5f -> %.5f" % (before, after))
        assert after < before, (before, after)
