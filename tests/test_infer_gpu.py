"""Inference session on the GPU: the eval-only kernels (one-launch LSTM layer, BatchNorm fold, greedy CTC match) against the per-step
kernels / float64 restatements, and the graph-captured session against the eager eval path, the golden vectors and the oracle."""
import numpy as np
import pytest
import torch

from oracle import tatt_oracle as O
from oracle.fixtures import make_inputs, randomize_state_dict
from tests.util import max_err

pytestmark = pytest.mark.gpu
STD = dict(scale_factor=2, width=128, height=32, STN=True, mask=True, srb_nums=5, hidden_units=32)
VOC_TYPES = ("digit", "lower", "upper", "all")


def build(cls, dev, seed=1234, **kw):
    import tatt_amd
    torch.manual_seed(seed)
    m = getattr(tatt_amd, cls)(**kw)
    m.load_state_dict(randomize_state_dict(m.state_dict()))
    return m.to(dev)


def build_crnn(dev, seed=5):
    import tatt_amd
    torch.manual_seed(seed)
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=seed))
    return c.to(dev).eval()


# ---- LSTM layer in one launch ------------------------------------------------------------------------------------------------------
def _lstm_case(dev, T, B, I=256, H=256, seed=0):
    g = torch.Generator().manual_seed(seed)
    rnn = torch.nn.LSTM(I, H, bidirectional=True)
    with torch.no_grad():
        for p in rnn.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * 0.06)
    x = torch.randn(T, B, I, generator=g)
    return rnn, x


@pytest.mark.parametrize("B", [1, 5, 48, 128])
@pytest.mark.parametrize("T", [1, 7, 26])
def test_lstm_chain_bitwise_and_fp64(dev, B, T):
    import tatt_amd
    from tatt_amd import ops
    from tatt_amd._lib import LIB
    from tatt_amd.infer import bilstm_eval, lstm_input_projection
    rnn, x = _lstm_case(dev, T, B, seed=B * 100 + T)
    ref = rnn.double()(x.double())[0]
    rg = torch.nn.LSTM(256, 256, bidirectional=True).to(dev)
    rg.load_state_dict({k: v.float() for k, v in rnn.state_dict().items()})
    xd = x.to(dev)
    with torch.no_grad():
        # the chain entry itself: it must take every B <= 128 (a silent fall-back would compare the step kernels with themselves)
        gi = lstm_input_projection(xd, rg)
        chain = torch.full((T, B, 512), float("nan"), device=dev)
        sync = torch.zeros(1024, dtype=torch.int32, device=dev)
        rc = LIB.tatt_lstm_fwd_chain(ops.P(gi), ops.P(rg.weight_hh_l0), ops.P(rg.weight_hh_l0_reverse), ops.P(rg.bias_hh_l0),
                                     ops.P(rg.bias_hh_l0_reverse), ops.P(chain), ops.P(sync), T, B, 256, ops.stream())
        assert rc == 0
        step = bilstm_eval(xd, rg, chain=False)
        via_session_path = bilstm_eval(xd, rg, chain=True)
    torch.cuda.synchronize()
    assert int(sync[1023]) == 0
    assert torch.equal(chain, step), max_err(chain, step)
    assert torch.equal(via_session_path, step)
    assert max_err(chain, ref) < 1e-5, max_err(chain, ref)
    tatt_amd.sync_check()


def test_lstm_chain_fallback_beyond_capacity(dev):
    """B = 200 needs 416 work-groups: the chain entry declines (code 1) and the per-step kernels give the same result."""
    import tatt_amd
    from tatt_amd import ops
    from tatt_amd._lib import LIB
    from tatt_amd.infer import bilstm_eval, lstm_chain_capacity
    assert lstm_chain_capacity(dev) >= 256
    rnn, x = _lstm_case(dev, 26, 200, seed=3)
    rg = torch.nn.LSTM(256, 256, bidirectional=True).to(dev)
    rg.load_state_dict(rnn.state_dict())
    xd = x.to(dev)
    sync = torch.zeros(1024, dtype=torch.int32, device=dev)
    gi, out = torch.zeros(26 * 200, 2048, device=dev), torch.zeros(26, 200, 512, device=dev)
    rc = LIB.tatt_lstm_fwd_chain(ops.P(gi), ops.P(rg.weight_hh_l0), ops.P(rg.weight_hh_l0_reverse), ops.P(rg.bias_hh_l0),
                                 ops.P(rg.bias_hh_l0_reverse), ops.P(out), ops.P(sync), 26, 200, 256, ops.stream())
    assert rc == 1
    with torch.no_grad():
        a = bilstm_eval(xd, rg, chain=True)
        b = bilstm_eval(xd, rg, chain=False)
    assert torch.equal(a, b)
    assert max_err(a, rnn.double()(x.double())[0]) < 1e-5
    tatt_amd.sync_check()


# ---- BatchNorm fold ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [True, False])
def test_bn_fold_against_fp64(dev, with_bias):
    from tatt_amd.infer import bn_fold
    g = torch.Generator().manual_seed(7)
    conv = torch.nn.Conv2d(64, 96, 3, padding=1, bias=with_bias)
    bn = torch.nn.BatchNorm2d(96)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        if with_bias:
            conv.bias.copy_(torch.randn(96, generator=g))
        bn.weight.copy_(torch.randn(96, generator=g))                  # negative gamma included
        bn.bias.copy_(torch.randn(96, generator=g))
        bn.running_mean.copy_(torch.randn(96, generator=g))
        var = torch.rand(96, generator=g) * 2
        var[:8] = torch.tensor([0.0, 1e-9, 1e-7, 1e-6, 1e-5, 3e-5, 1e-4, 1e-3])     # near zero: eps dominates
        bn.running_var.copy_(var)
    conv, bn = conv.to(dev), bn.to(dev).eval()
    with torch.no_grad():
        w, b = bn_fold(conv.weight, conv.bias, bn)
    s = bn.weight.detach().double().cpu() / torch.sqrt(bn.running_var.double().cpu() + bn.eps)
    w_ref = conv.weight.detach().double().cpu() * s.reshape(-1, 1, 1, 1)
    b0 = conv.bias.detach().double().cpu() if with_bias else torch.zeros(96, dtype=torch.float64)
    b_ref = (b0 - bn.running_mean.double().cpu()) * s + bn.bias.detach().double().cpu()
    assert float(((w.detach().double().cpu() - w_ref).abs() / (w_ref.abs() + 1e-30)).max()) < 1e-6
    assert float(((b.double().cpu() - b_ref).abs() / (b_ref.abs() + 1e-6)).max()) < 1e-5
    # and the folded convolution is the conv -> eval BatchNorm composition
    x = torch.randn(2, 64, 8, 8, device=dev)
    with torch.no_grad():
        y_ref = torch.nn.functional.batch_norm(torch.nn.functional.conv2d(x.double(), conv.weight.double(), conv.bias.double() if with_bias else None, padding=1),
                                               bn.running_mean.double(), bn.running_var.double(), bn.weight.double(), bn.bias.double(), False, 0.0, bn.eps)
        y = torch.nn.functional.conv2d(x.double(), w.double(), b.double(), padding=1)
    assert float((y - y_ref).abs().max()) < 1e-4 * float(y_ref.abs().max())


# ---- greedy CTC decode and match ---------------------------------------------------------------------------------------------------
def _ctc_logits(T=26, B=96, C=37, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 4, (T, B, C), generator=g).float()               # few distinct values: exact ties everywhere
    x[:, 0:8, 0] = 10.0                                                   # all-blank rows
    for b in range(8, 16):                                                # repeats separated by blanks: a a - a b b - b
        for t, c in enumerate([5, 5, 0, 5, 12, 12, 0, 12]):
            x[t, b] = 0.0
            x[t, b, c] = 1.0
    x[:, 16:40] = torch.randn(T, 24, C, generator=g)                      # generic rows
    x[3, 40, :] = 2.0                                                     # a whole step tied: class 0 wins
    return x


@pytest.mark.parametrize("voc", VOC_TYPES)
def test_ctc_greedy_match_against_host(dev, voc):
    from tatt_amd.infer import ctc_greedy_match, encode_labels, keep_mask, D2A
    from tatt_amd.io import ctc_greedy_decode, str_filt
    x = _ctc_logits(seed=len(voc))
    T, B, C = x.shape
    preds = ctc_greedy_decode(x)
    labels = []
    for b, p in enumerate(preds):                                         # matching labels, near misses, upper case, punctuation
        labels.append([p, p.upper(), p + "!", p[:-1], "x" + p, "", p][b % 7])
    codes, lens = encode_labels(labels, voc)
    keep = torch.tensor(keep_mask(voc), dtype=torch.int32, device=dev)
    lab = torch.tensor(codes, dtype=torch.int32, device=dev)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    xd = x.to(dev)
    correct, dec, dlen = ctc_greedy_match(xd, keep, lab, ln, counter, want_decoded=True)
    want = [str_filt(p, voc) == str_filt(t, voc) for p, t in zip(preds, labels)]
    assert correct.cpu().tolist() == [int(w) for w in want]
    assert int(counter) == sum(want) and sum(want) > 0
    for b in range(B):
        n = int(dlen[b])
        assert "".join(D2A[i] for i in dec[b, :n].tolist()) == str_filt(preds[b], voc), b
    # a non-contiguous (B-major) view of the same logits decodes the same way
    xt = xd.permute(1, 0, 2).contiguous().permute(1, 0, 2)
    assert torch.equal(ctc_greedy_match(xt, keep, lab, ln), correct)


# ---- the session against the eager eval path ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cls,tatt", [("tatt_eval_b2", "TSRN_TL_TRANS", True), ("tsrn_eval_b2", "TSRN", False)])
def test_session_golden_b2(dev, name, cls, tatt):
    from tatt_amd.infer import InferenceSession
    z = np.load("tests/golden/%s.npz" % name)
    m = build(cls, dev, **STD)
    s = InferenceSession(m, batch_size=2)
    x = torch.from_numpy(z["x"]).to(dev)
    sr, w, prior = s.run(x, text_prior=torch.from_numpy(z["tp"]).to(dev) if tatt else None)
    assert prior is None
    assert max_err(sr, torch.from_numpy(z["sr"])) < 2e-5, max_err(sr, torch.from_numpy(z["sr"]))
    if tatt:
        assert max_err(w, torch.from_numpy(z["pr_weights"])) < 1e-5
    else:
        assert w is None


@pytest.mark.parametrize("arith", ["split_bf16", "fp32"])
def test_session_b48_against_eager_and_oracle(dev, arith):
    import tatt_amd
    from tatt_amd.infer import InferenceSession
    kw = dict(STD, STN=False)
    m = build("TSRN_TL_TRANS", dev, **kw).eval()
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert any(float(v.abs().max()) > 0.05 for k, v in sd0.items() if k.endswith("running_mean"))
    x, tp, _ = make_inputs(48, seed=48)
    prev = tatt_amd.get_arithmetic()
    tatt_amd.set_arithmetic(arith)
    try:
        with torch.no_grad():
            y, w = m(x.to(dev), tp.to(dev))
        s = InferenceSession(m, batch_size=48)
        sr, pw, _ = s.run(x.to(dev), text_prior=tp.to(dev))
        torch.cuda.synchronize()
    finally:
        tatt_amd.set_arithmetic(prev)
    assert max_err(sr, y) < 2e-5, max_err(sr, y)
    assert max_err(pw, w) < 1e-5, max_err(pw, w)
    o = O.generator_forward(sd0, x, tp, training=False, tatt=True, stn=False)
    assert max_err(sr, o["sr"]) < 2e-5, max_err(sr, o["sr"])
    assert max_err(pw, o["pr_weights"]) < 1e-5


def test_session_tbsrn_equals_eager(dev):
    from tatt_amd.infer import InferenceSession
    m = build("TBSRN", dev, scale_factor=2, width=512, height=32, STN=False, mask=True).eval()
    x = torch.rand(2, 4, 16, 256, generator=torch.Generator().manual_seed(2)).to(dev)
    with torch.no_grad():
        y = m(x)
    # the session captures TBSRN's own eval forward: it switches the module to eval for that and must give every submodule its own
    # flag back -- here a training module holding a frozen (eval) BatchNorm
    m.train()
    frozen = [mod for mod in m.modules() if isinstance(mod, torch.nn.BatchNorm2d)][0]
    frozen.eval()
    flags = [mod.training for mod in m.modules()]
    assert any(flags) and not all(flags)
    s = InferenceSession(m, batch_size=2, lr_size=(16, 256))
    sr, _, _ = s.run(x)
    torch.cuda.synchronize()
    assert max_err(sr, y) < 1e-6, max_err(sr, y)
    assert [mod.training for mod in m.modules()] == flags


def test_session_with_crnn_prior(dev):
    from tatt_amd.crnn import parse_crnn_data, text_prior
    from tatt_amd.infer import InferenceSession
    m = build("TSRN_TL_TRANS", dev, **dict(STD, STN=False)).eval()
    crnn = build_crnn(dev)
    x, _, _ = make_inputs(8, seed=9)
    xd = x.to(dev)
    with torch.no_grad():
        p_ref = text_prior(crnn(parse_crnn_data(xd)))
        y_ref, _ = m(xd, p_ref)
    s = InferenceSession(m, prior=crnn, batch_size=8)
    sr, _, prior = s.run(xd)
    torch.cuda.synchronize()
    assert max_err(prior, p_ref) < 1e-5, max_err(prior, p_ref)
    assert max_err(sr, y_ref) < 2e-5, max_err(sr, y_ref)


# ---- evaluate_session --------------------------------------------------------------------------------------------------------------
def _eval_batches(dev, crnn, sizes=(8, 8, 5), seed=21):
    from tatt_amd.crnn import parse_crnn_data
    from tatt_amd.io import ctc_greedy_decode
    out = []
    for i, B in enumerate(sizes):
        x, tp, hr = make_inputs(B, seed=seed + i)
        hr = hr.clamp(0, 1)
        with torch.no_grad():                                             # labels the eager recogniser reads off the HR images:
            labels = ctc_greedy_decode(crnn(parse_crnn_data(hr[:, :3].contiguous().to(dev))))   # non-trivial accuracies
        labels = [l if j % 3 else l.upper() + "?" for j, l in enumerate(labels)]
        out.append((x.to(dev), hr.to(dev), tp.to(dev), labels))
    return out


def test_evaluate_session_matches_io_evaluate(dev):
    from tatt_amd.crnn import parse_crnn_data
    from tatt_amd.io import ctc_greedy_decode, evaluate, str_filt
    from tatt_amd.infer import InferenceSession, evaluate_session
    m = build("TSRN_TL_TRANS", dev, **dict(STD, STN=False)).eval()
    crnn = build_crnn(dev)
    batches = _eval_batches(dev, crnn)
    ref = evaluate(m, batches, recognizer=crnn, voc_type="all")
    got = evaluate_session(m, batches, recognizer=crnn, voc_type="all")
    print("io.evaluate", ref, "\nevaluate_session", got)
    assert got["n_batches"] == ref["n_batches"] == 3 and got["n_images"] == ref["n_images"] == 21
    for k in ("psnr", "ssim"):
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]), (k, got[k], ref[k])
    assert ref["accuracy_hr"] > 0
    # image by image: which recognitions the folded session decides differently from the eager path (a folded filter can flip an
    # arg-max that sits on a near-tie) -- every such image is reported, at most one per batch and image kind is accepted
    names = ("sr", "lr", "hr")
    flips = []
    per_batch = {}
    for bi, (x, hr, tp, labels) in enumerate(batches):
        with torch.no_grad():
            sr = m(x, tp)[0]
            eager = {nm: ctc_greedy_decode(crnn(parse_crnn_data(img[:, :3].contiguous()))) for nm, img in zip(names, (sr, x, hr))}
        s = InferenceSession(m, recognizer=crnn, batch_size=x.shape[0], accuracy_on=names, voc_type="all")
        s.run(x, hr, labels, tp)
        for nm in names:
            sess = ctc_greedy_decode(s._logits[nm])
            for j, (pe, ps, t) in enumerate(zip(eager[nm], sess, labels)):
                ok_e, ok_s = str_filt(pe, "all") == str_filt(t, "all"), str_filt(ps, "all") == str_filt(t, "all")
                if ok_e != ok_s:
                    flips.append((bi, j, nm, pe, ps, t))
                    per_batch[(bi, nm)] = per_batch.get((bi, nm), 0) + 1
    print("recognitions decided differently (batch, image, kind, eager, session, label):", flips)
    assert all(v <= 1 for v in per_batch.values()), flips
    for k, nm in (("accuracy", "sr"), ("accuracy_lr", "lr"), ("accuracy_hr", "hr")):
        n_flip = sum(1 for f in flips if f[2] == nm)
        assert abs(got[k] - ref[k]) * 21 <= n_flip + 1e-6, (k, got[k], ref[k], flips)


def test_evaluate_session_batches_never_wait_on_the_gpu(dev):
    """Once its sessions exist, evaluate_session stages every batch (label encodings included) without a synchronising copy: run
    under torch's sync debug mode 'error', the only host sync is the final read of the totals.  A reused session re-folds first."""
    from tatt_amd.infer import evaluate_session, evaluate_session_async
    m = build("TSRN_TL_TRANS", dev, **dict(STD, STN=False)).eval()
    crnn = build_crnn(dev)
    batches = _eval_batches(dev, crnn)
    sessions = {}
    first = evaluate_session(m, batches, prior=crnn, recognizer=crnn, voc_type="lower", sessions=sessions)
    assert len(sessions) == 2
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pending = evaluate_session_async(m, batches, prior=crnn, recognizer=crnn, voc_type="lower", sessions=sessions)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    second = pending.result()
    assert second == first, (first, second)


def test_session_counter_equals_host_decoding(dev):
    from tatt_amd.io import ctc_greedy_decode, str_filt
    from tatt_amd.infer import InferenceSession
    m = build("TSRN", dev, **dict(STD, STN=False)).eval()
    crnn = build_crnn(dev)
    (x, hr, _, labels), = _eval_batches(dev, crnn, sizes=(8,))
    for voc in ("lower", "all"):
        s = InferenceSession(m, recognizer=crnn, batch_size=8, accuracy_on=("sr", "lr", "hr"), voc_type=voc)
        s.run(x, hr, labels)
        for k, name in enumerate(("sr", "lr", "hr")):
            preds = ctc_greedy_decode(s._logits[name])
            want = sum(str_filt(p, voc) == str_filt(t, voc) for p, t in zip(preds, labels))
            assert int(s.correct[k]) == want, (voc, name, int(s.correct[k]), want)


# ---- session behaviour -------------------------------------------------------------------------------------------------------------
def test_session_replay_reload_and_module_state(dev):
    import tatt_amd
    from tatt_amd.infer import InferenceSession
    m = build("TSRN_TL_TRANS", dev, **dict(STD, STN=False)).train()
    crnn = build_crnn(dev).train()
    state0 = {k: v.detach().clone() for k, v in list(m.state_dict().items()) + [("crnn." + k, v) for k, v in crnn.state_dict().items()]}
    x, _, hr = make_inputs(4, seed=3)
    xd, hd = x.to(dev), hr.to(dev)
    s = InferenceSession(m, prior=crnn, recognizer=crnn, batch_size=4)
    a = [t.clone() for t in s.run(xd, hd, ["ab"] * 4)]
    b = [t.clone() for t in s.run(xd, hd, ["ab"] * 4)]
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # the modules' state is untouched
    assert m.training and crnn.training
    state1 = {k: v for k, v in list(m.state_dict().items()) + [("crnn." + k, v) for k, v in crnn.state_dict().items()]}
    for k, v in state0.items():
        assert torch.equal(v, state1[k]), k
    # new weights through load_state_dict: the next run equals a fresh session
    scaled = lambda sd: {k: (v * 0.9 if v.is_floating_point() else v) for k, v in sd.items()}
    m.load_state_dict(scaled(m.state_dict()))
    crnn.load_state_dict(scaled(crnn.state_dict()))
    c = s.run(xd, hd, ["ab"] * 4)
    d = InferenceSession(m, prior=crnn, recognizer=crnn, batch_size=4).run(xd, hd, ["ab"] * 4)
    assert all(bool(torch.isfinite(t).all()) for t in d), [bool(torch.isfinite(t).all()) for t in d]
    assert max_err(c[0], a[0]) > 1e-4
    for u, v in zip(c, d):
        assert torch.equal(u, v), max_err(u, v)
    torch.cuda.synchronize()
    tatt_amd.sync_check()


def test_session_refresh_after_raw_writes_and_recapture_after_a_move(dev):
    """A Trainer step writes the weights (Adam) and the running statistics (BatchNorm) through raw pointers: after `refresh()` the
    session equals a fresh one.  A parameter whose storage moves makes the next run re-capture: again equal to a fresh session."""
    import tatt_amd
    from tatt_amd.infer import InferenceSession
    from tatt_amd.train import Trainer
    m = build("TSRN", dev, **dict(STD, STN=False)).eval()
    x, _, hr = make_inputs(4, seed=5)
    xd, hd = x.to(dev), hr.to(dev)
    s = InferenceSession(m, batch_size=4)
    a = s.run(xd)[0].clone()
    m.train()
    tr = Trainer(m, use_graph=False)
    for _ in range(2):
        tr.step(xd, None, hd)
    torch.cuda.synchronize()
    m.eval()
    s.refresh()
    c = s.run(xd)[0].clone()
    d = InferenceSession(m, batch_size=4).run(xd)[0]
    assert max_err(c, a) > 1e-6
    assert torch.equal(c, d), max_err(c, d)
    # storage moves (a `.data =` re-home): the captured pointers are stale, the next run captures anew
    w = m.block1[0].weight
    w.data = w.data.clone() * 1.01
    e = s.run(xd)[0].clone()
    f = InferenceSession(m, batch_size=4).run(xd)[0]
    assert max_err(e, c) > 1e-6
    assert torch.equal(e, f), max_err(e, f)
    torch.cuda.synchronize()
    tatt_amd.sync_check()
