"""Full eval metrics on the GPU: tatt_ctc_greedy_score against its numpy restatement (exact integers) and the match kernel,
tatt_bicubic_resize against torch's CPU float32 operator, and the session / evaluate_session / io.evaluate paths with
full_metrics=True against host values computed from the session's own logits."""
import pytest
import torch
import torch.nn.functional as F

from oracle.fixtures import make_inputs, randomize_state_dict
from tests.greedy_score_ref import greedy_score_ref
from tests.test_eval_metrics import VOC_TYPES, _ctc_logits, score_labels
from tests.util import max_err

pytestmark = pytest.mark.gpu
KINDS = ("sr", "lr", "hr")
BASE_KEYS = {"psnr", "ssim", "n_batches", "accuracy", "accuracy_lr", "accuracy_hr", "n_images"}
FULL_KEYS = BASE_KEYS | {"psnr_lr", "ssim_lr", "ned", "ned_lr", "ned_hr", "ned_skipped"}


# ---- tatt_ctc_greedy_score -----------------------------------------------------------------------------------------------------------
def _score(dev, x, voc, labels, strided=False):
    """-> (record (B, T + 3), counter, stats) of the score launch and (correct, dec, dlen, counter) of the match launch, on the host"""
    from tatt_amd.infer import HIST, ctc_greedy_match, ctc_greedy_score, encode_labels, encode_labels_full, keep_mask
    T, B, C = x.shape
    keep = torch.tensor(keep_mask(voc), dtype=torch.int32, device=dev)
    codes, lens = encode_labels_full(labels, voc)
    lab = torch.tensor(codes, dtype=torch.int32, device=dev)
    ln = torch.tensor(lens, dtype=torch.int32, device=dev)
    xd = x.to(dev)
    if strided:                                                           # B-major memory behind the (T, B, C) view
        xd = xd.permute(1, 0, 2).contiguous().permute(1, 0, 2)
        assert not xd.is_contiguous()
    counter = torch.zeros(1, dtype=torch.int32, device=dev)
    stats = torch.zeros(HIST + 2, dtype=torch.int32, device=dev)
    rec = ctc_greedy_score(xd, keep, lab, ln, counter, stats)
    c26, l26 = encode_labels(labels, voc, T)
    counter_m = torch.zeros(1, dtype=torch.int32, device=dev)
    match = ctc_greedy_match(xd, keep, torch.tensor(c26, dtype=torch.int32, device=dev),
                             torch.tensor(l26, dtype=torch.int32, device=dev), counter_m, want_decoded=True)
    ref = greedy_score_ref(x.numpy(), keep_mask(voc), codes, lens)
    return rec.cpu(), int(counter), stats.cpu(), [t.cpu() for t in match], int(counter_m), ref


def _check_score(rec, counter, stats, match, counter_m, ref, T):
    assert rec[:, :T].tolist() == ref["dec"].tolist()
    assert rec[:, T].tolist() == ref["dec_len"].tolist()
    assert rec[:, T + 1].tolist() == ref["correct"].tolist()
    assert rec[:, T + 2].tolist() == ref["dist"].tolist()
    assert counter == ref["counter"]
    assert stats[:65].tolist() == ref["hist"].tolist() and int(stats[0]) == 0
    assert int(stats[65]) == ref["scored"] and int(stats[66]) == ref["skipped"]
    assert int(stats[65]) + int(stats[66]) == rec.shape[0]
    # what the match kernel gives on the same inputs
    correct, dec, dlen = match
    assert torch.equal(rec[:, T + 1], correct) and counter == counter_m
    assert torch.equal(rec[:, :T], dec) and torch.equal(rec[:, T], dlen)


@pytest.mark.parametrize("voc", VOC_TYPES)
def test_greedy_score_against_restatement(dev, voc):
    from tatt_amd.io import ctc_greedy_decode
    x = _ctc_logits(seed=len(voc))
    x[5, 41, 7] = float("nan")                                            # a NaN wins its step
    labels = score_labels(ctc_greedy_decode(x), seed=len(voc))
    out = _score(dev, x, voc, labels)
    _check_score(*out, T=26)
    assert int(out[2][66]) == sum(t == "1" * 65 for t in labels) == 8     # skipped: the 65-character labels, nothing else
    assert out[1] > 0 and int(out[2][:65].sum()) > 0
    strided = _score(dev, x, voc, labels, strided=True)
    assert torch.equal(strided[0], out[0]) and torch.equal(strided[2], out[2]) and strided[1] == out[1]


@pytest.mark.parametrize("voc", VOC_TYPES)
def test_greedy_score_crafted_rows(dev, voc):
    """B = 1: decoded lengths 0 and 26 (26 distinct consecutive classes) against label lengths 0, 1, 26, 27, 64, 65 and a label of
    foreign characters only."""
    from tatt_amd.infer import D2A
    from tatt_amd.io import edit_distance, str_filt
    T, C = 26, 37
    empty = torch.zeros(T, 1, C)
    empty[:, 0, 0] = 1.0
    full = torch.zeros(T, 1, C)
    for t in range(T):
        full[t, 0, t + 1] = 1.0
    word = D2A[1:27]
    labels = ["", "5", word, word + "q", word[:13] + "zz", "5" * 26, "5" * 27, (word + "012345")[::-1] * 2, "5" * 64, "5" * 65,
              "ABC!?", "!?#" * 21 + "!", word.upper()]
    assert [len(l) for l in labels[:4]] == [0, 1, 26, 27] and len(labels[7]) == 64
    for x, pred in ((empty, ""), (full, word)):
        for lab in labels:
            rec, counter, stats, match, counter_m, ref = out = _score(dev, x, voc, [lab])
            _check_score(*out, T=T)
            p, t = str_filt(pred, voc), str_filt(lab, voc)
            want = -1 if len(t) > 64 else edit_distance(p, t)
            assert int(rec[0, T + 2]) == want, (voc, pred, lab)
            assert int(rec[0, T]) == len(p) and int(stats[66]) == int(len(t) > 64)
            if want > 0:
                assert int(stats[max(len(p), len(t))]) == want and int(stats[:65].sum()) == want


def test_greedy_score_refusals(dev):
    from tatt_amd import ops
    from tatt_amd._lib import LIB
    z = torch.zeros(8, dtype=torch.int32, device=dev)
    x = torch.zeros(4, device=dev)
    args = lambda T, B, C, hist: (ops.P(x), 1, 1, 1, T, B, C, ops.P(z), ops.P(z), ops.P(z), None, None, None, None, None, T, 1,
                                  hist, None, None, ops.stream())
    assert LIB.tatt_ctc_greedy_score(*args(257, 1, 37, None)) == 1
    assert LIB.tatt_ctc_greedy_score(*args(26, 1, 65, None)) == 1
    assert LIB.tatt_ctc_greedy_score(*args(26, 0, 37, None)) == 1
    assert LIB.tatt_ctc_greedy_score(*args(65, 1, 37, ops.P(z))) == 1      # max(n, m) could leave the 65 bins


# ---- tatt_bicubic_resize -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,size", [((1, 3, 16, 64), (32, 128)), ((2, 4, 5, 7), (3, 11)), ((1, 1, 1, 1), (4, 4)),
                                        ((1, 3, 7, 1), (3, 5)), ((2, 3, 16, 64), (32, 100))])
def test_bicubic_resize_against_torch_cpu(dev, shape, size):
    from tatt_amd.crnn import bicubic_resize
    x = torch.rand(shape, generator=torch.Generator().manual_seed(sum(shape) + size[1]))
    ref = F.interpolate(x, size, mode="bicubic")                          # ATen's CPU float32 operator: what the reference runs
    got = bicubic_resize(x.to(dev), size)
    assert got.shape == ref.shape and got.is_contiguous()
    err = max_err(got, ref)
    print("bicubic_resize", shape, size, "max abs err %.3e" % err)
    assert err <= 5e-6, err
    # a channels-last input, and an output with channels-last strides, give the same planes
    xc = x.to(dev).contiguous(memory_format=torch.channels_last)
    assert torch.equal(bicubic_resize(xc, size), got)
    out = torch.empty(got.shape, device=dev).contiguous(memory_format=torch.channels_last)
    assert bicubic_resize(x.to(dev), size, out=out) is out and torch.equal(out, got)


def test_bicubic_resize_views_identity_and_refusals(dev):
    from tatt_amd import ops
    from tatt_amd._lib import LIB
    from tatt_amd.crnn import bicubic_resize
    x = torch.rand(2, 4, 16, 64, generator=torch.Generator().manual_seed(1)).to(dev)
    # equal sizes: the input, bit for bit
    assert torch.equal(bicubic_resize(x, (16, 64)), x)
    # x[:, :3] of a 4-channel tensor, read as it is
    v = x[:, :3]
    assert not v.is_contiguous()
    assert torch.equal(bicubic_resize(v, (32, 128)), bicubic_resize(v.contiguous(), (32, 128)))
    assert torch.equal(bicubic_resize(v, (32, 128)), bicubic_resize(x, (32, 128))[:, :3])
    with pytest.raises(RuntimeError, match="require grad"):
        bicubic_resize(x.clone().requires_grad_(True), (32, 128))
    o = torch.zeros(16, device=dev)
    for bad in [(0, 3, 4, 4, 8, 8), (1, 3, 4, 4, 0, 8), (1, 3, 4, 4, 8, -1), (1, 0, 4, 4, 8, 8)]:
        assert LIB.tatt_bicubic_resize(ops.P(x), 1, 1, 1, 1, ops.P(o), 1, 1, 1, 1, *bad, ops.stream()) == 1


# ---- the session and the evaluation loops --------------------------------------------------------------------------------------------
def _models(dev):
    import tatt_amd
    torch.manual_seed(1234)
    m = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=1, hidden_units=32)
    m.load_state_dict(randomize_state_dict(m.state_dict()))
    torch.manual_seed(5)
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=5))
    return m.to(dev).eval(), c.to(dev).eval()


def _eval_batches(dev, crnn, sizes=(2, 2, 1), seed=21):                     # (labels as in tests/test_infer_gpu.py)
    from tatt_amd.crnn import parse_crnn_data
    from tatt_amd.io import ctc_greedy_decode
    out = []
    for i, B in enumerate(sizes):
        x, tp, hr = make_inputs(B, seed=seed + i)
        hr = hr.clamp(0, 1)
        with torch.no_grad():
            labels = ctc_greedy_decode(crnn(parse_crnn_data(hr[:, :3].contiguous().to(dev))))
        labels = [l if j % 3 else l.upper() + "?" for j, l in enumerate(labels)]
        out.append((x.to(dev), hr.to(dev), None, labels))
    return out


@pytest.fixture(scope="module")
def ctx(dev):
    """Models, three batches (B = 2, 2 and a tail of 1), and ONE full-metrics evaluation shared by the tests below, together with
    the host values: per batch the session's own logits decoded with ctc_greedy_decode and scored with edit_distance."""
    from tatt_amd.infer import InferenceSession, evaluate_session_async
    from tatt_amd.io import ctc_greedy_decode, edit_distance, str_filt
    m, crnn = _models(dev)
    batches = _eval_batches(dev, crnn)
    sessions = {}
    pending = evaluate_session_async(m, batches, recognizer=crnn, voc_type="all", sessions=sessions, full_metrics=True)
    got = pending.result()
    # host values, through two sessions driven by hand (B = 2 replayed for two different batches, and the tail)
    own = {B: InferenceSession(m, recognizer=crnn, batch_size=B, accuracy_on=KINDS, voc_type="all", full_metrics=True) for B in (2, 1)}
    rows, device_rows = [], []
    for x, hr, _, labels in batches:
        s = own[x.shape[0]]
        s.run(x, hr, labels)
        device_rows.append(s.records.clone())
        dec = {k: [str_filt(p, "all") for p in ctc_greedy_decode(s._logits[k])] for k in KINDS}
        for j, lab in enumerate(labels):
            t = str_filt(lab, "all")
            row = {"label": lab}
            for k in KINDS:
                row[k] = dec[k][j]
                row[k + "_correct"] = dec[k][j] == t
                row[k + "_dist"] = edit_distance(dec[k][j], t)
                row[k + "_ned"] = row[k + "_dist"] / (max(len(dec[k][j]), len(t)) + 1e-10)
            rows.append(row)
    return dict(m=m, crnn=crnn, batches=batches, sessions=sessions, pending=pending, got=got, rows=rows, device_rows=device_rows)


def test_session_full_metrics_against_host_values(dev, ctx):
    from tatt_amd.crnn import bicubic_resize
    from tatt_amd.infer import evaluate_session
    from tatt_amd.losses import SSIM
    from tatt_amd.train import calculate_psnr
    got, rows, batches = ctx["got"], ctx["rows"], ctx["batches"]
    assert set(got) == FULL_KEYS and len(ctx["sessions"]) == 2
    assert got["n_batches"] == 3 and got["n_images"] == 5 and got["ned_skipped"] == 0
    # the bicubic baseline, composed eagerly
    with torch.no_grad():
        psnr = sum(float(calculate_psnr(bicubic_resize(x[:, :3], hr.shape[-2:]), hr[:, :3])) for x, hr, _, _ in batches) / 3
        ssim = sum(float(SSIM()(bicubic_resize(x[:, :3], hr.shape[-2:]), hr[:, :3])) for x, hr, _, _ in batches) / 3
    print("psnr_lr", got["psnr_lr"], psnr, "ssim_lr", got["ssim_lr"], ssim)
    assert abs(got["psnr_lr"] - psnr) <= 1e-5 * abs(psnr) and abs(got["ssim_lr"] - ssim) <= 1e-5 * abs(ssim)
    assert got["psnr_lr"] > 0 and got["psnr_lr"] != got["psnr"]
    # edit distances and records: exact, the host values come from the same logits
    for key, k in (("ned", "sr"), ("ned_lr", "lr"), ("ned_hr", "hr")):
        want = sum(r[k + "_ned"] for r in rows) / (5 + 1e-10)
        assert abs(got[key] - want) <= 1e-12, (key, got[key], want)
    assert min(got["ned"], got["ned_lr"], got["ned_hr"]) > 0            # every third label ends in a foreign character
    recs = ctx["pending"].records()
    assert len(recs) == 5
    for r, want in zip(recs, rows):
        assert r == {k: v for k, v in want.items() if not k.endswith("_ned")}, (r, want)
    # the accuracies are those of the same batches without the keyword
    base = evaluate_session(ctx["m"], batches, recognizer=ctx["crnn"], voc_type="all")
    assert set(base) == BASE_KEYS                                         # default off: the keys of before
    for k in BASE_KEYS:
        assert base[k] == got[k], k
    for key, k in (("accuracy", "sr"), ("accuracy_lr", "lr"), ("accuracy_hr", "hr")):
        assert got[key] == round(sum(r[k + "_correct"] for r in rows) / 5, 4)


def test_records_survive_the_next_replay(dev, ctx):
    """Two consecutive batches with different images and labels through ONE session (B = 2): each keeps its own record, neither
    returns the other's.  The labels are built so that the two batches' distances must differ whatever the recogniser reads."""
    from tatt_amd.infer import D2A, evaluate_session_async
    from tatt_amd.io import edit_distance, str_filt
    (x0, h0, _, l0), (x1, h1, _, l1) = ctx["batches"][:2]
    assert not torch.equal(x0, x1)
    la, lb = ["0" + l0[0], l0[1] + "zz9"], ["", "Q" * 30]                   # at most 29 characters against 30 foreign ones
    pending = evaluate_session_async(ctx["m"], [(x0, h0, None, la), (x1, h1, None, lb)], recognizer=ctx["crnn"], voc_type="all",
                                     sessions=ctx["sessions"], full_metrics=True)
    assert len(ctx["sessions"]) == 2
    pending.result()
    recs, rows = pending.records(), ctx["rows"]
    assert [r["label"] for r in recs] == la + lb
    for r, own in zip(recs, rows[:4]):
        t = str_filt(r["label"], "all")
        for k in KINDS:
            assert r[k] == own[k]                                         # the decoding of the batch's own images
            assert r[k + "_dist"] == edit_distance(r[k], t) and r[k + "_correct"] == (r[k] == t)
    assert all(r[k + "_dist"] == 30 for r in recs[3:] for k in KINDS) and all(r[k + "_dist"] < 30 for r in recs[:2] for k in KINDS)
    assert all(r[k + "_dist"] == len(r[k]) for r in recs[2:3] for k in KINDS)
    # the record tensors of the sessions driven by hand: batch 0 and batch 1 through the same B = 2 session
    for t, base in ((ctx["device_rows"][0].cpu(), 0), (ctx["device_rows"][1].cpu(), 2)):
        for k, name in enumerate(KINDS):
            for j in range(2):
                n = int(t[k, j, 26])
                assert "".join(D2A[c] for c in t[k, j, :n].tolist()) == rows[base + j][name]
                assert int(t[k, j, 28]) == rows[base + j][name + "_dist"]


def test_session_scores_only_the_kinds_asked_for(dev, ctx):
    """accuracy_on=("lr",): one score launch; the SR and HR rows of the record, the histograms and the counters stay untouched."""
    from tatt_amd.infer import HIST, InferenceSession
    x, hr, _, labels = ctx["batches"][0]
    s = InferenceSession(ctx["m"], recognizer=ctx["crnn"], batch_size=2, accuracy_on=("lr",), voc_type="all", full_metrics=True)
    for _ in range(2):                                                    # the eager capture run must not count twice
        s.reset_metrics()
        s.run(x, hr, labels)
    rec, stats, correct = s.records.cpu(), s.ned_stats.cpu(), s.correct.cpu()
    assert bool((rec[0] == -1).all()) and bool((rec[2] == -1).all())
    assert stats[0].tolist() == [0] * (HIST + 2) == stats[2].tolist()
    assert int(stats[1, HIST]) == 2 and int(stats[1, HIST + 1]) == 0
    want = ctx["rows"][:2]
    assert rec[1, :, 28].tolist() == [r["lr_dist"] for r in want]
    assert int(stats[1, :HIST].sum()) == sum(r["lr_dist"] for r in want)
    assert correct.tolist() == [0, sum(r["lr_correct"] for r in want), 0]
    assert float(s.psnr_lr_sum) > 0
    s.reset_metrics()
    assert int(s.ned_stats.abs().sum()) == 0 and float(s.psnr_lr_sum) == 0 and float(s.ssim_lr_sum) == 0


def test_full_metrics_batches_never_wait_on_the_gpu(dev, ctx):
    from tatt_amd.infer import evaluate_session_async
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pending = evaluate_session_async(ctx["m"], ctx["batches"], recognizer=ctx["crnn"], voc_type="all", sessions=ctx["sessions"],
                                         full_metrics=True)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert len(ctx["sessions"]) == 2
    assert pending.result() == ctx["got"]
    assert pending.records() == ctx["pending"].records()


def test_io_evaluate_full_metrics_against_session(dev, ctx):
    from tatt_amd.crnn import parse_crnn_data
    from tatt_amd.io import ctc_greedy_decode, evaluate, str_filt
    m, crnn, batches, got = ctx["m"], ctx["crnn"], ctx["batches"], ctx["got"]
    ref = evaluate(m, batches, recognizer=crnn, voc_type="all", full_metrics=True)
    print("io.evaluate", ref, "\nevaluate_session", got)
    assert set(ref) == FULL_KEYS and ref["ned_skipped"] == 0
    assert set(evaluate(m, batches[:1], recognizer=crnn, voc_type="all")) == BASE_KEYS
    for k in ("psnr", "ssim", "psnr_lr", "ssim_lr"):
        assert abs(got[k] - ref[k]) <= 1e-5 * abs(ref[k]), (k, got[k], ref[k])
    # image by image: a decoding the folded session reads differently from the eager path moves a mean by at most 1 / n_images
    flips = {k: 0 for k in KINDS}
    i = 0
    for x, hr, _, labels in batches:
        with torch.no_grad():
            sr = m(x)
            sr = sr[0] if isinstance(sr, tuple) else sr
            eager = {k: ctc_greedy_decode(crnn(parse_crnn_data(img[:, :3].contiguous()))) for k, img in zip(KINDS, (sr, x, hr))}
        for j in range(len(labels)):
            for k in KINDS:
                flips[k] += str_filt(eager[k][j], "all") != ctx["rows"][i][k]
            i += 1
    print("decodings read differently:", flips)
    for key, k in (("ned", "sr"), ("ned_lr", "lr"), ("ned_hr", "hr")):
        assert abs(got[key] - ref[key]) <= flips[k] / 5 + 1e-12, (key, got[key], ref[key], flips)
