"""CTC label supervision, the parts that need no GPU: the module surface (torch.nn.CTCLoss's constructor), the C ABI declarations, the host
half of TextPriorSR.set_labels, and the refusal of CPU tensors (there is no fallback)."""
import inspect

import pytest
import torch


def test_ctc_loss_module_has_torchs_constructor():
    from tatt_amd.losses import CTCLoss
    want = inspect.signature(torch.nn.CTCLoss.__init__).parameters
    got = inspect.signature(CTCLoss.__init__).parameters
    assert list(got) == list(want)
    for k in want:
        assert got[k].default == want[k].default, k
    m = CTCLoss()
    assert (m.blank, m.reduction, m.zero_infinity) == (0, "mean", False)
    assert list(inspect.signature(CTCLoss.forward).parameters) == list(inspect.signature(torch.nn.CTCLoss.forward).parameters)
    with pytest.raises(ValueError):
        CTCLoss(reduction="batchmean")


def test_header_declares_the_ctc_entry_points():
    from tatt_amd._lib import parse_header
    protos = parse_header()
    for name in ("tatt_ctc_loss_fwd", "tatt_ctc_loss_bwd", "tatt_ctc_loss_takes"):
        assert name in protos, name
    args = [n for _, n in protos["tatt_ctc_loss_fwd"]]
    for a in ("st_t", "st_b", "st_c", "normalized", "codes", "offs", "tgt_len", "in_len", "blank", "zero_infinity", "nll", "grad"):
        assert a in args, a
    from tatt_amd.build import SOURCES
    assert "ctc.hip" in SOURCES


def test_host_half_of_set_labels():
    from tatt_amd.infer import D2A
    from tatt_amd.train import encode_label_batch
    words = ["", "a", "HeLLo", "?!-", "x" * 30, "bookkeeper", "a.b", "z" * 26]
    codes, lens, tics = encode_label_batch(words)
    assert codes.dtype == torch.int32 and lens.dtype == torch.int32 and tics.dtype == torch.float32
    assert tuple(codes.shape) == (len(words), 26) and tuple(lens.shape) == (len(words),) == tuple(tics.shape)
    assert lens.tolist() == [0, 1, 5, 0, -1, 10, 2, 26]
    assert tics.tolist() == [0.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    dec = lambda b: "".join(D2A[c] for c in codes[b, :max(int(lens[b]), 0)].tolist())
    assert [dec(b) for b in range(len(words))] == ["", "a", "hello", "", "", "bookkeeper", "ab", "z" * 26]
    assert codes[5, :10].tolist() == [12, 25, 25, 21, 21, 15, 15, 26, 15, 28]            # doubled letters stay doubled: plain word
    for b in range(len(words)):                                                          # padding / unencodable rows: -1, never a class
        assert (codes[b, max(int(lens[b]), 0):] == -1).all()
    assert int(codes.max()) <= 36 and int(codes[codes >= 0].min()) >= 1                  # the blank (0) never appears in a target


def test_text_prior_sr_without_label_weight_has_no_label_state():
    import tatt_amd
    from tatt_amd.train import TextPriorSR
    sr = tatt_amd.TSRN_TL_TRANS(scale_factor=2, width=128, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    tpg = tatt_amd.CRNN(32, 1, 37, 256)
    m = TextPriorSR(sr, tpg)
    assert m.label_weight == 0.0 and not hasattr(m, "_labels") and not hasattr(m, "_student_logits") and not hasattr(m, "_lab_dev")
    assert m.extra_loss(torch.zeros(1)) is None
    with pytest.raises(RuntimeError):
        m.set_labels(["a"])
    m = TextPriorSR(sr, tpg, None, 100, False)                       # the old positional arguments
    assert m.detach_prior is False and m.in_width == 100 and m.label_weight == 0.0
    p = inspect.signature(TextPriorSR.__init__).parameters
    assert list(p)[1:] == ["sr", "tpg", "teacher", "in_width", "detach_prior", "label_weight", "voc_type"]
    assert p["label_weight"].default == 0.0 and p["voc_type"].default == "lower"
    m = TextPriorSR(sr, tpg, label_weight=0.5)
    assert m._labels is None
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # the model lives on the CPU: nowhere to put the labels
        m.set_labels(["a"])
    with pytest.raises(ValueError):
        TextPriorSR(sr, tpg, label_weight=-1.0)


def test_cpu_tensors_are_refused():
    from tatt_amd import functional as Fh
    from tatt_amd.losses import CTCLoss, ctc_loss_from_logits
    x = torch.zeros(5, 2, 4)
    i32 = lambda *v: torch.tensor(v, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CTCLoss()(x.log_softmax(2), torch.ones(2, 2, dtype=torch.long), [5, 5], [2, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ctc_loss_from_logits(x, torch.ones(2, 2, dtype=torch.int32), i32(2, 2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Fh.CtcLossFn.apply(x, i32(1, 1, 1, 1), i32(0, 2), i32(2, 2), None, 0, False, False)
    assert "ctc_loss" in __import__("tatt_amd.torch_ops", fromlist=["OPS"]).OPS and hasattr(torch.ops.tatt_hip, "ctc_loss")
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.tatt_hip.ctc_loss(x, i32(1, 1, 1, 1), i32(0, 2), i32(2, 2), None, 0, False, False)
