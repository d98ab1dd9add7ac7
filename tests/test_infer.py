"""Inference session (tatt_amd.infer): the parts that need no GPU -- C ABI of the eval-only kernels, refusal of CPU modules and
tensors, and the host-side label encoding / keep mask against the reference's string filter."""
import ctypes
import random
import string

import pytest
import torch

NEW_SYMBOLS = ("tatt_lstm_fwd_chain", "tatt_lstm_chain_capacity", "tatt_bn_fold", "tatt_ctc_greedy_match")
VOC_TYPES = ("digit", "lower", "upper", "all")


def test_new_symbols_declared_and_exported():
    from tatt_amd._lib import LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, name
        assert hasattr(dll, name), name
    assert [n for _, n in protos["tatt_lstm_fwd_chain"]][-5:] == ["sync", "T", "Bt", "H", "st"]


def test_session_refuses_cpu_modules_and_tensors():
    import tatt_amd
    from tatt_amd.infer import InferenceSession, bilstm_eval, ctc_greedy_match, bn_fold
    torch.manual_seed(0)
    g = tatt_amd.TSRN(scale_factor=2, width=128, height=32, STN=False, srb_nums=1, mask=True, hidden_units=32)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        InferenceSession(g, batch_size=2)
    crnn = tatt_amd.CRNN(32, 1, 37, 256)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        InferenceSession(g, prior=crnn, recognizer=crnn, batch_size=2)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        ctc_greedy_match(torch.zeros(26, 2, 37), torch.ones(37, dtype=torch.int32), torch.zeros(2, 26, dtype=torch.int32),
                         torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="AMD GPU"):
        bn_fold(crnn.cnn.conv2.weight, crnn.cnn.conv2.bias, crnn.cnn.batchnorm2)
    with pytest.raises(RuntimeError, match="AMD GPU"):
        bilstm_eval(torch.zeros(3, 2, 512), crnn.rnn[0].rnn)


def test_keep_mask_matches_str_filt():
    from tatt_amd.infer import keep_mask, D2A
    from tatt_amd.io import str_filt
    for voc in VOC_TYPES:
        k = keep_mask(voc)
        assert len(k) == 37 and k[0] == 0
        for c in range(1, 37):
            assert k[c] == (1 if str_filt(D2A[c], voc) == D2A[c] else 0), (voc, c)
    assert sum(keep_mask("digit")) == 10 and sum(keep_mask("lower")) == 36


def _random_labels(n, seed):
    rnd = random.Random(seed)
    pool = string.digits + string.ascii_letters + string.punctuation + " "
    out = ["", "-", "ABC", "abc", "a.b", "x" * 26, "y" * 27, "Hello", "0123"]
    while len(out) < n:
        out.append("".join(rnd.choice(pool) for _ in range(rnd.randint(0, 12))))
    return out


@pytest.mark.parametrize("voc", VOC_TYPES)
def test_label_encoder_matches_str_filt(voc):
    """A label encodes to the class sequence of str_filt(label) when a greedy decoding could ever produce it, else to length -1."""
    from tatt_amd.infer import encode_labels, D2A, CTC_T
    from tatt_amd.io import ALPHABET, str_filt
    labels = _random_labels(300, 11)
    codes, lens = encode_labels(labels, voc)
    assert len(codes) == len(lens) == len(labels)
    for lab, c, n in zip(labels, codes, lens):
        want = str_filt(lab, voc)
        assert len(c) == CTC_T
        possible = len(want) <= CTC_T and all(ch in ALPHABET for ch in want)
        if possible:
            assert n == len(want)
            assert "".join(D2A[i] for i in c[:n]) == want
            assert all(i == -1 for i in c[n:])
        else:
            assert n == -1 and all(i == -1 for i in c)
    # empty labels (after filtering) encode to length 0: they match an empty decoding
    assert encode_labels([""], voc)[1] == [0]
