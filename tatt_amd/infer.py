"""Graph-captured inference: the reference's eval / test loop (interfaces/super_resolution.py:1203-1700, `model_inference` for `tatt`:
CRNN prior on LR -> generator in eval mode -> recogniser on SR / LR / HR, PSNR and SSIM) as ONE replayed hipGraph per batch size.

`InferenceSession` runs an eval-only forward of its own:
  * eval BatchNorm is folded into the preceding convolution on the device (tatt_bn_fold): residual blocks' conv1 + bn1 (mish in the
    convolution's epilogue), conv2 + bn2, block 7, the CRNN's conv2 / 4 / 6 + BatchNorm (ReLU epilogue).  The folded filters are
    tensors the session owns, packed through the ordinary `ops.PACKED` cache;
  * each CRNN BiLSTM layer is one launch (tatt_lstm_fwd_chain: W_hh resident per work-group, no cell / gate saves) instead of T;
  * everything runs under `torch.no_grad()`, so no operator keeps anything for a backward (GruBlocks take their save=False path);
  * greedy CTC decoding and the label comparison run on the device (tatt_ctc_greedy_match): no host wait inside a batch.
TBSRN generators are captured as they are (their own eval forward, no folding).
The operators between those (GruBlocks, TP interpreter, convolutions, activations) are the generators' own helpers, i.e. the autograd
Functions of `functional`, called under `no_grad`: their `needs_input_grad` is all False, so they save nothing and the GruBlocks
take their save=False path, and inside the replayed graph the Function layer costs no GPU time.

`evaluate_session` is the drop-in for `tatt_amd.io.evaluate` built on it: every accumulator lives on the device, one host sync at
the end.  Neither changes the modules' state (training flags, parameters, running statistics, `num_batches_tracked`).

`SuperResolver` is the reference's `demo()` (interfaces/super_resolution.py:1788-1876) with an output: PIL crops in, PIL images out, through
`io.DeviceCollator.stack` -> a session -> `io.DeviceExporter` per batch; the host waits only when the result is read.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence

import torch

from . import functional as Fh
from . import ops
from ._lib import LIB
from .ops import ACT_MISH, ACT_RELU, ACT_TANH
from .io import ALPHABET, LABEL_CAP, str_filt

# A/B hook: False -> the CRNN's LSTM layers run the per-step kernels (tatt_lstm_fwd_step) inside the session as well
LSTM_CHAIN = True
LABEL_RING = 4           # pinned host slots the label encoding of consecutive batches rotates through
CTC_T = 26               # steps of the recogniser's output for its 100-pixel input (parse_crnn_data): W / 4 + 1
D2A = "-" + ALPHABET     # class c -> character (class 0 is the CTC blank)
LABEL_FOREIGN = 64       # the one code of every kept label character outside ALPHABET: it equals no class (C <= 64)
KINDS = ("sr", "lr", "hr")
HIST = LABEL_CAP + 1     # bins of the edit-distance histogram, indexed by max(len(pred), len(label))


# ---- host-side label plumbing ---------------------------------------------------------------------------------------------------
def keep_mask(voc_type: str = "lower") -> list:
    """37 entries: 1 where `str_filt` keeps the class's character (the blank is never kept)."""
    return [0] + [1 if str_filt(ch, voc_type) == ch else 0 for ch in ALPHABET]


def encode_labels(labels: Sequence[str], voc_type: str = "lower", T: int = CTC_T):
    """-> (codes: B lists of T class indices padded with -1, lengths: B ints).  A label is filtered with `str_filt` first; one that holds
    a character outside ALPHABET (upper case under 'upper', punctuation under 'all') or more than T characters can never equal a
    greedy decoding and gets length -1."""
    a2d = {ch: i for i, ch in enumerate(D2A)}
    codes, lens = [], []
    for lab in labels:
        s = str_filt(lab, voc_type)
        ids = [a2d.get(ch, -1) for ch in s]
        if len(ids) > T or any(i <= 0 for i in ids):
            codes.append([-1] * T)
            lens.append(-1)
        else:
            codes.append(ids + [-1] * (T - len(ids)))
            lens.append(len(ids))
    return codes, lens


def encode_labels_full(labels: Sequence[str], voc_type: str = "lower", cap: int = LABEL_CAP):
    """The encoding tatt_ctc_greedy_score reads -> (codes: B lists of `cap` ints padded with -1, lengths: B ints).  The characters of
    `str_filt(label, voc_type)` in ALPHABET map to their classes 1..36, every other kept character (upper case under 'upper',
    punctuation under 'all') to the ONE code LABEL_FOREIGN: a decoding holds alphabet classes only, so a foreign character mismatches
    whatever it meets and the edit distance is exact.  A filtered label longer than `cap` gets length -1 (not scored)."""
    a2d = {ch: i for i, ch in enumerate(D2A)}
    codes, lens = [], []
    for lab in labels:
        s = str_filt(lab, voc_type)
        if len(s) > cap:
            codes.append([-1] * cap)
            lens.append(-1)
        else:
            ids = [a2d[ch] if a2d.get(ch, 0) > 0 else LABEL_FOREIGN for ch in s]
            codes.append(ids + [-1] * (cap - len(ids)))
            lens.append(len(ids))
    return codes, lens


# ---- device entry points --------------------------------------------------------------------------------------------------------
def bn_fold(weight, bias, bn, w_out=None, b_out=None):
    """Eval BatchNorm `bn` folded into the convolution (weight, bias) -> (w_out, b_out), computed by tatt_bn_fold."""
    ops._check_dev(weight)
    Cout = weight.shape[0]
    w_out = torch.empty_like(weight, memory_format=torch.contiguous_format) if w_out is None else w_out
    b_out = ops.new(weight, Cout) if b_out is None else b_out
    gamma = bn.weight if bn.affine else torch.ones(Cout, device=weight.device)
    beta = bn.bias if bn.affine else torch.zeros(Cout, device=weight.device)
    ops.call("tatt_bn_fold", ops.P(weight.contiguous()), ops.P(bias), ops.P(gamma), ops.P(beta), ops.P(bn.running_mean),
             ops.P(bn.running_var), float(bn.eps), ops.P(w_out), ops.P(b_out), Cout, weight.numel() // Cout, ops.stream())
    return w_out, b_out


def ctc_greedy_match(logits, keep, label, label_len, counter=None, want_decoded=False):
    """logits (T, B, C) on the GPU; keep (C,) / label (B, T) / label_len (B,) int32 device tensors -> correct (B,) int32
    [, decoded (B, T) int32 padded with -1, lengths (B,)].  `counter` (int32 device scalar): += number of correct images."""
    ops._check_dev(logits)
    T, B, C = logits.shape
    correct = torch.empty(B, dtype=torch.int32, device=logits.device)
    dec = torch.empty(B, T, dtype=torch.int32, device=logits.device) if want_decoded else None
    dlen = torch.empty(B, dtype=torch.int32, device=logits.device) if want_decoded else None
    ops.call("tatt_ctc_greedy_match", ops.P(logits), *logits.stride(), T, B, C, ops.P(keep), ops.P(label), ops.P(label_len),
             ops.P(correct), ops.P(counter), ops.P(dec), ops.P(dlen), ops.stream())
    return (correct, dec, dlen) if want_decoded else correct


def ctc_greedy_score(logits, keep, label, label_len, counter=None, stats=None, record=None):
    """`ctc_greedy_match` plus the edit distance, one launch (tatt_ctc_greedy_score).  logits (T, B, C) on the GPU; keep (C,), label
    (B, LABEL_CAP) and label_len (B,) int32 device tensors from `encode_labels_full` -> record (B, T + 3) int32:
    decoded classes padded with -1 | decoded length | correct 0/1 | distance (-1 for a label of length -1).
    `counter`: += correct images; `stats` (HIST + 2,) int32: [max(len(pred), len(label))] += distance | scored += 1 | skipped += 1
    (see `ned_from_stats`); `record`: the (B, T + 3) int32 tensor to write into."""
    ops._check_dev(logits)
    T, B, C = logits.shape
    if tuple(label.shape) != (B, LABEL_CAP) or not label.is_contiguous():
        raise ValueError("label must be a contiguous (%d, %d) int32 tensor, got %s" % (B, LABEL_CAP, tuple(label.shape)))
    if record is None:
        record = torch.empty(B, T + 3, dtype=torch.int32, device=logits.device)
    elif tuple(record.shape) != (B, T + 3) or record.dtype != torch.int32 or not record.is_contiguous():
        raise ValueError("record must be a contiguous (%d, %d) int32 tensor" % (B, T + 3))
    if stats is not None and (stats.numel() != HIST + 2 or stats.dtype != torch.int32 or not stats.is_contiguous()):
        raise ValueError("stats must be a contiguous (%d,) int32 tensor" % (HIST + 2))
    col = lambda k: ops.P(record[:, T + k])
    hist, scored, skipped = (None,) * 3 if stats is None else (ops.P(stats), ops.P(stats[HIST:]), ops.P(stats[HIST + 1:]))
    ops.call("tatt_ctc_greedy_score", ops.P(logits), *logits.stride(), T, B, C, ops.P(keep), ops.P(label), ops.P(label_len),
             col(1), ops.P(counter), ops.P(record), col(0), col(2), T + 3, T + 3, hist, scored, skipped, ops.stream())
    return record


def ned_from_stats(stats) -> float:
    """Mean of distance / (max(len(pred), len(label)) + 1e-10) over the scored images (reference
    interfaces/super_resolution.py:1531-1556,1633-1635) from the integers of one `stats` row (host values): bins | scored | skipped,
    with as many bins as the row has (HIST = 65 from tatt_ctc_greedy_score, max(L, 64) + 1 from tatt_ids_score)."""
    vals = [int(v) for v in stats]
    bins = len(vals) - 2
    return sum(vals[M] / (M + 1e-10) for M in range(1, bins)) / (vals[bins] + 1e-10)


def lstm_chain_capacity(device=None) -> int:
    return Fh.sync_capacity(device)[6]


def _lstm_sync(ref):
    return Fh._sync_register(torch.zeros(1024, dtype=torch.int32, device=ref.device), Fh.SYNC_LSTM)


def lstm_input_projection(x, rnn):
    """gi (T * B, 8H) = x W_ih^T + b_ih of both directions ([forward | reverse] x gates), the operand of the recurrence kernels."""
    T, B, I = x.shape
    H = rnn.weight_hh_l0.shape[1]
    x2 = Fh._c(x).reshape(T * B, I)
    gi = ops.new(x, T * B, 8 * H)
    ops.linear_fwd(x2, rnn.weight_ih_l0, rnn.bias_ih_l0, out=gi[:, :4 * H])
    ops.linear_fwd(x2, rnn.weight_ih_l0_reverse, rnn.bias_ih_l0_reverse, out=gi[:, 4 * H:])
    return gi


def bilstm_eval(x, rnn, sync=None, chain=None):
    """nn.LSTM(I, H, bidirectional=True) holder on a time-major (T, B, I) sequence, forward only -> (T, B, 2H).  The input projection
    is the GEMM BiLSTMFn uses; the recurrence is ONE tatt_lstm_fwd_chain launch where it takes the geometry, else the per-step kernels
    (with scratch for what they save).  `sync`: the chain's 1024-word workspace (allocated here when None)."""
    chain = LSTM_CHAIN if chain is None else chain
    T, B, I = x.shape
    H = rnn.weight_hh_l0.shape[1]
    gi = lstm_input_projection(x, rnn)
    out = ops.new(x, T, B, 2 * H)
    whh_f, whh_r, bhh_f, bhh_r = rnn.weight_hh_l0, rnn.weight_hh_l0_reverse, rnn.bias_hh_l0, rnn.bias_hh_l0_reverse
    if chain:
        if sync is None:
            sync = _lstm_sync(x)
        rc = getattr(LIB, "tatt_lstm_fwd_chain")(ops.P(gi), ops.P(whh_f), ops.P(whh_r), ops.P(bhh_f), ops.P(bhh_r), ops.P(out),
                                                 ops.P(sync), T, B, H, ops.stream())
        if rc == 0:
            return out
        if rc != 1:
            raise RuntimeError("tatt_lstm_fwd_chain failed with code %d" % rc)
    cseq, gsave = ops.new(x, 2, T, B, H), ops.new(x, 2, T, B, 4, H)
    for s in range(T):
        ops.call("tatt_lstm_fwd_step", ops.P(gi), ops.P(whh_f), ops.P(whh_r), ops.P(bhh_f), ops.P(bhh_r), ops.P(out), ops.P(cseq),
                 ops.P(gsave), T, B, H, s, ops.stream())
    return out


# ---- the session ------------------------------------------------------------------------------------------------------------------
class _Fold:
    """conv (weight, bias) + eval BatchNorm -> a folded filter the session owns (refolded in place when the sources change)."""

    def __init__(self, conv, bn):
        self.conv, self.bn = conv, bn
        w = conv.weight
        self.w = torch.empty(w.shape, device=w.device, dtype=torch.float32)
        self.b = ops.new(w, w.shape[0])
        self.run()

    def run(self):
        bn_fold(self.conv.weight, self.conv.bias, self.bn, self.w, self.b)


def _refuse_attention_recognizer(m, who):
    from .aster import ASTER
    from .moran import MORAN
    if isinstance(m, (ASTER, MORAN)):
        raise TypeError("%s: %s recogniser is not captured into a session (its attention decoder, and MORAN's rectifier, are not "
                        "graph-captured); evaluate with tatt_amd.io.evaluate(model, batches, recognizer=<%s>), which reads SR / LR / HR "
                        "with it" % (who, "an ASTER" if isinstance(m, ASTER) else "a MORAN", type(m).__name__))


def _check_module(m, what):
    if m is None:
        return
    p = next(m.parameters(), None)
    if p is None or not p.is_cuda:
        raise RuntimeError("tatt_amd.infer: the %s must live on an AMD GPU (found %s); the product path has no CPU fallback (the CPU "
                           "restatement lives in oracle/ and is test infrastructure)." % (what, "no parameters" if p is None else p.device))


def _crnn_folds(crnn):
    return {i: _Fold(getattr(crnn.cnn, "conv%d" % i), getattr(crnn.cnn, "batchnorm%d" % i))
            for i in range(7) if hasattr(crnn.cnn, "batchnorm%d" % i)}


def crnn_eval(crnn, folds, img, sync):
    """CRNN.forward (crnn.py) with BatchNorm folded and the chained LSTM layers: img (B, 1, 32, W) -> logits (W/4 + 1, B, 37).
    folds: `_crnn_folds(crnn)`; sync(ref) -> the 1024-word workspace of the next LSTM layer.  The sessions and `read.LineReader` share it."""
    from .crnn import CRNN
    h = img.permute(0, 2, 3, 1)
    for i in range(7):
        conv = getattr(crnn.cnn, "conv%d" % i)
        w, b = (folds[i].w, folds[i].b) if i in folds else (conv.weight, conv.bias)
        if conv.kernel_size == (3, 3):
            h = Fh.conv2d(h, w, b, ACT_RELU, any_width=True)
        else:
            h = Fh.ActFn.apply(Fh.Conv2x2ValidFn.apply(Fh._c(h), w, b), ACT_RELU)
        if i in CRNN._POOLS:
            h = Fh.max_pool(h, *CRNN._POOLS[i])
    B, Hh, Wd, C = h.shape
    seq = Fh.Permute4dFn.apply(h, (2, 1, 0, 3)).reshape(Wd, B, C)
    for blk in crnn.rnn:
        seq = Fh.linear(bilstm_eval(seq, blk.rnn, sync(seq)), blk.embedding.weight, blk.embedding.bias)
    return seq


def repack_filters(owned, modules, force):
    """Packed layouts of the folded filters `owned` (always rebuilt: their version counters never move) and of the modules' own filters
    (rebuilt when their version changed, or all of them with `force`).  Same buffers, so pointers a graph captured hold."""
    params = [p for m in modules if m is not None for p in m.parameters() if p.dim() == 4]
    for w, always in [(w, True) for w in owned] + [(p, force) for p in params]:
        h = getattr(w, "_tatt_packed", None)
        if h is None or h.key != (w.data_ptr(), tuple(w.shape), str(w.device)):
            continue
        for mode, (buf, ver) in list(h.bufs.items()):
            if always or ver != w._version:
                Cout, Cin, KH, KW = w.shape
                ops.call("tatt_repack_conv_weight", ops.P(w), ops.P(buf), Cout, Cin, KH, KW, mode, ops.stream())
                h.bufs[mode] = (buf, w._version)


class InferenceSession:
    """One eval pass -- [prior CRNN on LR ->] generator [-> PSNR / SSIM against HR] [-> recogniser + greedy CTC match on the images
    named in `accuracy_on`] -- captured as ONE hipGraph for a fixed batch size and replayed by `run`.

    generator: TSRN / TSRN_TL_TRANS (folded eval forward of the session's own) or TBSRN (its own eval forward, captured as is);
    prior: optional CRNN applied as text_prior(prior(parse_crnn_data(lr))) (the reference's model_inference for `tatt`);
    recognizer: optional CRNN whose greedy decodings of the images in `accuracy_on` ("sr", "lr", "hr") are compared with the labels.

    Weights contract: every `run` compares the version counters of all parameters and buffers of the three modules (host side, no
    sync); after a change torch sees (load_state_dict, a `.data` copy, an optimiser step) the folded filters and the packed layouts are
    rebuilt eagerly in the same buffers before the replay.  Writes torch cannot see (raw pointers) need `refresh()`.  A parameter that
    moved to another address means a new capture, done automatically.
    The arithmetic (`tatt_amd.set_arithmetic`) is the one in force at capture time: changing it later needs a new session.

    full_metrics=True (opt-in; without it the captured graph is what it always was): with `hr`, `psnr_lr_sum` / `ssim_lr_sum` of
    bicubic_resize(lr[:, :3], hr size) against HR; for every name in `accuracy_on` tatt_ctc_greedy_score runs INSTEAD of the match
    launch and fills, per image kind, `ned_stats[k]` (edit-distance histogram | scored | skipped, see `ned_from_stats`) and the last
    batch's `records[k]` (B, T + 3): decoded | length | correct | distance.  Labels are then encoded LABEL_CAP = 64 wide."""

    def __init__(self, generator, prior=None, recognizer=None, batch_size: int = None, lr_size=(16, 64), accuracy_on=("sr",),
                 voc_type: str = "lower", full_metrics: bool = False):
        from .tsrn import TSRN, TSRN_TL_TRANS
        from .tbsrn import TBSRN
        _refuse_attention_recognizer(recognizer, "InferenceSession")
        _check_module(generator, "generator")
        _check_module(prior, "prior CRNN")
        _check_module(recognizer, "recogniser CRNN")
        if not isinstance(generator, (TSRN, TSRN_TL_TRANS, TBSRN)):
            raise TypeError("InferenceSession takes a TSRN, TSRN_TL_TRANS or TBSRN generator, got %s" % type(generator).__name__)
        if not (isinstance(batch_size, int) and batch_size > 0):
            raise ValueError("batch_size must be a positive int")
        bad = set(accuracy_on) - {"sr", "lr", "hr"}
        if bad:
            raise ValueError("accuracy_on takes 'sr', 'lr', 'hr'; got %s" % sorted(bad))
        self.gen, self.prior, self.rec = generator, prior, recognizer
        self.B, self.lr_size, self.accuracy_on, self.voc_type = batch_size, tuple(lr_size), tuple(accuracy_on), voc_type
        self.device = next(generator.parameters()).device
        self.is_tatt = isinstance(generator, TSRN_TL_TRANS)
        self.fold_gen = isinstance(generator, (TSRN, TSRN_TL_TRANS))
        Fh.sticky_word(self.device)                               # (outside any capture)
        with torch.no_grad():
            self._folds = {}
            if self.fold_gen:
                k = generator.srb_nums
                for i in range(k):
                    blk = getattr(generator, "block%d" % (i + 2))
                    self._folds["srb%d" % i] = (_Fold(blk.conv1, blk.bn1), _Fold(blk.conv2, blk.bn2))
                b7 = getattr(generator, "block%d" % (k + 2))
                self._folds["b7"] = _Fold(b7[0], b7[1])
            self._crnn_folds = {id(m): _crnn_folds(m) for m in (prior, recognizer) if m is not None}
        self._keep = torch.tensor(keep_mask(voc_type), dtype=torch.int32, device=self.device)
        self.psnr_sum = torch.zeros((), device=self.device)
        self.ssim_sum = torch.zeros((), device=self.device)
        self.correct = torch.zeros(3, dtype=torch.int32, device=self.device)      # sr, lr, hr
        # full_metrics: the bicubic LR baseline's sums, per image kind the edit-distance histogram | scored | skipped, and (allocated
        # with the label buffers) the record of the LAST batch, (3, B, T + 3): decoded | length | correct | distance, -1 where not run
        self.full_metrics = bool(full_metrics)
        self.psnr_lr_sum = torch.zeros((), device=self.device)
        self.ssim_lr_sum = torch.zeros((), device=self.device)
        self.ned_stats = torch.zeros(3, HIST + 2, dtype=torch.int32, device=self.device)
        self.records = None
        self.graph = None
        self._syncs, self._sync_i = [], 0
        self._sources = [t for m in (generator, prior, recognizer) if m is not None
                         for t in list(m.parameters()) + list(m.buffers())]
        self._seen = self._snapshot()

    # -- weights contract ------------------------------------------------------------------------------------------------------------
    def _snapshot(self):
        return tuple(t._version for t in self._sources), tuple(t.data_ptr() for t in self._sources)

    def _all_folds(self):
        out = [f for pair in self._folds.values() for f in (pair if isinstance(pair, tuple) else (pair,))]
        return out + [f for d in self._crnn_folds.values() for f in d.values()]

    def _repack(self, force):
        """Packed layouts the graph reads: of the folded filters (always rebuilt: their version counters never move) and of the modules'
        own filters (rebuilt when their version changed, or all of them with `force`).  Same buffers, so the captured pointers hold."""
        repack_filters([f.w for f in self._all_folds()], (self.gen, self.prior, self.rec), force)

    def refresh(self, force: bool = True):
        """Re-fold and re-pack now (eager launches into the buffers the graph reads).  Call it after writing weights through raw
        pointers; `run` does it by itself for changes torch sees."""
        with torch.no_grad():
            for f in self._all_folds():
                f.run()
            self._repack(force)
        # versions only: a tensor that moved since the capture still makes the next run re-capture
        self._seen = (self._snapshot()[0], self._seen[1])

    def _check_weights(self):
        snap = self._snapshot()
        if snap == self._seen:
            return
        if snap[1] != self._seen[1]:                              # storage moved: the captured pointers are stale
            with torch.no_grad():
                for f in self._all_folds():
                    f.run()
            self.graph = None
            self._seen = snap
            return
        self.refresh(force=False)

    # -- the eval forward ------------------------------------------------------------------------------------------------------------
    def _sync(self, ref):
        if self._sync_i == len(self._syncs):
            self._syncs.append(_lstm_sync(ref))
        s = self._syncs[self._sync_i]
        self._sync_i += 1
        return s

    def _crnn(self, crnn, img):
        """CRNN.forward (crnn.py) with BatchNorm folded and the chained LSTM layers: img (B, 1, 32, W) -> logits (W/4 + 1, B, 37)."""
        return crnn_eval(crnn, self._crnn_folds[id(crnn)], img, self._sync)

    def _generator(self, x, tp):
        """TSRN / TSRN_TL_TRANS eval forward (tsrn._GeneratorBase._trunk_forward with training False) on folded BatchNorms."""
        from .tsrn import _gru_block, _nchw, _query_pos, _tp_interpreter
        m = self.gen
        k = m.srb_nums
        qpos = _query_pos(m.infoGen, x.shape[0], x.shape[2], x.shape[3]) if self.is_tatt else None
        if k > 0:
            Fh.gru_precompose([g for i in range(k) for g in (getattr(m, "block%d" % (i + 2)).gru1, getattr(m, "block%d" % (i + 2)).gru2)])
        xin = x.permute(0, 2, 3, 1)
        c1 = m.block1[0]
        b1 = Fh.prelu(Fh.conv2d(xin, c1.weight, c1.bias), m.block1[1].weight)
        tp_map = pr_weights = None
        if self.is_tatt:
            tp_map, pr_weights = _tp_interpreter(b1, tp.float(), m.infoGen, False, qpos, None)
        h = b1
        for i in range(k):
            blk = getattr(m, "block%d" % (i + 2))
            f1, f2 = self._folds["srb%d" % i]
            r = Fh.conv2d(h, f1.w, f1.b, ACT_MISH)                          # conv1 + bn1 + mish
            r = Fh.conv2d(r, f2.w, f2.b)                                    # conv2 + bn2
            r = _gru_block(r, blk.gru1, True, x_cat=tp_map)
            h = _gru_block(Fh.add(h, r), blk.gru2, False)
        f7 = self._folds["b7"]
        h = Fh.conv2d(h, f7.w, f7.b)
        b8 = getattr(m, "block%d" % (k + 3))
        u = Fh.add(b1, h)
        for up in list(b8)[:-1]:
            u = Fh.PixelShuffleActFn.apply(Fh.conv2d(u, up.conv.weight, up.conv.bias), ACT_MISH)
        last = b8[len(b8) - 1]
        sr = Fh.ActFn.apply(Fh.conv2d(u, last.weight, last.bias), ACT_TANH)
        Fh.gru_precompose_done()
        return _nchw(sr), pr_weights

    def _forward(self):
        from .crnn import parse_crnn_data, text_prior
        self._sync_i = 0
        lr, hr, tp = self._lr, self._hr, self._tp
        prior = None
        if self.prior is not None:
            prior = text_prior(self._crnn(self.prior, parse_crnn_data(lr)))
            tp = prior
        if self.fold_gen:
            sr, pr_weights = self._generator(lr, tp)
        else:
            sr, pr_weights = self.gen(lr), None
        if hr is not None:
            from .losses import SSIM
            from .train import calculate_psnr
            self.psnr_sum += calculate_psnr(sr[:, :3], hr[:, :3])
            self.ssim_sum += SSIM()(sr[:, :3], hr[:, :3])
            if self.full_metrics:                                 # the bicubic baseline (reference :1417-1418, :1452)
                from .crnn import bicubic_resize
                up = bicubic_resize(lr[:, :3], hr.shape[-2:])
                self.psnr_lr_sum += calculate_psnr(up, hr[:, :3])
                self.ssim_lr_sum += SSIM()(up, hr[:, :3])
        if self.rec is not None and self._labels is not None:
            from .crnn import parse_crnn_data
            imgs = {"sr": sr, "lr": lr, "hr": hr}
            self._logits = {}
            for name in self.accuracy_on:
                if imgs[name] is None:
                    continue
                logits = self._crnn(self.rec, parse_crnn_data(imgs[name][:, :3].contiguous()))
                if logits.shape[0] != CTC_T:
                    raise RuntimeError("recogniser output has %d steps, the label buffers %d" % (logits.shape[0], CTC_T))
                self._logits[name] = logits
                k = KINDS.index(name)
                if self.full_metrics:                             # the score launch INSTEAD of the match launch
                    ctc_greedy_score(logits, self._keep, self._labels[0], self._labels[1], self.correct[k:], self.ned_stats[k],
                                     self.records[k])
                else:
                    ctc_greedy_match(logits, self._keep, self._labels[0], self._labels[1], self.correct[k:])
        return sr, pr_weights, prior

    # -- capture and replay ----------------------------------------------------------------------------------------------------------
    def _stage_inputs(self, lr, hr, labels, text_prior):
        self._lr.copy_(lr)
        if hr is not None:
            self._hr.copy_(hr)
        if text_prior is not None:
            self._tp.copy_(text_prior)
        if labels is not None and self._labels is not None:
            # encoded on the host into the next pinned staging slot and copied asynchronously: no host wait on the GPU per batch.  A slot
            # is rewritten only after its previous copy has been consumed (its event; LABEL_RING slots keep the host that far ahead)
            codes, lens = (encode_labels_full if self.full_metrics else encode_labels)(labels, self.voc_type)
            k = self._ring_i % LABEL_RING
            self._ring_i += 1
            host, ev = self._lab_host[k], self._lab_events[k]
            if ev is not None:
                ev.synchronize()
            n = self.B * self._lab_w
            host[:n].copy_(torch.tensor(codes, dtype=torch.int32).reshape(-1))
            host[n:].copy_(torch.tensor(lens, dtype=torch.int32))
            self._lab_dev.copy_(host, non_blocking=True)
            ev = self._lab_events[k] = ev if ev is not None else torch.cuda.Event()
            ev.record()

    def _build(self, lr, hr, labels, text_prior):
        dev = self.device
        self._lr = torch.empty_like(lr, memory_format=torch.contiguous_format)
        self._hr = None if hr is None else torch.empty_like(hr, memory_format=torch.contiguous_format)
        self._tp = None
        if self.is_tatt and self.prior is None:
            self._tp = torch.zeros(1, 37, 1, 26, device=dev) if text_prior is None else torch.empty_like(text_prior)
        self._labels = None
        if labels is not None and self.rec is not None:
            self._lab_w = LABEL_CAP if self.full_metrics else CTC_T                          # label codes per image
            n = self.B * self._lab_w
            self._lab_dev = torch.full((n + self.B,), -1, dtype=torch.int32, device=dev)        # codes (B, width) | lengths (B)
            self._labels = (self._lab_dev[:n].view(self.B, self._lab_w), self._lab_dev[n:])
            if self.full_metrics:
                self.records = torch.full((3, self.B, CTC_T + 3), -1, dtype=torch.int32, device=dev)
            self._lab_host = [torch.empty(n + self.B, dtype=torch.int32, pin_memory=True) for _ in range(LABEL_RING)]
            self._lab_events, self._ring_i = [None] * LABEL_RING, 0
        self._has = (hr is not None, labels is not None, text_prior is not None)
        self._stage_inputs(lr, hr, labels, text_prior)
        accs = (self.psnr_sum, self.ssim_sum, self.correct, self.psnr_lr_sum, self.ssim_lr_sum, self.ned_stats)
        acc = [t.clone() for t in accs]
        self._forward()                                          # eager warm-up: workspaces, packed layouts, sync buffers
        for t, v in zip(accs, acc):
            t.copy_(v)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._out = self._forward()
        self.graph = g

    def run(self, lr, hr=None, labels: Optional[Sequence[str]] = None, text_prior=None):
        """One eval pass on a batch of `batch_size` LR images (B, C, h, w) [with HR images for PSNR / SSIM, label strings for the
        accuracies, a text prior (B, 37, 1, 26) for a TATT generator without a prior CRNN].  The first call runs eagerly once and
        captures; later calls copy the inputs into the session's static buffers and replay the graph.
        Returns (sr, pr_weights, prior) -- None where the configuration has none.  The tensors are the graph's static outputs:
        the NEXT run overwrites them (clone what must survive), as with `Trainer.step`."""
        from .tsrn import _require_gpu
        _require_gpu(lr)
        if hr is not None:
            _require_gpu(hr)
        if lr.dim() != 4 or lr.shape[0] != self.B or tuple(lr.shape[2:]) != self.lr_size:
            raise ValueError("session built for (%d, C, %d, %d) LR batches, got %s" % ((self.B,) + self.lr_size + (tuple(lr.shape),)))
        if labels is not None and len(labels) != self.B:
            raise ValueError("%d labels for a batch of %d" % (len(labels), self.B))
        if text_prior is not None and self.prior is not None:
            raise ValueError("the session computes its text prior with its prior CRNN")
        saved = [(sub, sub.training) for sub in self.gen.modules()] if not self.fold_gen and self.graph is None else []
        fork = (Fh.FWD_FORK.enabled, Fh.FWD_FORK_B.enabled)
        Fh.FWD_FORK.enabled = Fh.FWD_FORK_B.enabled = False      # one stream: no parallel branches in the captured graph
        try:
            self._check_weights()
            with torch.no_grad():
                if self.graph is None:
                    if not self.fold_gen:
                        self.gen.eval()                          # (captured as is: its own eval forward)
                    self._build(lr, hr, labels, text_prior)
                else:
                    has = (hr is not None, labels is not None, text_prior is not None)
                    if has != self._has:
                        raise ValueError("run() must get the same kinds of inputs (hr, labels, text_prior) as the call that captured")
                    self._stage_inputs(lr, hr, labels, text_prior)
                self.graph.replay()
        finally:
            Fh.FWD_FORK.enabled, Fh.FWD_FORK_B.enabled = fork
            for sub, tr in saved:                                # every submodule's own flag, as it was
                sub.training = tr
        return self._out

    def reset_metrics(self):
        self.psnr_sum.zero_()
        self.ssim_sum.zero_()
        self.correct.zero_()
        self.psnr_lr_sum.zero_()
        self.ssim_lr_sum.zero_()
        self.ned_stats.zero_()


class PendingEvaluation:
    """What `evaluate_session_async` started: the device-side totals of its sessions.  `result()` is the one host sync; with
    full_metrics `records()` reads the per-image recognition record afterwards (one more copy)."""

    def __init__(self, totals, n, n_img, full=None, records=None):
        self._totals, self.n_batches, self.n_images = totals, n, n_img
        self._full, self._records, self._rows = full, records, None

    def result(self):
        if self._totals is None:
            return {"psnr": 0.0, "ssim": 0.0, "n_batches": 0}
        # the one host sync (with full_metrics the second tensor rides behind it on the same stream)
        tot, full = self._totals.cpu(), None if self._full is None else self._full.cpu()
        n, n_img = self.n_batches, self.n_images
        corr = [int(v) for v in tot[2:].tolist()]
        res = {"psnr": float(tot[0]) / n, "ssim": float(tot[1]) / n, "n_batches": n}
        if full is not None:
            res.update(psnr_lr=float(full[0]) / n, ssim_lr=float(full[1]) / n)
        if n_img:
            res.update(accuracy=round(corr[0] / n_img, 4), accuracy_lr=round(corr[1] / n_img, 4), accuracy_hr=round(corr[2] / n_img, 4),
                       n_images=n_img)
            if full is not None:
                stats = full[2:].reshape(3, HIST + 2).round().long().tolist()
                res.update(ned=ned_from_stats(stats[0]), ned_lr=ned_from_stats(stats[1]), ned_hr=ned_from_stats(stats[2]),
                           ned_skipped=max(row[HIST + 1] for row in stats))
        return res

    def records(self):
        """The recognition record behind the reference's `vis` output (interfaces/super_resolution.py:1518-1560), one dict per image
        in batch order: 'label' (as given), the filtered decodings 'sr' / 'lr' / 'hr', the flags 'sr_correct' / 'lr_correct' /
        'hr_correct' and the edit distances 'sr_dist' / 'lr_dist' / 'hr_dist' (-1: the filtered label is longer than LABEL_CAP; an
        image kind that was not recognised gives None for its three entries).  Read it after `result()`; needs full_metrics."""
        if self._records is None:
            raise RuntimeError("records() needs evaluate_session_async(..., full_metrics=True) with a recogniser and labels")
        if self._rows is None:
            recs, labels = self._records
            host = torch.cat(recs, 1).cpu().tolist() if recs else [[], [], []]         # (3, images, T + 3)
            rows = []
            for i, lab in enumerate(labels):
                row = {"label": lab}
                for k, name in enumerate(KINDS):
                    r = host[k][i]
                    n = r[-3]
                    ran = n >= 0
                    row[name] = "".join(D2A[c] for c in r[:n]) if ran else None
                    row[name + "_correct"] = bool(r[-2]) if ran else None
                    row[name + "_dist"] = r[-1] if ran else None
                rows.append(row)
            self._rows = rows
        return self._rows


def evaluate_session_async(generator, batches: Iterable, prior=None, recognizer=None, voc_type: str = "lower",
                           sessions: dict = None, export=None, full_metrics: bool = False) -> PendingEvaluation:
    """`evaluate_session` without its final host sync: every batch is staged and replayed without the host waiting on the GPU (the
    label encodings travel through pinned staging buffers); `.result()` of the returned object reads the totals.
    `export(batch_index, pending_panels)`: when given, the lr_sr_hr panels of every batch (the eval loop's canvas,
    `DeviceExporter.panels(lr, sr, hr, gap=5)`, reference interfaces/super_resolution.py:1572-1622) are enqueued behind the batch's
    replay and the callback gets the `PendingExport`; reading it (`.result()`) is the callback's only wait, and it may keep it for
    later.  The metrics do not depend on it.
    `full_metrics`: see `evaluate_session`; each batch's record tensor is cloned on the stream behind its replay (a device copy)."""
    sessions = {} if sessions is None else sessions
    exporter = None
    if export is not None:
        from .io import DeviceExporter
        exporter = DeviceExporter(device=next(generator.parameters()).device, rule="floor")
    used, n, n_img = [], 0, 0
    recs, rec_labels = [], []
    for batch in batches:
        lr, hr = batch[0], batch[1]
        tp = batch[2] if len(batch) > 2 and batch[2] is not None and prior is None else None
        labels = batch[3] if len(batch) > 3 and recognizer is not None else None
        key = (lr.shape[0], tuple(lr.shape[2:]), tp is not None, labels is not None) + ((True,) if full_metrics else ())
        s = sessions.get(key)
        built = s is None
        if built:
            s = sessions[key] = InferenceSession(generator, prior, recognizer, batch_size=lr.shape[0], lr_size=tuple(lr.shape[2:]),
                                                 accuracy_on=("sr", "lr", "hr"), voc_type=voc_type, full_metrics=full_metrics)
        if not any(s is u for u in used):
            if not built:
                # a session kept from an earlier call: the weights and running statistics may have been written since through raw
                # pointers (the Trainer's Adam and BatchNorm kernels), which no version counter shows -- re-fold and re-pack first
                s.refresh()
            s.reset_metrics()
            used.append(s)
        out = s.run(lr, hr, labels, tp)
        if exporter is not None:
            export(n, exporter.panels(lr, out[0], hr, gap=5))          # (reads the static SR output before the next replay: same stream)
        if full_metrics and labels is not None:
            recs.append(s.records.clone())                             # (before the next replay overwrites it: same stream)
            rec_labels.extend(labels)
        n += 1
        if labels is not None:
            n_img += len(labels)
    totals = full = None
    if used:
        totals = torch.stack([torch.cat([s.psnr_sum.reshape(1).double(), s.ssim_sum.reshape(1).double(), s.correct.double()])
                              for s in used]).sum(0)
        if full_metrics:
            full = torch.stack([torch.cat([s.psnr_lr_sum.reshape(1).double(), s.ssim_lr_sum.reshape(1).double(),
                                           s.ned_stats.reshape(-1).double()]) for s in used]).sum(0)
    return PendingEvaluation(totals, n, n_img, full, (recs, rec_labels) if full_metrics and recognizer is not None else None)


def evaluate_session(generator, batches: Iterable, prior=None, recognizer=None, voc_type: str = "lower", sessions: dict = None,
                     export=None, full_metrics: bool = False):
    """Drop-in for `tatt_amd.io.evaluate` on graph-captured sessions: batches of (images_lr, images_hr[, text_prior[, label_strs]]);
    with a `prior` CRNN the text prior is computed from LR inside the graph (a batch's own prior is then ignored).  One session per
    batch size (a smaller last batch gets its own, no padding), kept in `sessions` when a dict is passed (reuse across calls: a kept
    session re-folds and re-packs from the current weights at the start of each call).  PSNR / SSIM sums and the correct-image counters
    stay on the device and no batch makes the host wait; one host sync at the end.  Returns the dict of io.evaluate.
    `export`: see `evaluate_session_async`.
    `full_metrics=True` adds the rest of the reference's report, still without a host wait per batch: 'psnr_lr' / 'ssim_lr' (the
    bicubic baseline, tatt_bicubic_resize of LR against HR) and, with a recogniser, 'ned' / 'ned_lr' / 'ned_hr' (mean normalised edit
    distance of the SR / LR / HR decodings, tatt_ctc_greedy_score in place of the match launch) and 'ned_skipped' (images whose
    filtered label has more than LABEL_CAP = 64 characters: the means leave them out).  Sessions of the two modes are kept apart."""
    _refuse_attention_recognizer(recognizer, "evaluate_session")
    return evaluate_session_async(generator, batches, prior, recognizer, voc_type, sessions, export, full_metrics).result()


# ---- PIL crops in, PIL images out ---------------------------------------------------------------------------------------------------
class PendingUpscale:
    """What `SuperResolver.__call__` started.  `result()` is the only host wait: -> the SR images as RGB PIL images, in input order
    (with a recogniser, or with a reader on long_lines: (images, texts)).  `sr`: with keep_sr, a clone of every batch's SR tensor; with
    long_lines the ONE (n_windows, C, H, W) buffer of all SR windows, beside `lr` (the window stack the sessions read) and `lines`
    (`io.Line` records).  With a reader `readings()` gives the `read.Reading` record of every line (text, confidences, steps, rw)."""

    def __init__(self, parts, with_text, sr, lr=None, lines=None, reading=None, located=None):
        self._located = located                                      # read_locate: (the (H, W) of every line canvas, out_sizes or None)
        self._parts, self._with_text, self.sr = parts, with_text, sr
        self.lr, self.lines = lr, lines                              # long_lines with keep_sr: the window stack and its Line records
        self._reading = reading                                      # long_lines with a reader: the PendingReading of the lines

    def result(self):
        images, texts = [], []
        for pending, dec, ev in self._parts:
            images.extend(pending.result())
            if dec is not None:
                ev.synchronize()
                for row in dec.tolist():                               # (T codes padded with -1 | length)
                    texts.append("".join(D2A[c] for c in row[:row[-1]]))
        if self._reading is not None:
            texts = self._reading.texts()
        return (images, texts) if self._with_text else images

    def readings(self):
        """one `read.Reading` per line, in input order (long_lines on an instance with `reader=`)"""
        if self._reading is None:
            raise RuntimeError("readings() needs SuperResolver(..., reader=crnn, long_lines=True)")
        return self._reading.result()

    def locations(self):
        """one `read.LineLocation` per line, in input order (long_lines on an instance with `read_locate=True`); every character is a
        `locate.LocatedChar`: the CharSpan's fields and `polygon`, its rectangle in the image `result()` returns for the line"""
        from .locate import locate_lines
        if self._reading is None or self._located is None:
            raise RuntimeError("locations() needs SuperResolver(..., reader=crnn, read_locate=True, long_lines=True)")
        return locate_lines(self._reading.locations(), *self._located)


class PendingScene:
    """What `SuperResolver.scene` started.  `result()` is the only host wait: -> the RGB PIL image of size (scale * Ws, scale * Hs).
    With keep_sr: `sr` the ONE (n_windows, C, H, W) buffer of all SR windows (None without boxes), `lr` the window stack the sessions
    read, `lines` its `io.Line` records (one per box), `boxes` the checked boxes and `layers` their paste layers (`io.scene_layers`).
    On an instance with `reader=`: `texts()` / `readings()`, one string / `read.Reading` per box or quad in input order ([] without
    boxes), read from the blended lines BEFORE they were pasted (so `feather` does not reach them)."""

    def __init__(self, pending, sr=None, lr=None, lines=None, boxes=None, layers=None, reading=None, located=None):
        self._pending, self.sr, self.lr, self.lines, self.boxes, self.layers = pending, sr, lr, lines, boxes, layers
        self._reading = reading
        self._located = located                                      # read_locate: (the regions, the widths of their line canvases, scale)

    def result(self):
        return self._pending.result()[0]

    def readings(self):
        if self._reading is None:
            raise RuntimeError("readings() / texts() need SuperResolver(..., reader=crnn)")
        return self._reading.result()

    def texts(self):
        return [r.text for r in self.readings()]

    def locations(self):
        """one `read.LineLocation` per box, quad or polygon, in input order (an instance with `read_locate=True`); every character is a
        `locate.LocatedChar`: the CharSpan's fields and `polygon`, its outline in the coordinates of the picture `result()` returns
        (`locate.span_polygon`)"""
        from .locate import locate_regions
        if self._reading is None or self._located is None:
            raise RuntimeError("locations() needs SuperResolver(..., reader=crnn, read_locate=True)")
        return locate_regions(self._reading.locations(), *self._located)


class SuperResolver:
    """The reference's `demo()` (interfaces/super_resolution.py:1788-1876: every file resized to the LR size, the model run at B = 1, no
    image produced) as it should have been: RGB PIL crops of any size in, RGB PIL images out.

        up = SuperResolver(generator, prior=None, recognizer=None, batch_size=48, lr_size=(16, 64), mask=True, rule="floor")
        images = up(pil_images, out_sizes=None).result()          # with a recogniser: (images, texts)

    The list is cut into batches of `batch_size` (a smaller last batch gets its own session, as in `evaluate_session`; no padding); per
    batch `DeviceCollator.stack` (PIL's resize to lr_size = (height, width) + ToTensor + mask plane in one launch) ->
    `InferenceSession.run` (one replayed hipGraph) -> `DeviceExporter` (quantise + resize in one launch, one copy back).  out_sizes: None =
    the model's HR size, or one (width, height) per image (e.g. twice each crop's own size).  Nothing waits for the device before
    `PendingUpscale.result()` (but the first batch of each size, which captures its session).  With `recognizer` (a CRNN) the greedy CTC strings of the SR images come back as well: an eager recogniser
    pass over the SR tensor after the replay, tatt_ctc_greedy_match for the decoding, the codes through a second non-blocking copy.
    A TSRN_TL_TRANS generator without a `prior` CRNN runs on the session's zero text prior.  keep_sr=True keeps a clone of each batch's
    SR tensor on the PendingUpscale (`.sr`).

    long_lines=True (opt-in; without it nothing changes) takes text lines of ANY width: an image is not squeezed into lr_size but
    resized to the LR height at its own aspect ratio and cut into LR windows `stride` columns apart (`io.line_plan`,
    `DeviceCollator.windows`: one launch for all windows of the call); the window stack is cut into batches of `batch_size` and run
    through the sessions exactly as batches are (a batch may mix windows of different lines), each batch's SR copied on the stream into
    one (n_windows, C, H, W) buffer; `DeviceExporter.lines` merges the windows of every line with tent weights in one launch.  One RGB
    image of size (scale * wl, H) per input -- an image no wider than the LR window's aspect ratio yields one window and the bytes it
    gets with long_lines=False; out_sizes: PIL resizes the finished line on the host.  Byte for byte `io.super_resolve_lines_host` on
    the same SR windows.  A TSRN_TL_TRANS generator without a `prior` runs every window on a zero row of the text prior.  No
    `recognizer` with long_lines (ValueError): it reads a 32 x 128 crop squeezed to 32 x 100; tiled lines are read by `reader=`.

    `scene(image, boxes, feather=0)` (any instance without a recogniser) takes a whole picture and a detector's boxes and returns the
    up-scaled picture with the text of every box super-resolved and pasted back: see the method.  `scene_quads(image, quads, feather=0)`
    is the same for quadrilaterals (four corner points per text instance, rotated or under perspective), `scene_polys(image, polys,
    feather=0)` for polygons of 2 N points (curved text).

    reader=crnn (opt-in; images and pictures are byte for byte those without it) reads every tiled line at its OWN width
    (`read.LineReader`, specification `read.read_lines_host`): the blended uint8 line is resized to (32, rw), rw = `read.read_width(wl)`
    (100 for a one-window line, a multiple of 20, at most 1020: a wider line is read squeezed), lines of one rw share a forward without
    padding, the greedy CTC decoding reports the soft-max probability of every decision.  Per call +1 tatt_line_luma launch, per
    bucket chunk one eager CRNN forward and one tatt_ctc_greedy_read launch, +1 copy; nothing waits before `result()`.  With
    long_lines `result()` is (images, texts) and `PendingUpscale.readings()` the `read.Reading` records; `scene` / `scene_quads` keep
    `result()` (the picture) and add `PendingScene.texts()` / `.readings()`, one per box in input order.  Lines are read before
    `out_sizes` and `feather` apply.  A plain call on an instance with `reader=` and no `recognizer=` raises ValueError.
    read_decode="beam" (read_beam, read_nbest) decodes with the CTC prefix beam search instead: one tatt_ctc_beam_read launch per
    chunk in place of the greedy one, and `readings()` gives `read.BeamReading`s (text, logp, alternatives); `texts()` as before.
    With read_lm = a `read.CharLM` (read_lm_weight, read_lm_bonus: `LineReader`'s lm_weight, lm_bonus) a character n-gram model is fused
    into that search: one tatt_ctc_beam_lm_read launch per chunk in place of the beam launch, `readings()` gives
    `read.BeamLMReading`s (text, logp, lm, score, alternatives).
    With read_pattern = a `read.Pattern` or a regular expression (read_decode="beam"; not together with read_lm) every line is read
    against that FORMAT: per chunk one tatt_ctc_beam_pattern_read launch and one tatt_ctc_pattern_mass launch in place of the greedy
    one, `readings()` gives `read.PatternReading`s (text, logp, mass, posterior, alternatives); images and pictures are unchanged.
    read_decode="lexicon" (read_lexicon = a `read.Lexicon` or a list of words, read_nbest <= 16) reads every line against that closed
    list: per chunk the tatt_ctc_lexicon_score launches and one tatt_ctc_lexicon_select launch in place of the greedy one, and
    `readings()` gives `read.LexiconReading`s (text, logp, posterior, alternatives); every text is a word of the list.
    read_decode="words" (read_lexicon, read_word_penalty = a finite float) reads every line as a SEQUENCE of list words: per chunk one
    tatt_ctc_words_read launch in place of the greedy one, `readings()` gives `read.WordsReading`s (text: the words joined by spaces,
    logp, words: one `read.WordSpan` per word with its steps and columns) and `texts()` the space-joined strings.
    read_decode="lexicons" (read_nbest <= 16) reads every line against a list of words of its OWN: the call (`__call__` with
    long_lines, `scene`, `scene_quads`, `scene_polys`) takes the keyword lexicons = a `read.LineLexicons` or one list of words per image,
    box, quad or polygon, in input order (an empty list is legal: that line reads "").  Per call one more host-to-device copy (the
    union of the lists and every chunk's tables), per chunk ONE tatt_ctc_lexicon_score_pairs launch and ONE
    tatt_ctc_lexicon_select_rows launch in place of the greedy one; `readings()` gives `read.LexiconReading`s whose text and
    alternatives are words of the line's own list and whose posterior is taken among them.  ValueError before anything is enqueued for
    a wrong number of lists, a call without the keyword, and the keyword on an instance with another read_decode.
    read_locate=True (needs reader=; read_decode "greedy" or "beam", plain or with read_lm / read_pattern: `LineReader(locate=True)`)
    says WHERE every character was read: per chunk one tatt_ctc_align launch behind the decode launch, the alignment travelling back in
    the reader's one copy.  `PendingUpscale.locations()` / `PendingScene.locations()` give one `read.LineLocation` per line whose
    characters carry `polygon`, their outline in the image or picture the caller gets back (`tatt_amd/locate.py`); images and pictures
    are byte for byte those without the keyword."""

    def __init__(self, generator, prior=None, recognizer=None, batch_size: int = 48, lr_size=(16, 64), mask: bool = True,
                 rule: str = "floor", keep_sr: bool = False, long_lines: bool = False, stride: int = 32, reader=None,
                 read_decode: str = "greedy", read_beam: int = 8, read_nbest: int = 4, read_lexicon=None,
                 read_word_penalty: float = 0.0, read_lm=None, read_lm_weight=None, read_lm_bonus=None, read_pattern=None,
                 read_locate: bool = False):
        from .io import DeviceCollator, DeviceExporter
        _refuse_attention_recognizer(recognizer, "SuperResolver")
        _check_module(generator, "generator")
        _check_module(prior, "prior CRNN")
        _check_module(recognizer, "recogniser CRNN")
        _check_module(reader, "reader CRNN")
        if not (isinstance(batch_size, int) and batch_size > 0):
            raise ValueError("batch_size must be a positive int")
        if long_lines:
            from .io import line_plan
            if recognizer is not None:
                raise ValueError("SuperResolver: a recogniser cannot read tiled lines (long_lines=True); pass recognizer=None")
            line_plan((lr_size[1], lr_size[0]), lr_size, stride)      # (raises for a stride outside [w / 2, w])
        self.gen, self.prior, self.rec = generator, prior, recognizer
        self.B, self.lr_size, self.keep_sr = batch_size, tuple(lr_size), bool(keep_sr)
        self.long_lines, self.stride, self._zero_tp = bool(long_lines), stride, {}
        self.device = next(generator.parameters()).device
        self.collator = DeviceCollator(imgH=self.lr_size[0], imgW=self.lr_size[1], down_sample_scale=1, mask=mask, device=self.device)
        self.exporter = DeviceExporter(device=self.device, rule=rule)
        self.sessions = {}
        self._ctc = {}                                               # batch size -> (keep, label, label_len) the decoding ignores
        self.reader = None
        if reader is None and read_locate:
            raise ValueError("SuperResolver: read_locate=True needs reader=crnn")
        if reader is None and read_pattern is not None:
            raise ValueError("SuperResolver: read_pattern= needs reader=crnn, read_decode='beam'")
        if reader is not None:
            from .read import LineReader
            self.reader = LineReader(reader, batch_size=batch_size, device=self.device, w=self.lr_size[1], decode=read_decode,
                                     beam=read_beam, nbest=read_nbest, lexicon=read_lexicon, word_penalty=read_word_penalty,
                                     lm=read_lm, lm_weight=read_lm_weight, lm_bonus=read_lm_bonus, pattern=read_pattern,
                                     **({"locate": True} if read_locate else {}))

    def _texts(self, sr):
        """-> (pinned (n, T + 1) int32: decoded classes | length, its event)"""
        from .crnn import parse_crnn_data
        was = self.rec.training
        self.rec.eval()
        try:
            with torch.no_grad():
                logits = self.rec(parse_crnn_data(sr[:, :3].contiguous()))
        finally:
            self.rec.train(was)
        T, n, C = logits.shape
        if (n, T) not in self._ctc:
            self._ctc[(n, T)] = (torch.ones(C, dtype=torch.int32, device=self.device),
                                 torch.zeros(n, T, dtype=torch.int32, device=self.device),
                                 torch.full((n,), -1, dtype=torch.int32, device=self.device))
        _, dec, dlen = ctc_greedy_match(logits, *self._ctc[(n, T)], want_decoded=True)
        host = torch.empty(n, T + 1, dtype=torch.int32, pin_memory=True)
        host[:, :T].copy_(dec, non_blocking=True)
        host[:, T].copy_(dlen, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return host, ev

    def _lexicons(self, who, lexicons, n):
        """the `lexicons=` keyword of a call over n lines, checked before anything is enqueued -> a `read.LineLexicons` or None"""
        if self.reader is None:
            if lexicons is not None:
                raise ValueError("SuperResolver.%s: lexicons= needs an instance with reader=crnn, read_decode='lexicons'" % who)
            return None
        return self.reader.check_lexicons(lexicons, n, "SuperResolver.%s" % who)

    def __call__(self, images, out_sizes=None, lexicons=None) -> PendingUpscale:
        images = list(images)
        if out_sizes is not None:
            out_sizes = [tuple(s) for s in out_sizes]
            if len(out_sizes) != len(images):
                raise ValueError("%d out_sizes for %d images" % (len(out_sizes), len(images)))
        if self.long_lines:
            return self._lines(images, out_sizes, self._lexicons("__call__", lexicons, len(images)))
        if lexicons is not None:
            raise ValueError("SuperResolver: lexicons= reads tiled lines (long_lines=True, scene, scene_quads, scene_polys)")
        if self.reader is not None and self.rec is None:
            raise ValueError("SuperResolver: reader= reads tiled lines (long_lines=True, scene, scene_quads); a plain call squeezes every "
                             "crop into the LR size: pass recognizer= for its texts, or build the instance with long_lines=True")
        h, w = self.lr_size
        parts, kept, fresh = [], [], set()
        with torch.cuda.device(self.device):
            for i in range(0, len(images), self.B):
                chunk = images[i:i + self.B]
                n = len(chunk)
                lr = self.collator.stack(chunk, (w, h))
                sr = self._session(n, fresh).run(lr)[0]
                parts.append((self.exporter(sr, None if out_sizes is None else out_sizes[i:i + n]),) +
                             (self._texts(sr) if self.rec is not None else (None, None)))
                if self.keep_sr:
                    kept.append(sr.clone())
        return PendingUpscale(parts, self.rec is not None, kept if self.keep_sr else None)

    def _scale(self):
        """the generator's up-scaling factor without running it: one PixelShuffle(2) stage per UpsampleBLock"""
        from .tsrn import UpsampleBLock
        return 2 ** sum(isinstance(m, UpsampleBLock) for m in self.gen.modules())

    def scene(self, image, boxes, feather: int = 0, lexicons=None) -> PendingScene:
        """A whole picture: image: an RGB PIL image, boxes: integer (x0, y0, x1, y1) rectangles of text in it (`io.scene_check`) ->
        PendingScene whose `result()` (the only host wait) is the RGB PIL image of size (scale * Ws, scale * Hs): the bicubic up-scale of
        the picture with every box replaced by its super-resolved text, later boxes over earlier ones; feather = F > 0 fades the outer F
        pixels of every pasted rectangle into what lies below.  Every box is a text line (long_lines' windows, whatever `long_lines`
        says; the instance's `stride`): `DeviceCollator.scene_windows` uploads the picture once and cuts all windows in one launch, the
        windows go through the sessions in batches of `batch_size` exactly as `long_lines` runs them, `DeviceExporter.scene` merges,
        up-scales and pastes on the device and copies the canvas back once.  Byte for byte `io.super_resolve_scene_host` on the same SR
        windows.  No boxes: the up-scaled picture, no session runs.  Not with a recogniser (ValueError)."""
        from .io import scene_layers
        return self._scene("scene", image, boxes, feather, self.collator.scene_windows, self.exporter.scene,
                           lambda b: tuple(int(v) for v in b), scene_layers, lexicons)

    def scene_quads(self, image, quads, feather: int = 0, lexicons=None) -> PendingScene:
        """`scene` for a detector's QUADRILATERALS: image: an RGB PIL image, quads: four integer corner points per text instance,
        top-left, top-right, bottom-right, bottom-left in reading direction (`io.quad_check`) -> PendingScene whose `result()` (the only
        host wait) is the RGB PIL image of size (scale * Ws, scale * Hs): the bicubic up-scale of the picture with every quad replaced by
        its super-resolved text, later quads over earlier ones, only the pixels of the quad painted; feather = F > 0 fades the outer F
        pixels of every line into what lies below.  `DeviceCollator.quad_windows` uploads the picture once, rectifies every quad into an
        upright crop and cuts all windows on the device, the windows go through the sessions in batches of `batch_size` exactly as
        `scene` runs them, `DeviceExporter.scene_quads` merges, up-scales, warps back and pastes on the device and copies the canvas back
        once.  Byte for byte `io.super_resolve_quads_host` on the same SR windows; axis-aligned quads give the bytes of `scene` on their
        boxes.  No quads: the up-scaled picture, no session runs.  Not with a recogniser (ValueError).  With keep_sr the PendingScene's
        `boxes` are the checked quads and `layers` their paste layers (`io.quad_layers`)."""
        from .io import quad_layers
        return self._scene("scene_quads", image, quads, feather, self.collator.quad_windows, self.exporter.scene_quads,
                           lambda q: tuple((int(x), int(y)) for x, y in q), quad_layers, lexicons)

    def scene_polys(self, image, polys, feather: int = 0, lexicons=None) -> PendingScene:
        """`scene_quads` for a detector's POLYGONS, curved text: image: an RGB PIL image, polys: 2 N integer points per text instance,
        2 <= N <= 8, N along the top of the text in reading direction, then N back along the bottom (`io.poly_check`; N = 2 is a quad)
        -> PendingScene whose `result()` (the only host wait) is the RGB PIL image of size (scale * Ws, scale * Hs): the bicubic up-scale
        of the picture with every polygon replaced by its super-resolved text, later polygons over earlier ones, only the pixels of the
        polygon painted; feather = F > 0 fades the outer F pixels of every line, never a seam between two strips.
        `DeviceCollator.poly_windows` straightens every polygon strip by strip into an upright crop and cuts all windows on the device,
        the windows go through the sessions as `scene` runs them, `DeviceExporter.scene_polys` merges, up-scales and pastes every line
        back along its polygon (csrc/polys.hip) and copies the canvas back once.  Byte for byte `io.super_resolve_polys_host` on the same
        SR windows; polygons of four points give the bytes of `scene_quads`.  No polygons: the up-scaled picture, no session runs.  Not
        with a recogniser (ValueError); a reader reads one line per polygon, in input order.  With keep_sr the PendingScene's `boxes` are
        the checked polygons and `layers` their paste layers (`io.poly_layers`)."""
        from .io import poly_layers
        return self._scene("scene_polys", image, polys, feather, self.collator.poly_windows, self.exporter.scene_polys,
                           lambda q: tuple((int(x), int(y)) for x, y in q), poly_layers, lexicons)

    def _scene(self, who, image, boxes, feather, windows, export, norm, layers, lexicons=None) -> PendingScene:
        """`scene`, `scene_quads` and `scene_polys` (`who`): windows = the collator's method that cuts them, export = the exporter's that
        pastes them, norm(box) = a box as the PendingScene keeps it, layers(boxes) = their paste layers"""
        from .io import line_plan
        if self.rec is not None:
            raise ValueError("SuperResolver: a recogniser cannot read tiled lines (%s); pass recognizer=None" % who)
        if not (isinstance(feather, int) and not isinstance(feather, bool) and feather >= 0):
            raise ValueError("SuperResolver.%s: feather must be an int >= 0; got %r" % (who, feather))
        h, w = self.lr_size
        line_plan((w, h), self.lr_size, self.stride)                 # (raises for a stride outside [w / 2, w])
        boxes = list(boxes)
        lexicons = self._lexicons(who, lexicons, len(boxes))
        with torch.cuda.device(self.device):
            stack, lines, scene_dev = windows(image, boxes, self.stride)
            buf, scale = self._run_windows(stack)
            boxes = [norm(b) for b in boxes]                         # (checked by `windows`)
            pending = export(scene_dev, buf, lines, boxes, scale, feather)
            reading = self._read(pending, scale, lexicons)
        located = (boxes, [r[2] for r in pending.line_canvases[1]], scale) if self.reader is not None and self.reader.locate else None
        if not self.keep_sr:
            return PendingScene(pending, reading=reading, located=located)
        return PendingScene(pending, buf, stack, lines, boxes, layers(boxes), reading, located)

    def _run_windows(self, stack):
        """a window stack through the sessions in batches of `batch_size` -> (buf, scale): the ONE (n_windows, C, H, W) buffer of all SR
        windows, each batch's SR copied into it on the stream, and H // h; (None, `_scale()`) for an empty stack"""
        from .lines import sr_scale
        fresh, buf, N = set(), None, stack.shape[0]
        for i in range(0, N, self.B):
            n = min(self.B, N - i)
            sr = self._session(n, fresh).run(stack[i:i + n], text_prior=self._zero_prior(n))[0]
            if buf is None:                                          # (in the layout the session leaves: a plain copy per batch)
                cl = sr.stride(1) == 1 and not sr.is_contiguous()
                buf = torch.empty((N,) + tuple(sr.shape[1:]), dtype=sr.dtype, device=sr.device,
                                  memory_format=torch.channels_last if cl else torch.contiguous_format)
            buf[i:i + n].copy_(sr)                                   # the session's output is static: the next replay overwrites it
        if buf is None:
            return None, self._scale()
        return buf, sr_scale(*buf.shape[2:], *self.lr_size)

    def _read(self, pending, scale, lexicons=None):
        """with a reader: its launches on the blended lines of `pending` (a PendingExport of lines / scene / scene_quads), enqueued right
        behind the exporter's on the same stream -- the lines stay where they are until the exporter's next call"""
        if self.reader is None:
            return None
        if lexicons is None:
            return self.reader.read(*pending.line_canvases, scale)
        return self.reader.read(*pending.line_canvases, scale, lexicons=lexicons)

    def _session(self, n, fresh):
        """the session of batch size n, captured on first use; refreshed once per call (`fresh`: the sizes this call has met)"""
        s = self.sessions.get(n)
        if s is None:
            s = self.sessions[n] = InferenceSession(self.gen, self.prior, None, batch_size=n, lr_size=self.lr_size)
        elif n not in fresh:
            s.refresh()                                              # weights written through raw pointers since the last call
        fresh.add(n)
        return s

    def _zero_prior(self, n):
        """a TSRN_TL_TRANS generator without a prior CRNN: the zero text prior, one row per window of the batch (the session's own
        fallback is the reference's single row, which serves a batch of one); None for every other configuration"""
        from .tsrn import TSRN_TL_TRANS
        if self.prior is not None or not isinstance(self.gen, TSRN_TL_TRANS):
            return None
        if n not in self._zero_tp:
            self._zero_tp[n] = torch.zeros(n, 37, 1, 26, device=self.device)
        return self._zero_tp[n]

    def _lines(self, images, out_sizes, lexicons=None) -> PendingUpscale:
        """the long_lines call: windows of all images -> sessions over batches of windows -> one SR buffer -> one blend launch"""
        with_text = self.reader is not None
        if not images:
            return PendingUpscale([], with_text, None, reading=self.reader.read(None, [], 1, lexicons=lexicons) if with_text else None,
                                  located=([], None) if with_text and self.reader.locate else None)
        with torch.cuda.device(self.device):
            stack, lines = self.collator.windows(images, self.stride)
            buf, scale = self._run_windows(stack)
            pending = self.exporter.lines(buf, lines, scale, out_sizes=out_sizes)
            reading = self._read(pending, scale, lexicons)
        keep = self.keep_sr
        located = ([(r[1], r[2]) for r in pending.line_canvases[1]], out_sizes) if with_text and self.reader.locate else None
        return PendingUpscale([(pending, None, None)], with_text, buf if keep else None, stack if keep else None, lines if keep else None,
                              reading, located)
