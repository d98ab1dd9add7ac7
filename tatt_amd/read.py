"""Reading super-resolved text lines at their own width (csrc/read.hip; `LineReader`, `infer.SuperResolver(reader=...)`).

The recogniser (CRNN) is trained on 32 x 100 inputs of word crops, but it is fully convolutional in width and its BiLSTMs take any number
of steps.  A tiled line (`lines.py`) is therefore read at a width of its own: `read_width` maps the line's LR width to the width `rw` of
the recogniser's input, a multiple of 20 so that lines sharing an `rw` batch together WITHOUT padding (the BiLSTM is bidirectional:
padding would change the result), and at most 1020 so that T = rw / 4 + 1 <= 256.

This module is the specification on the host, pure PIL / numpy, and the yardstick of the kernels (the CRNN itself has no CPU path and is
passed in as a callable):
* `read_width`: wl -> rw.
* `line_luma_host`: the recogniser's input of a line: Pillow's integer bicubic resize to (rw, 32), then an integer luma and ONE fp32
  multiply -- so the device equals it bit for bit.
* `ctc_greedy_read_host`: greedy CTC that says how sure it is (probabilities in float64).
* `ctc_beam_read_host`: the CTC prefix beam search (N best strings, each with the log-probability summed over its alignments in float64),
  `ctc_string_logp_host`: the exact CTC log-probability of one string.
* `read_plan`: buckets, descriptor rows and float offsets -- the host half shared by both paths.
* `read_lines_host`: the composition.
`LineReader` is the device path: one tatt_line_luma launch for all lines of a call, per bucket chunk the folded eval forward of the
session and one tatt_ctc_greedy_read launch (decode="beam": one tatt_ctc_beam_read launch of csrc/ctcbeam.hip in its place), one copy
of the record buffer back.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple

import torch

READ_QUANTUM = 20         # rw is a multiple of it
READ_MAX = 1020           # widest recogniser input: T = 1020 / 4 + 1 = 256 steps, what the decoding kernels take
READ_HEIGHT = 32          # the recogniser's input height
READ_DESC = 8             # ints per line row of tatt_line_luma (include/tatt_hip.h)
READ_CHUNK = 128          # most lines of one forward: the chained LSTM kernel's row limit
_ALIGN = 16

Reading = namedtuple("Reading", "text conf chars char_conf steps rw squeezed")
Decoded = namedtuple("Decoded", "classes steps char_conf conf")
BeamReading = namedtuple("BeamReading", "text logp alternatives rw squeezed")
BeamDecoded = namedtuple("BeamDecoded", "entries flag margin reentry", defaults=(None, None))
ReadPlan = namedtuple("ReadPlan", "buckets desc offsets floats rws squeezed")


def read_width(wl: int, w: int = 64) -> int:
    """The width at which a line of LR width `wl` (window width `w`) is read: min(READ_MAX, READ_QUANTUM * ceil(100 wl / (w READ_QUANTUM)))
    in integers.  A one-window line gives 100, the reference's parse_crnn_data width; beyond READ_MAX the line is read squeezed."""
    wl, w = int(wl), int(w)
    if wl < 1 or w < 1:
        raise ValueError("read_width: widths must be positive; got wl = %r, w = %r" % (wl, w))
    return min(READ_MAX, READ_QUANTUM * -(-100 * wl // (w * READ_QUANTUM)))


def read_squeezed(wl: int, w: int = 64) -> bool:
    """True where `read_width` hit its cap: the line is read narrower than its own aspect ratio asks for."""
    return READ_QUANTUM * -(-100 * int(wl) // (int(w) * READ_QUANTUM)) > READ_MAX


def line_luma_host(line_u8, rw: int):
    """line_u8: the (H, Wl, 3) uint8 line, the very bytes the caller gets back -> the (32, rw) float32 input of the recogniser:
    Image.fromarray(line).resize((rw, 32), BICUBIC), then n = 299 R + 587 G + 114 B as int32 (at most 255000: exact in fp32) and
    float32(n) * float32(1 / 255000)."""
    import numpy as np
    from PIL import Image
    a = np.asarray(line_u8)
    if a.ndim != 3 or a.shape[2] != 3 or a.dtype != np.uint8:
        raise ValueError("line_luma_host takes an (H, W, 3) uint8 array; got %s %s" % (a.shape, a.dtype))
    r = np.asarray(Image.fromarray(a, "RGB").resize((int(rw), READ_HEIGHT), Image.BICUBIC)).astype(np.int32)
    n = 299 * r[..., 0] + 587 * r[..., 1] + 114 * r[..., 2]
    return n.astype(np.float32) * np.float32(1.0 / 255000.0)


def ctc_greedy_read_host(logits):
    """logits (T, B, C) -> one Decoded per image: `classes` greedy CTC (arg-max per step with ties to the lower class, repeats merged,
    blank 0 dropped, every other class kept), `steps` the first time step of every emitted character's run, `char_conf` the soft-max
    probability of the arg-max at that step, `conf` the minimum over ALL T steps of the arg-max's probability (the weakest decision on
    the path; defined for an empty string too).  Probabilities are computed in float64 from the given logits."""
    import numpy as np
    x = np.asarray(logits.detach().cpu().numpy() if isinstance(logits, torch.Tensor) else logits)
    if x.ndim != 3:
        raise ValueError("ctc_greedy_read_host takes (T, B, C) logits; got %s" % (x.shape,))
    T, B, C = x.shape
    arg = x.argmax(-1)                                               # (first maximum: ties to the lower class)
    x64 = x.astype(np.float64)
    p = 1.0 / np.exp(x64 - x64.max(-1, keepdims=True)).sum(-1)       # soft-max probability of the maximum, (T, B)
    out = []
    for b in range(B):
        classes, steps, last = [], [], 0
        for t in range(T):
            c = int(arg[t, b])
            if c != last:
                if c != 0:
                    classes.append(c)
                    steps.append(t)
                last = c
        out.append(Decoded(classes, steps, [float(p[t, b]) for t in steps], float(p[:, b].min())))
    return out


def _beam_real(real):
    """the arithmetic of the beam specification: Python floats (float64), or a numpy scalar type such as np.longdouble, with which the
    tests measure the specification's own rounding -> (real, exp, log, lse)"""
    if real is None:
        import math
        real, exp, log, log1p = float, math.exp, math.log, math.log1p
    else:
        import numpy as np
        exp, log, log1p = np.exp, np.log, np.log1p
    neg = real("-inf")

    def lse(a, b):
        m, n = (a, b) if a > b else (b, a)
        return m if n == neg else m + log1p(exp(n - m))
    return real, exp, log, lse


def _beam_rows(logits, name):
    """(T, B, C) logits -> (T, B, C, rows): rows[b][t] the C logits of a step as Python floats (the fp32 values, exactly)"""
    x = logits.detach().cpu() if isinstance(logits, torch.Tensor) else torch.as_tensor(logits)
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("%s takes non-empty (T, B, C) logits; got %s" % (name, tuple(x.shape)))
    T, B, C = x.shape
    return T, B, C, x.to(torch.float32).permute(1, 0, 2).tolist()


def _log_softmax_row(x, real, exp, log):
    """one step: lp = x - max - log(sum(exp(x - max))), the sum taken class by class; None for a step with a NaN, a +inf or nothing
    finite (the line is flagged)"""
    mx = max(x)
    if any(v != v for v in x) or mx == float("inf") or mx == float("-inf"):
        return None
    d = [real(v) - real(mx) for v in x]
    s = real(0.0)
    for v in d:
        s = s + exp(v)
    ls = log(s)
    return [v - ls for v in d]


def ctc_beam_read_host(logits, beam: int = 8, nbest: int = 4, details: bool = False, real=None):
    """logits (T, B, C) -> one BeamDecoded per image: the CTC prefix beam search with blank 0, stated so that it is deterministic.

    Per step lp = log-soft-max of the fp32 logits in float64.  A beam is an ordered list of at most `beam` entries (prefix, pb, pnb):
    the log-probability of the prefix over the alignments seen so far that end in the blank / in a non-blank; it starts as
    [((), 0, -inf)].  lse(a, b) = max + log1p(exp(min - max)), lse(-inf, v) = v.  One step, for the entry of rank r (its position in
    the beam) with tot = lse(pb, pnb):
      stay      the candidate with the same prefix gets pb' = tot + lp[0] and, for a non-empty prefix, pnb' = pnb + lp[last];
      extend    by c = 1 .. C - 1: the candidate prefix + (c,) gets pnb' = (pb if c == last else tot) + lp[c], pb' = -inf.
    Candidates are identified BY THE PREFIX: an extension whose string is a prefix already in the beam adds into that prefix's stay
    candidate, pnb' = lse(pnb', contribution) (at most one per stay candidate: prefixes in a beam are distinct).  A candidate whose
    lse(pb', pnb') is -inf is none.  The new beam: the `beam` candidates of largest lse(pb', pnb'), descending, ties to the lower key;
    the key is r C for the stay candidate of rank r and r C + c for the extension of rank r by c.  After T steps the first `nbest`
    entries: BeamDecoded(entries=[(classes, logp)], flag=0), logp = lse(pb, pnb).  -inf logits are legal; a line with a NaN, a +inf or a
    step without a finite logit gives entries = [], flag = 1.

    details=True adds `margin`: the smallest gap, over all steps, between the last kept and the first dropped candidate, and over the
    final list between neighbours up to and including the first entry not returned (inf where nothing was dropped), and `reentry`:
    whether a prefix came (back) into the beam while a longer string that starts with it was in the beam -- the case in which an
    implementation that keeps prefixes as trie nodes must find the prefix's old node, not make a new one.
    `real`: a numpy scalar type (np.longdouble) to run the same arithmetic in; the default is float64."""
    beam, nbest = int(beam), int(nbest)
    if not 1 <= nbest <= beam:
        raise ValueError("ctc_beam_read_host: 1 <= nbest <= beam expected; got beam = %r, nbest = %r" % (beam, nbest))
    T, B, C, rows = _beam_rows(logits, "ctc_beam_read_host")
    real, exp, log, lse = _beam_real(real)
    neg, inf = real("-inf"), float("inf")
    out = []
    for row in rows:
        lps = [_log_softmax_row(x, real, exp, log) for x in row]
        if any(lp is None for lp in lps):
            out.append(BeamDecoded([], 1, inf, False) if details else BeamDecoded([], 1))
            continue
        cur, margin, reentry = [((), real(0.0), neg, real(0.0))], inf, False          # (prefix, pb, pnb, tot), by rank
        for lp in lps:
            where = {e[0]: r for r, e in enumerate(cur)}
            child = {}                                               # (rank of the parent, class) -> rank of that string in the beam
            for r, e in enumerate(cur):
                q = where.get(e[0][:-1]) if e[0] else None
                if q is not None:
                    child[(q, e[0][-1])] = r
            stay = [[tot + lp[0], pnb + lp[p[-1]] if p else neg] for p, pb, pnb, tot in cur]
            cands = []                                               # (total, key, pb', pnb')
            for r, (p, pb, pnb, tot) in enumerate(cur):
                last = p[-1] if p else -1
                for c in range(1, C):
                    v = (pb if c == last else tot) + lp[c]
                    q = child.get((r, c))
                    if q is not None:
                        stay[q][1] = lse(stay[q][1], v)
                    elif v != neg:
                        cands.append((v, r * C + c, neg, v))
            for r, (a, b) in enumerate(stay):
                v = lse(a, b)
                if v != neg:
                    cands.append((v, r * C, a, b))
            cands.sort(key=lambda e: (-e[0], e[1]))
            if len(cands) > beam:
                margin = min(margin, float(cands[beam - 1][0] - cands[beam][0]))
            new = []
            for v, key, a, b in cands[:beam]:
                r, c = divmod(key, C)
                new.append((cur[r][0] + (c,) if c else cur[r][0], a, b, v))
            if details:
                for e in new:
                    p = e[0]
                    if p not in where and any(len(o) > len(p) and o[:len(p)] == p for o in where):
                        reentry = True
            cur = new
        for i in range(min(nbest, len(cur) - 1)):
            margin = min(margin, float(cur[i][3] - cur[i + 1][3]))
        entries = [(list(p), v) for p, pb, pnb, v in cur[:nbest]]
        out.append(BeamDecoded(entries, 0, margin, reentry) if details else BeamDecoded(entries, 0))
    return out


def ctc_string_logp_host(logits_row, classes, real=None):
    """The exact CTC log-probability of the string `classes` (class ids 1 .. C - 1, blank 0) under the (T, C) logits of one line: the
    forward recursion over the string with a blank between and around its characters, in float64 (log-soft-max and lse as in
    `ctc_beam_read_host`).  -inf where no alignment of T steps spells the string; nan for a line `ctc_beam_read_host` flags.  This is
    the number to score a dictionary word with."""
    x = logits_row.detach().cpu() if isinstance(logits_row, torch.Tensor) else torch.as_tensor(logits_row)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError("ctc_string_logp_host takes the non-empty (T, C) logits of one line; got %s" % (tuple(x.shape),))
    C = x.shape[1]
    classes = [int(c) for c in classes]
    if any(not 1 <= c < C for c in classes):
        raise ValueError("ctc_string_logp_host: class ids are 1 .. %d; got %r" % (C - 1, classes))
    real, exp, log, lse = _beam_real(real)
    neg = real("-inf")
    lps = [_log_softmax_row(r, real, exp, log) for r in x.to(torch.float32).tolist()]
    if any(lp is None for lp in lps):
        return real("nan")
    ext = [0]
    for c in classes:
        ext += [c, 0]
    alpha = [neg] * len(ext)
    alpha[0] = lps[0][0]
    if classes:
        alpha[1] = lps[0][ext[1]]
    for lp in lps[1:]:
        nxt = []
        for s, c in enumerate(ext):
            a = alpha[s]
            if s >= 1:
                a = lse(a, alpha[s - 1])
            if s >= 2 and c != 0 and c != ext[s - 2]:
                a = lse(a, alpha[s - 2])
            nxt.append(a + lp[c])
        alpha = nxt
    return lse(alpha[-1], alpha[-2]) if classes else alpha[-1]


def _alphabet():
    from .io import ALPHABET
    return "-" + ALPHABET


def _reading(dec: Decoded, rw: int, squeezed: bool) -> Reading:
    d2a = _alphabet()
    return Reading("".join(d2a[c] for c in dec.classes), dec.conf, list(dec.classes), list(dec.char_conf), list(dec.steps), rw, squeezed)


def read_plan(line_sizes, scale, w: int = 64):
    """Host half of a read, shared by both paths.  line_sizes: per line (H, W) of its uint8 canvas -- or (byte offset, H, W, pitch) where
    it lies in a buffer; with (H, W) the lines are taken as packed one after the other, 16-byte aligned, pitch 3 W.  scale: the SR factor
    (an int, or one per line): the line's LR width is wl = W / scale -> ReadPlan(buckets, desc, offsets, floats, rws, squeezed):
    buckets [(rw, [line indices in input order])] in ascending rw; desc (n, READ_DESC) int32 rows [byte offset, H, W, pitch, rw, float
    offset of the (32, rw) target, 0, 0] in INPUT order; offsets = desc[:, 5]: the lines of one bucket lie one after the other, the
    buckets in ascending rw, so each bucket is a contiguous (n, 1, 32, rw) view of one buffer of `floats` floats."""
    import numpy as np
    rows = [tuple(int(v) for v in r) for r in line_sizes]
    scales = [int(scale)] * len(rows) if not hasattr(scale, "__len__") else [int(s) for s in scale]
    if len(scales) != len(rows):
        raise ValueError("read_plan: %d scales for %d lines" % (len(scales), len(rows)))
    desc, rws, squeezed, off = np.zeros((len(rows), READ_DESC), np.int32), [], [], 0
    for i, (r, s) in enumerate(zip(rows, scales)):
        if len(r) == 2:
            r = (off, r[0], r[1], 3 * r[1])
            off += -(-r[1] * r[3] // _ALIGN) * _ALIGN
        if len(r) != 4:
            raise ValueError("read_plan: line %d: (H, W) or (offset, H, W, pitch) expected; got %r" % (i, r))
        o, H, W, pitch = r
        if s < 1 or H < 1 or W < 1 or W % s:
            raise ValueError("read_plan: line %d: the scale %d does not divide the width of the %d x %d canvas" % (i, s, H, W))
        if o < 0 or o + H * pitch >= 2 ** 31:
            raise ValueError("read_plan: the lines do not fit 32-bit offsets")
        rws.append(read_width(W // s, w))
        squeezed.append(read_squeezed(W // s, w))
        desc[i, :5] = (o, H, W, pitch, rws[-1])
    buckets, foff = [], 0
    for rw in sorted(set(rws)):
        idx = [i for i, v in enumerate(rws) if v == rw]
        buckets.append((rw, idx))
        for i in idx:
            desc[i, 5] = foff
            foff += READ_HEIGHT * rw
        if foff >= 2 ** 31:
            raise ValueError("read_plan: the recogniser inputs do not fit 32-bit offsets")
    return ReadPlan(buckets, desc, [int(v) for v in desc[:, 5]], foff, rws, squeezed)


def read_lines_host(lines_u8, run_crnn, scale=2, w: int = 64):
    """The composition on the host: per (H, W, 3) uint8 line `line_luma_host` at rw = read_width(W / scale, w) -> `run_crnn` (a callable:
    the (1, 1, 32, rw) float tensor -> (T, 1, 37) logits) -> `ctc_greedy_read_host` -> one Reading per line."""
    import numpy as np
    lines = [np.asarray(a) for a in lines_u8]
    plan = read_plan([a.shape[:2] for a in lines], scale, w)
    out = []
    for a, rw, sq in zip(lines, plan.rws, plan.squeezed):
        x = torch.from_numpy(line_luma_host(a, rw)).reshape(1, 1, READ_HEIGHT, rw)
        out.append(_reading(ctc_greedy_read_host(run_crnn(x))[0], rw, sq))
    return out


# ---- device entry points ----------------------------------------------------------------------------------------------------------------
def read_limits():
    """tatt_read_limits: {'height', 'rw', 'down', 'width', 'lines', 'steps', 'classes', 'desc'}.  A host-only entry: needs no GPU."""
    from ._lib import LIB
    out = (ctypes.c_int * 8)()
    if LIB.tatt_read_limits(out) != 0:
        raise RuntimeError("tatt_read_limits failed")
    return dict(zip(("height", "rw", "down", "width", "lines", "steps", "classes", "desc"), (int(v) for v in out)))


def line_luma(src, desc_dev, desc_host, out):
    """ONE tatt_line_luma launch: src: the uint8 device buffer that holds the line canvases, desc_dev / desc_host: the (n, READ_DESC)
    int32 rows of `read_plan` in device memory (a tensor) and in host memory (a numpy array), out: the fp32 device buffer of the
    targets.  Raises ValueError for what the entry refuses (codes 1 / 2 / 3 of include/tatt_hip.h), before any launch."""
    from . import ops
    from ._lib import LIB
    n = int(desc_host.shape[0])
    rc = LIB.tatt_line_luma(ops.P(src), src.numel(), ops.P(desc_dev), ctypes.c_void_p(desc_host.ctypes.data), n, ops.P(out), out.numel(),
                            ops.stream())
    if rc in (1, 2, 3):
        raise ValueError("tatt_line_luma refuses these lines (code %d: %s)" % (rc, {
            1: "bad arguments", 2: "a geometry beyond read_limits()", 3: "a line or a target that leaves its buffer"}[rc]))
    if rc != 0:
        raise RuntimeError("tatt_line_luma failed with code %d" % rc)


def ctc_greedy_read(logits, index, record, cap: int):
    """ONE tatt_ctc_greedy_read launch: logits (T, B, C) fp32 on the device (any strides), index (B,) int32 on the device: the record row
    of every image, record (n_rows, >= 3 cap + 2) int32 on the device, rows contiguous, cap >= T (see `parse_records`)."""
    from . import ops
    ops._check_dev(logits)
    T, B, C = logits.shape
    if record.dtype != torch.int32 or record.dim() != 2 or record.stride(1) != 1 or index.dtype != torch.int32 or index.numel() < B:
        raise ValueError("ctc_greedy_read: record must be a 2-D int32 tensor with contiguous rows, index an int32 tensor of B entries")
    ops.call("tatt_ctc_greedy_read", ops.P(logits), *logits.stride(), T, B, C, ops.P(index), ops.P(record), record.shape[0], int(cap),
             record.stride(0), ops.stream())
    return record


def parse_records(record, cap: int):
    """record: the (n, 3 cap + 2) int32 HOST tensor tatt_ctc_greedy_read filled -> one Decoded per row"""
    ints = record.tolist()
    flts = record.view(torch.float32).tolist()
    out = []
    for ri, rf in zip(ints, flts):
        n = ri[3 * cap]
        out.append(Decoded(ri[:n], ri[cap:cap + n], rf[2 * cap:2 * cap + n], rf[3 * cap + 1]))
    return out


def beam_limits():
    """tatt_beam_limits: {'steps', 'classes', 'beam', 'nodes', 'table'}: most steps T, classes C and beam entries of
    tatt_ctc_beam_read, the nodes of a line's prefix trie and the slots of its lookup table.  A host-only entry: needs no GPU."""
    from ._lib import LIB
    out = (ctypes.c_int * 5)()
    if LIB.tatt_beam_limits(out) != 0:
        raise RuntimeError("tatt_beam_limits failed")
    return dict(zip(("steps", "classes", "beam", "nodes", "table"), (int(v) for v in out)))


def beam_entry_words(cap: int) -> int:
    """32-bit words of one entry of a beam record row: the float64 logp (2), the length, a pad word, then `cap` classes, rounded up to
    an even count so that every entry's logp is 8-byte aligned within the row"""
    return 4 + int(cap) + (int(cap) & 1)


def beam_record_words(cap: int, nbest: int) -> int:
    """32-bit words of a beam record row for `nbest` entries: [0] entries written, [1] flag, then the entries"""
    return 2 + int(nbest) * beam_entry_words(cap)


def _check_beam(what, beam, nbest, limit):
    if not (isinstance(beam, int) and isinstance(nbest, int) and 1 <= nbest <= beam <= limit):
        raise ValueError("%s: 1 <= nbest <= beam <= %d expected; got beam = %r, nbest = %r" % (what, limit, beam, nbest))


def ctc_beam_read(logits, index, record, cap: int, beam: int = 8, nbest: int = 4):
    """ONE tatt_ctc_beam_read launch: logits (T, B, C) fp32 on the device (any strides), index (B,) int32 on the device: the record row
    of every image, record (n_rows, >= beam_record_words(cap, nbest)) int32 on the device, rows contiguous, cap >= T (see
    `parse_beam_records`).  ValueError for what the entry refuses (T, C, beam, nbest, cap, the row width), before any launch."""
    from . import ops
    from ._lib import LIB
    ops._check_dev(logits)
    T, B, C = logits.shape
    if record.dtype != torch.int32 or record.dim() != 2 or record.stride(1) != 1 or index.dtype != torch.int32 or index.numel() < B:
        raise ValueError("ctc_beam_read: record must be a 2-D int32 tensor with contiguous rows, index an int32 tensor of B entries")
    _check_beam("ctc_beam_read", beam, nbest, beam_limits()["beam"])
    if record.shape[1] < beam_record_words(cap, nbest):
        raise ValueError("ctc_beam_read: rows of %d words; cap = %d and nbest = %d need %d" % (record.shape[1], cap, nbest,
                                                                                             beam_record_words(cap, nbest)))
    rc = LIB.tatt_ctc_beam_read(ops.P(logits), *logits.stride(), T, B, C, beam, nbest, ops.P(index), ops.P(record), record.shape[0],
                                int(cap), record.stride(0), ops.stream())
    if rc == 1:
        raise ValueError("tatt_ctc_beam_read refuses T = %d, C = %d, beam = %d, nbest = %d, cap = %d, rows of %d words"
                         % (T, C, beam, nbest, cap, record.stride(0)))
    if rc != 0:
        raise RuntimeError("tatt_ctc_beam_read failed with code %d" % rc)
    return record


def parse_beam_records(record, cap: int, nbest: int):
    """record: the (n, >= beam_record_words(cap, nbest)) int32 HOST tensor tatt_ctc_beam_read filled -> one BeamDecoded per row.  Row, in
    32-bit words: [0] entries written (<= nbest)  [1] flag  then per entry, beam_entry_words(cap) words: the float64 logp as it is (low
    word first), the length, a pad word, `cap` classes padded with -1."""
    import struct
    es, out = beam_entry_words(cap), []
    for row in record.tolist():
        n, flag = row[0], row[1]
        if not 0 <= n <= nbest or flag not in (0, 1):
            raise ValueError("parse_beam_records: no beam record row: entries = %r, flag = %r" % (n, flag))
        entries = []
        for i in range(n):
            e = row[2 + i * es:2 + (i + 1) * es]
            entries.append((e[4:4 + e[2]], struct.unpack("<d", struct.pack("<ii", e[0], e[1]))[0]))
        out.append(BeamDecoded(entries, flag))
    return out


def _beam_reading(dec: BeamDecoded, rw: int, squeezed: bool) -> BeamReading:
    d2a = _alphabet()
    alts = [("".join(d2a[c] for c in classes), logp) for classes, logp in dec.entries]
    text, logp = alts[0] if alts else ("", float("nan"))
    return BeamReading(text, logp, alts, rw, squeezed)


class PendingReading:
    """What `LineReader.read` started.  `result()` is the only host wait: -> one Reading (decode="beam": one BeamReading) per line, in
    input order.  With keep_logits: `logits` [(line indices of the chunk, its (T, n, C) logits on the device)]."""

    def __init__(self, host, event, cap, plan, logits=None, nbest=None):
        self._host, self._event, self._cap, self._plan, self.logits, self._out = host, event, cap, plan, logits, None
        self._nbest = nbest                                          # None: greedy records

    def result(self):
        if self._out is None:
            if self._host is None:
                self._out = []
            elif self._nbest is None:
                self._event.synchronize()
                self._out = [_reading(d, rw, sq) for d, rw, sq in zip(parse_records(self._host, self._cap), self._plan.rws,
                                                                       self._plan.squeezed)]
            else:
                self._event.synchronize()
                self._out = [_beam_reading(d, rw, sq) for d, rw, sq in zip(parse_beam_records(self._host, self._cap, self._nbest),
                                                                            self._plan.rws, self._plan.squeezed)]
        return self._out

    def texts(self):
        return [r.text for r in self.result()]


class LineReader:
    """A recogniser (CRNN) that reads uint8 text lines where they lie in device memory, each at its own width:

        reader = LineReader(crnn, batch_size=48)
        readings = reader.read(dev_bytes, rows, scale).result()      # rows: (byte offset, H, W, pitch) per line, scale = H // h

    `read` enqueues, on the current stream: the descriptor rows host-to-device from pinned memory, ONE tatt_line_luma launch for all
    lines (their (32, rw) inputs land bucket by bucket in one buffer), per bucket chunks of at most min(batch_size, 128) lines (128: the
    chained LSTM kernel's row limit; beyond its capacity the per-step kernels take over as in the session), per chunk the session's eval
    forward (`infer.crnn_eval`: BatchNorm folded, chained LSTM layers) launched eagerly and ONE tatt_ctc_greedy_read launch that
    scatters into the call's one record buffer, then ONE non-blocking copy of that buffer to pinned memory and an event.  Nothing waits
    for the device before `PendingReading.result()`.  Graph capture per (n, rw) is out of scope: the forward is launched eagerly.
    Weights contract as `InferenceSession`'s: every `read` compares the version counters of the CRNN's parameters and buffers and
    re-folds / re-packs after a change torch sees; writes torch cannot see (raw pointers) need `refresh()`.
    The arithmetic is whatever `tatt_amd.set_arithmetic` has in force at the call.  keep_logits=True keeps every chunk's logits.
    decode="beam" (with beam <= 16 and 1 <= nbest <= beam): every chunk gets ONE tatt_ctc_beam_read launch in place of the greedy one
    (the CTC prefix beam search, specification `ctc_beam_read_host`), the record buffer is sized for its rows and `result()` gives
    `BeamReading`s: the most probable string, its log-probability summed over its alignments in float64, and the `nbest` best strings
    as `alternatives`.  Everything else of a call is the same; decode="greedy" is the default."""

    def __init__(self, crnn, batch_size: int = 48, device=None, keep_logits: bool = False, w: int = 64, decode: str = "greedy",
                 beam: int = 8, nbest: int = 4):
        from . import functional as Fh
        from .infer import _check_module, _crnn_folds
        if decode not in ("greedy", "beam"):
            raise ValueError("LineReader: decode is 'greedy' or 'beam'; got %r" % (decode,))
        _check_beam("LineReader", beam, nbest, beam_limits()["beam"])
        self.decode, self.beam, self.nbest = decode, beam, nbest
        _check_module(crnn, "reader CRNN")
        if not (isinstance(batch_size, int) and batch_size > 0):
            raise ValueError("batch_size must be a positive int")
        self.crnn, self.B, self.keep_logits, self.w = crnn, batch_size, bool(keep_logits), int(w)
        self.device = next(crnn.parameters()).device
        want = self.device if device is None else torch.device(device)
        if want.type != "cuda" or (want.index is not None and want.index != self.device.index):
            raise ValueError("LineReader: the CRNN lives on %s, not on %s" % (self.device, want))
        self._limits = read_limits()
        with torch.cuda.device(self.device), torch.no_grad():
            Fh.sticky_word(self.device)
            self._folds = _crnn_folds(crnn)
        self._syncs, self._sync_i = [], 0
        self._sources = list(crnn.parameters()) + list(crnn.buffers())
        self._seen = self._snapshot()

    # -- weights contract ------------------------------------------------------------------------------------------------------------
    def _snapshot(self):
        return tuple(t._version for t in self._sources), tuple(t.data_ptr() for t in self._sources)

    def refresh(self, force: bool = True):
        """Re-fold and re-pack now.  Call it after writing weights through raw pointers; `read` does it for changes torch sees."""
        from .infer import repack_filters
        with torch.cuda.device(self.device), torch.no_grad():
            for f in self._folds.values():
                f.run()
            repack_filters([f.w for f in self._folds.values()], [self.crnn], force)
        self._seen = self._snapshot()

    def _check_weights(self):
        if self._snapshot() != self._seen:
            self.refresh(force=False)

    # -- the forward -----------------------------------------------------------------------------------------------------------------
    def _sync(self, ref):
        from .infer import _lstm_sync
        if self._sync_i == len(self._syncs):
            self._syncs.append(_lstm_sync(ref))
        s = self._syncs[self._sync_i]
        self._sync_i += 1
        return s

    def forward(self, img):
        """the folded eval forward: img (n, 1, 32, rw) fp32 on the device -> logits (rw / 4 + 1, n, 37)"""
        from .infer import crnn_eval
        self._sync_i = 0
        with torch.no_grad():
            return crnn_eval(self.crnn, self._folds, img, self._sync)

    def read(self, dev_bytes, rows, scale, keep_logits=None) -> PendingReading:
        """dev_bytes: the uint8 device buffer holding the lines, rows: (byte offset, H, W, pitch) per line (what the `line_canvases` of a
        `PendingExport` of `DeviceExporter.lines` / `.scene` / `.scene_quads` gives), scale: the SR factor -> PendingReading."""
        import numpy as np
        rows = list(rows)
        keep = self.keep_logits if keep_logits is None else bool(keep_logits)
        if not rows:
            return PendingReading(None, None, 0, None, [] if keep else None)
        if not (isinstance(dev_bytes, torch.Tensor) and dev_bytes.dtype == torch.uint8 and dev_bytes.device == self.device and
                dev_bytes.is_contiguous()):
            raise ValueError("LineReader.read takes a contiguous uint8 tensor on %s" % (self.device,))
        plan = read_plan(rows, scale, self.w)
        n = len(rows)
        order = [i for _, idx in plan.buckets for i in idx]            # bucket order -> input index: the decode launches' row indices
        cap = max(rw for rw, _ in plan.buckets) // 4 + 1
        chunk = min(self.B, READ_CHUNK)
        kept = [] if keep else None
        with torch.cuda.device(self.device):
            self._check_weights()
            head = torch.empty(n * READ_DESC + n, dtype=torch.int32, pin_memory=True)
            hn = head.numpy()
            hn[:n * READ_DESC] = plan.desc.reshape(-1)
            hn[n * READ_DESC:] = order
            head_dev = torch.empty(head.numel(), dtype=torch.int32, device=self.device)
            head_dev.copy_(head, non_blocking=True)
            luma = torch.empty(plan.floats, dtype=torch.float32, device=self.device)
            line_luma(dev_bytes, head_dev, plan.desc, luma)
            beam = self.decode == "beam"
            words = beam_record_words(cap, self.nbest) if beam else 3 * cap + 2
            record = torch.empty(n, words, dtype=torch.int32, device=self.device)
            index, pos, foff = head_dev[n * READ_DESC:], 0, 0
            for rw, idx in plan.buckets:
                x = luma[foff:foff + len(idx) * READ_HEIGHT * rw].view(len(idx), 1, READ_HEIGHT, rw)
                foff += len(idx) * READ_HEIGHT * rw
                for i in range(0, len(idx), chunk):
                    m = min(chunk, len(idx) - i)
                    logits = self.forward(x[i:i + m])
                    if beam:
                        ctc_beam_read(logits, index[pos:pos + m], record, cap, self.beam, self.nbest)
                    else:
                        ctc_greedy_read(logits, index[pos:pos + m], record, cap)
                    if keep:
                        kept.append((idx[i:i + m], logits))
                    pos += m
            host = torch.empty(n, words, dtype=torch.int32, pin_memory=True)
            host.copy_(record, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        return PendingReading(host, ev, cap, plan, kept, self.nbest if beam else None)
