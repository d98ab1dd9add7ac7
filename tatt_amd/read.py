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
* `CharLM`, `char_lm_score_host`, `ctc_beam_lm_read_host`: a character n-gram model and the beam search with it fused in (shallow
  fusion: every step ranks by acoustic mass + LM term; the specification of tatt_ctc_beam_lm_read, `LineReader(decode="beam", lm=...)`).
* `read_plan`: buckets, descriptor rows and float offsets -- the host half shared by both paths.
* `read_lines_host`: the composition.
`LineReader` is the device path: one tatt_line_luma launch for all lines of a call, per bucket chunk the folded eval forward of the
session and one tatt_ctc_greedy_read launch (decode="beam": one tatt_ctc_beam_read launch of csrc/ctcbeam.hip in its place;
decode="lexicon": the score and select launches of csrc/ctclex.hip), one copy of the record buffer back.
Reading against a closed list of words: `Lexicon` (the words as class ids, packed for the device), `ctc_lexicon_scores_host` /
`ctc_lexicon_read_host` (the specification: `ctc_string_logp_host` of every word, the N best, the normaliser over the list).
Reading a line of SEVERAL words against the list: `ctc_words_host` / `ctc_words_read_host` (the specification of csrc/ctcwords.hip: token
passing, the most probable alignment that spells a sequence of list words, with the steps every word spans); decode="words": one
tatt_ctc_words_read launch per bucket chunk in place of the greedy one.
Reading every line against a list of ITS OWN: `LineLexicons` (one list per line, their union packed for the device, `pack` the tile
table and pairs of a launch), `ctc_line_lexicons_read_host` (the specification); decode="lexicons": per bucket chunk one
tatt_ctc_lexicon_score_pairs launch and one tatt_ctc_lexicon_select_rows launch of csrc/ctclexp.hip in place of the greedy one.
Locating what was read: `ctc_align_host` / `ctc_align_read_host` (the specification of csrc/ctcalign.hip: CTC forced alignment, the most
probable alignment that spells a GIVEN string, with the steps every character spans); `LineReader(locate=True)`: one tatt_ctc_align
launch per bucket chunk behind the decode launch, which reads the best string from the decode record on the device;
`LineReader.align`: the same for strings the caller knows.  The geometry that carries the spans into the picture is tatt_amd/locate.py.
"""
from __future__ import annotations

import ctypes
import math
import struct
from collections import namedtuple

import numpy as np
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
BeamLMReading = namedtuple("BeamLMReading", "text logp lm score alternatives rw squeezed")
BeamLMDecoded = namedtuple("BeamLMDecoded", "entries flag margin reentry reranked", defaults=(None, None, None))
LexiconReading = namedtuple("LexiconReading", "text logp posterior alternatives rw squeezed")
LexiconDecoded = namedtuple("LexiconDecoded", "entries logz flag margin", defaults=(None,))
WordsDecoded = namedtuple("WordsDecoded", "words logp flag")          # words: [(the caller's word index, first step, last step)]
WordSpan = namedtuple("WordSpan", "text index first last x0 x1")
WordsReading = namedtuple("WordsReading", "text logp words rw squeezed")
LEXICON_SEGMENTS = (16, 32, 64)   # lanes of a word's segment on the device: the smallest that holds its 2 L + 1 states
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
        real, exp, log, log1p = float, math.exp, math.log, math.log1p
    else:
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
        entries, margin, reentry = _beam_search(lps, C, beam, nbest, real, lse, details)
        out.append(BeamDecoded(entries, 0, margin, reentry) if details else BeamDecoded(entries, 0))
    return out


def _beam_search(lps, C, beam, nbest, real, lse, details, table=None, accept=None):
    """the search of `ctc_beam_read_host` on a clean line's log-soft-max rows -> (entries, margin, reentry).  With `table` (rows of C
    next states, 255: none) and `accept` it is the search of `ctc_beam_pattern_read_host`: every entry carries the DFA state of its
    prefix, an extension the table has no state for is no candidate, and after the last step the entries in a non-accepting state are
    dropped before the first `nbest` are taken."""
    neg, inf = real("-inf"), float("inf")
    cur, margin, reentry = [((), real(0.0), neg, real(0.0), 0)], inf, False           # (prefix, pb, pnb, tot, state), by rank
    for lp in lps:
        where = {e[0]: r for r, e in enumerate(cur)}
        child = {}                                                   # (rank of the parent, class) -> rank of that string in the beam
        for r, e in enumerate(cur):
            q = where.get(e[0][:-1]) if e[0] else None
            if q is not None:
                child[(q, e[0][-1])] = r
        stay = [[tot + lp[0], pnb + lp[p[-1]] if p else neg] for p, pb, pnb, tot, st in cur]
        cands = []                                                   # (total, key, pb', pnb')
        for r, (p, pb, pnb, tot, st) in enumerate(cur):
            last = p[-1] if p else -1
            for c in range(1, C):
                if table is not None and table[st][c] == 255:
                    continue
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
            st = cur[r][4]
            new.append((cur[r][0] + (c,), a, b, v, table[st][c] if table is not None else 0) if c else (cur[r][0], a, b, v, st))
        if details:
            for e in new:
                p = e[0]
                if p not in where and any(len(o) > len(p) and o[:len(p)] == p for o in where):
                    reentry = True
        cur = new
    if accept is not None:
        cur = [e for e in cur if accept[e[4]]]
    for i in range(min(nbest, len(cur) - 1)):
        margin = min(margin, float(cur[i][3] - cur[i + 1][3]))
    return [(list(e[0]), e[3]) for e in cur[:nbest]], margin, reentry


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
    lps = [_log_softmax_row(r, real, exp, log) for r in x.to(torch.float32).tolist()]
    if any(lp is None for lp in lps):
        return real("nan")
    return _string_logp(lps, classes, real, lse)


def _string_logp(lps, classes, real, lse):
    """the forward recursion of `ctc_string_logp_host` on a line's log-soft-max rows"""
    neg = real("-inf")
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


def _segment(length: int, min_segment: int = 16) -> int:
    """lanes of the segment a word of `length` characters runs in: the smallest of 16, 32, 64 that holds its 2 L + 1 states, not below
    `min_segment`"""
    return next(g for g in LEXICON_SEGMENTS if 2 * length + 1 <= g and g >= min_segment)


class Lexicon:
    """A closed list of words to read lines against (`ctc_lexicon_read_host`, `LineReader(decode="lexicon")`).

    Words are lower-cased and mapped to class ids through `alphabet`: alphabet[0] stands for the blank and is no character of a word;
    the default is the reader's, "-" + io.ALPHABET.  ValueError, naming the word, for a character outside the alphabet, a word longer
    than lexicon_limits()["length"], a duplicate after lower-casing (it would be counted twice in logz); for an empty list and more than
    lexicon_limits()["words"] words.  The empty word "" is legal.
    `words`, `classes`, len() and every word index anywhere are in the CALLER's order.  For the device the words are sorted once by
    segment class (`_segment`; min_segment = 64 puts every word into a whole wave): `order` packed position -> caller's index,
    `segments` the class of every word (caller's order), `counts` words per class (a class's words are one range of the packed order,
    so the three counts are the whole tile table), `codes` the class ids of all words in packed order, `table` (K, 4) int32 per packed
    word [length, offset of its codes, caller's index, 0].  Both arrays are uploaded once per device and kept."""
    LENGTH, WORDS = 31, 65536                                        # tatt_lexicon_limits, stated here so that a list needs no library

    def __init__(self, words, alphabet=None, min_segment: int = 16):
        if isinstance(words, str):
            raise ValueError("Lexicon takes a list of words, not one string")
        words = [str(w).lower() for w in words]
        self.alphabet = _alphabet() if alphabet is None else str(alphabet)
        if min_segment not in LEXICON_SEGMENTS:
            raise ValueError("Lexicon: min_segment is one of %r; got %r" % (LEXICON_SEGMENTS, min_segment))
        if not words:
            raise ValueError("Lexicon: an empty list of words")
        if len(words) > self.WORDS:
            raise ValueError("Lexicon: %d words; at most %d" % (len(words), self.WORDS))
        a2d = {ch: i for i, ch in enumerate(self.alphabet) if i >= 1}
        seen, classes = set(), []
        for w in words:
            if len(w) > self.LENGTH:
                raise ValueError("Lexicon: the word %r has %d characters; at most %d" % (w, len(w), self.LENGTH))
            for ch in w:
                if ch not in a2d:
                    raise ValueError("Lexicon: the word %r has the character %r, which the alphabet %r lacks" % (w, ch, self.alphabet[1:]))
            if w in seen:
                raise ValueError("Lexicon: the word %r appears twice (after lower-casing)" % (w,))
            seen.add(w)
            classes.append([a2d[ch] for ch in w])
        self.words, self.classes, self.min_segment = words, classes, int(min_segment)
        self.n_classes = len(self.alphabet)
        self.segments = [_segment(len(c), self.min_segment) for c in classes]
        self.order = sorted(range(len(words)), key=lambda k: (self.segments[k], k))
        self.counts = tuple(sum(1 for g in self.segments if g == G) for G in LEXICON_SEGMENTS)
        table, codes = np.zeros((len(words), 4), np.int32), []
        for p, k in enumerate(self.order):
            table[p, :3] = (len(classes[k]), len(codes), k)
            codes += classes[k]
        self.table, self.codes, self.n_codes = table, np.asarray(codes + [0], np.int32), len(codes)     # (never an empty buffer)
        self._dev = {}

    def __len__(self):
        return len(self.words)

    def device(self, device):
        """-> (codes, table) on `device`, uploaded once"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:           # ("cuda" and "cuda:0" are one upload)
            device = torch.device("cuda", torch.cuda.current_device())
        if device not in self._dev:
            self._dev[device] = (torch.from_numpy(self.codes).to(device), torch.from_numpy(self.table).to(device))
        return self._dev[device]


class LineLexicons:
    """One closed list of words PER LINE, in the caller's line order (`ctc_line_lexicons_read_host`, `LineReader(decode="lexicons")`):
    the 50-words-per-image protocol, a detector's box that arrives with candidates of its own.

    Words are lower-cased and mapped through `alphabet` exactly as `Lexicon` does.  ValueError, naming the line and the word, for a
    character outside the alphabet, a word longer than `Lexicon.LENGTH`, a duplicate WITHIN one line's list (after lower-casing), a
    line with more than `Lexicon.WORDS` words and a union of more than `UNION` distinct words.  An EMPTY list is legal: that line
    reads "".  The same word in several lines' lists is one entry of the union.
    `lists` the lower-cased words per line, `classes` the same as class ids, `union` the distinct words in order of first appearance,
    `index` per line the union index of every word; len() the number of lines.  For the device the union is packed like a `Lexicon`:
    sorted once by segment class (`_segment`), `order` packed position -> union index, `packed` its inverse, `segments` the class of
    every union word, `codes` the class ids of all union words in packed order, `table` (U, 4) int32 per packed word [length, offset of
    its codes, union index, 0] (one zero row for an empty union: never an empty buffer).  `pack(lines)` makes the tables of one launch."""
    UNION = 1048576                                                  # tatt_line_lexicons_limits, stated here so that lists need no library

    def __init__(self, lists, alphabet=None, min_segment: int = 16):
        if isinstance(lists, str) or any(isinstance(ws, str) for ws in lists):
            raise ValueError("LineLexicons takes one list of words per line, not strings")
        self.alphabet = _alphabet() if alphabet is None else str(alphabet)
        if min_segment not in LEXICON_SEGMENTS:
            raise ValueError("LineLexicons: min_segment is one of %r; got %r" % (LEXICON_SEGMENTS, min_segment))
        a2d = {ch: i for i, ch in enumerate(self.alphabet) if i >= 1}
        self.lists, self.classes, self.index, self.union, where, union_classes = [], [], [], [], {}, []
        for b, ws in enumerate(lists):
            ws = [str(w).lower() for w in ws]
            if len(ws) > Lexicon.WORDS:
                raise ValueError("LineLexicons: line %d has %d words; at most %d" % (b, len(ws), Lexicon.WORDS))
            seen, classes, index = set(), [], []
            for w in ws:
                if len(w) > Lexicon.LENGTH:
                    raise ValueError("LineLexicons: line %d: the word %r has %d characters; at most %d" % (b, w, len(w), Lexicon.LENGTH))
                for ch in w:
                    if ch not in a2d:
                        raise ValueError("LineLexicons: line %d: the word %r has the character %r, which the alphabet %r lacks"
                                         % (b, w, ch, self.alphabet[1:]))
                if w in seen:
                    raise ValueError("LineLexicons: line %d: the word %r appears twice (after lower-casing)" % (b, w))
                seen.add(w)
                if w not in where:
                    if len(self.union) == self.UNION:
                        raise ValueError("LineLexicons: line %d: the word %r is distinct word %d of all lists; at most %d"
                                         % (b, w, self.UNION + 1, self.UNION))
                    where[w] = len(self.union)
                    self.union.append(w)
                    union_classes.append([a2d[ch] for ch in w])
                index.append(where[w])
                classes.append(union_classes[where[w]])
            self.lists.append(ws)
            self.classes.append(classes)
            self.index.append(index)
        self.min_segment, self.n_classes = int(min_segment), len(self.alphabet)
        self.segments = [_segment(len(c), self.min_segment) for c in union_classes]
        self.order = sorted(range(len(self.union)), key=lambda k: (self.segments[k], k))
        self.packed, self._groups = [0] * len(self.union), {}
        table, codes = np.zeros((max(1, len(self.union)), 4), np.int32), []
        for p, k in enumerate(self.order):
            self.packed[k] = p
            table[p, :3] = (len(union_classes[k]), len(codes), k)
            codes += union_classes[k]
        self.table, self.codes, self.n_codes = table, np.asarray(codes + [0], np.int32), len(codes)

    def __len__(self):
        return len(self.lists)

    def pack(self, lines):
        """lines: the input indices of a chunk's lines, in the order of its logits -> (tiles (n_tiles, 4) int32, pairs (n_pairs, 2)
        int32, counts (len(lines),) int32) as tatt_ctc_lexicon_score_pairs takes them: the pairs of line b (its row in the chunk) are
        grouped by segment class, within a class by position j in the line's own list; one tile row (b, G, first pair, pairs <= 256 / G)
        per non-empty tile, every pair in exactly one tile."""
        tiles, pairs, counts, n_pairs = [], [], [], 0
        for b, i in enumerate(lines):
            if i not in self._groups:                                # a line's pairs, grouped, are made once: (pairs, [(G, pairs of G)])
                index = self.index[i]
                groups = [[(self.packed[u], j) for j, u in enumerate(index) if self.segments[u] == G] for G in LEXICON_SEGMENTS]
                self._groups[i] = (np.asarray([p for g in groups for p in g], np.int32).reshape(-1, 2),
                                   [(G, len(g)) for G, g in zip(LEXICON_SEGMENTS, groups) if g])
            mine, groups = self._groups[i]
            counts.append(len(mine))
            pairs.append(mine)
            for G, n in groups:
                for f in range(0, n, 256 // G):
                    tiles.append((b, G, n_pairs + f, min(256 // G, n - f)))
                n_pairs += n
        pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2), np.int32)
        return np.asarray(tiles, np.int32).reshape(-1, 4), pairs, np.asarray(counts, np.int32)


class CharLM:
    """A character n-gram language model for the beam search (`ctc_beam_lm_read_host`, `LineReader(decode="beam", lm=...)`).

    `logp`: a float64 array of shape (C,) * order, 1 <= order <= 3, 2 <= C <= 64 (`lm_limits`): logp[h_1, .., h_{order-1}, c] is the
    log-probability of class c after the history h, the most recent class LAST; history class 0 stands for "before the line begins",
    c = 0 in the last axis for "the line ends here".  Every value must be finite (a smoothed model has no zeros): ValueError
    otherwise, and for a wrong shape or an order or class count outside the limits.  `alphabet` (default: the reader's,
    "-" + io.ALPHABET) names the classes for `from_corpus`; one that is given must have C characters."""
    ORDER, CLASSES = 3, 64                                           # tatt_lm_limits, stated here so that a model needs no library
    STEPS = 256                                                      # most steps of a line (read_limits), so most characters of a string

    def __init__(self, logp, alphabet=None):
        try:
            a = np.array(logp, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError("CharLM: logp is a float64 array of shape (C,) * order") from None
        if not 1 <= a.ndim <= self.ORDER:
            raise ValueError("CharLM: an order of 1 .. %d expected (logp has shape (C,) * order); got %d axes" % (self.ORDER, a.ndim))
        C = a.shape[-1]
        if any(n != C for n in a.shape) or not 2 <= C <= self.CLASSES:
            raise ValueError("CharLM: logp has shape (C,) * order with 2 <= C <= %d; got %s" % (self.CLASSES, a.shape))
        if not bool(np.isfinite(a).all()):
            raise ValueError("CharLM: every log-probability must be finite (smooth the model: it has no zeros)")
        if alphabet is not None and len(str(alphabet)) != C:
            raise ValueError("CharLM: the alphabet %r has %d classes, logp %d" % (str(alphabet), len(str(alphabet)), C))
        a.setflags(write=False)
        self.logp, self.order, self.n_classes = a, a.ndim, int(C)
        self.alphabet = str(alphabet) if alphabet is not None else _alphabet() if len(_alphabet()) == C else None

    @classmethod
    def from_corpus(cls, strings, order: int = 3, alphabet=None, smoothing: float = 1.0):
        """Count and smooth: every string is lower-cased and mapped through the alphabet (ValueError, naming the string, for a character
        outside it); n-grams of every order up to `order` are counted with begin padding (class 0) and ONE end event (class 0) per
        string.  P_0(c) = 1 / C and P_n(c | h) = (count(h, c) + smoothing P_{n-1}(c | h')) / (count(h) + smoothing), h' = h without its
        oldest class; in float64, in this order, so the table is deterministic and every row sums to 1."""
        if isinstance(strings, str):
            raise ValueError("CharLM.from_corpus takes a list of strings, not one string")
        alphabet = _alphabet() if alphabet is None else str(alphabet)
        C = len(alphabet)
        if not (isinstance(order, int) and 1 <= order <= cls.ORDER) or not 2 <= C <= cls.CLASSES:
            raise ValueError("CharLM.from_corpus: 1 <= order <= %d and 2 <= classes <= %d expected; got order = %r, %d classes"
                             % (cls.ORDER, cls.CLASSES, order, C))
        smoothing = float(smoothing)
        if not (math.isfinite(smoothing) and smoothing > 0.0):
            raise ValueError("CharLM.from_corpus: smoothing is a positive finite float; got %r" % (smoothing,))
        a2d = {ch: i for i, ch in enumerate(alphabet) if i >= 1}
        counts = [np.zeros((C,) * n, np.float64) for n in range(1, order + 1)]
        for s in strings:
            low = str(s).lower()
            for ch in low:
                if ch not in a2d:
                    raise ValueError("CharLM.from_corpus: the string %r has the character %r, which the alphabet %r lacks"
                                     % (s, ch, alphabet[1:]))
            padded = [0] * (order - 1) + [a2d[ch] for ch in low] + [0]
            for i in range(order - 1, len(padded)):
                for n in range(1, order + 1):
                    counts[n - 1][tuple(padded[i - n + 1:i + 1])] += 1.0
        p = np.full((), 1.0 / C, np.float64)
        for cnt in counts:
            p = (cnt + smoothing * p) / (cnt.sum(-1, keepdims=True) + smoothing)       # (p broadcasts over the new, oldest class)
        return cls(np.log(p), alphabet)

    def increments(self, weight: float = 0.5, bonus: float = 0.0):
        """-> the table W the decoders add, float64, the shape of `logp`: W[h, c] = weight logp[h, c] + bonus for c >= 1 (a character),
        W[h, 0] = weight logp[h, 0] (the end of the line gets no bonus).  Worked out ONCE here, in numpy; the host specification and the
        device read this table and only ever add its entries.  ValueError, too, where max |W| x (256 + 1) is not finite: the sum over
        the longest line and its end term must not overflow."""
        try:
            weight, bonus = float(weight), float(bonus)
        except (TypeError, ValueError):
            raise ValueError("CharLM.increments: weight and bonus are finite floats; got %r, %r" % (weight, bonus)) from None
        if not (math.isfinite(weight) and math.isfinite(bonus)):
            raise ValueError("CharLM.increments: weight and bonus are finite floats; got %r, %r" % (weight, bonus))
        with np.errstate(over="ignore"):
            w = np.float64(weight) * self.logp
            out = w + np.float64(bonus)
        out[..., 0] = w[..., 0]
        # a line adds at most STEPS entries and the end term: that sum must stay finite whatever the string, or a score could become
        # +-inf and, added to an acoustic -inf, a NaN
        if not bool(np.isfinite(out).all()) or not np.isfinite(float(np.abs(out).max()) * (self.STEPS + 1)):
            raise ValueError("CharLM.increments: with weight = %r and bonus = %r the LM term of a line of %d characters is not finite"
                             % (weight, bonus, self.STEPS))
        return np.ascontiguousarray(out)


def _limits(entry: str, names):
    """a limits entry of the library (host-only: needs no GPU) -> {name: value}"""
    from ._lib import LIB
    out = (ctypes.c_int * len(names))()
    if getattr(LIB, entry)(out) != 0:
        raise RuntimeError("%s failed" % entry)
    return dict(zip(names, (int(v) for v in out)))


def lm_limits():
    """tatt_lm_limits: {'order', 'classes'}: the largest order and the most classes of a `CharLM` table the beam kernel takes.  A
    host-only entry: needs no GPU."""
    return _limits("tatt_lm_limits", ("order", "classes"))


def _lm_row(W, prefix, order):
    """the row of the nested-list table W (`order` axes) that `prefix` selects: its last order - 1 classes, left-padded with 0"""
    if order == 1:
        return W
    if order == 2:
        return W[prefix[-1] if prefix else 0]
    return W[prefix[-2] if len(prefix) > 1 else 0][prefix[-1] if prefix else 0]


def char_lm_score_host(W, classes):
    """W: the increments table of `CharLM.increments`; classes: a string as class ids >= 1 -> (the left-to-right sum, from 0.0, of
    W[h(prefix), c] over the string's characters, the end term W[h(string), 0]); h(p): the last order - 1 classes of p, left-padded
    with 0.  Python floats: float64."""
    W = np.asarray(W, np.float64)
    classes = [int(c) for c in classes]
    if not 1 <= W.ndim <= CharLM.ORDER or any(not 1 <= c < W.shape[-1] for c in classes):
        raise ValueError("char_lm_score_host: a table of 1 .. %d axes and class ids 1 .. %d expected" % (CharLM.ORDER, W.shape[-1] - 1))
    Wl, total = W.tolist(), 0.0
    for i, c in enumerate(classes):
        total = total + _lm_row(Wl, classes[:i], W.ndim)[c]
    return total, _lm_row(Wl, classes, W.ndim)[0]


def ctc_beam_lm_read_host(logits, lm: CharLM, beam: int = 8, nbest: int = 4, weight: float = 0.5, bonus: float = 0.0,
                          details: bool = False, real=None):
    """`ctc_beam_read_host` with a character n-gram model fused into the search (shallow fusion), the specification of
    tatt_ctc_beam_lm_read.  W = lm.increments(weight, bonus).  Every beam entry carries one more number, `lm`, 0.0 for the initial
    empty prefix:
      stay      lm' = lm (an extension that spells a prefix already in the beam adds acoustically into that prefix's stay candidate, as
                in the plain search; the LM term is that prefix's own -- a function of the string alone, summed in the same order);
      extend    rank r by c: lm' = lm_r + W[h(prefix_r), c].
    A candidate whose lse(pb', pnb') is -inf is none.  The new beam: the `beam` candidates of largest score = lse(pb', pnb') + lm' (first
    lm' is formed, then the one sum), descending, ties to the lower key r C + c.  After T steps final_i = (tot_i + lm_i) +
    W[h(prefix_i), 0]; the beam is re-ranked by final, descending, ties to the lower rank, and the first `nbest` are returned:
    BeamLMDecoded(entries=[(classes, logp, lm)], flag): logp the ACOUSTIC mass lse(pb, pnb), lm the LM term with the end term.
    Flagged lines as in the plain search.  details=True adds `margin` (the smallest gap between a kept and a dropped score over all
    steps, and between neighbours of the final list up to and including the first entry not returned), `reentry` (as in the plain
    search) and `reranked` (whether the end term changed the order of the beam).  `real` as in the plain search; the LM term is float64
    under both settings, since it is data.
    The default weight and bonus are the usual shallow-fusion convention; they are not tuned on anything."""
    beam, nbest = int(beam), int(nbest)
    if not 1 <= nbest <= beam:
        raise ValueError("ctc_beam_lm_read_host: 1 <= nbest <= beam expected; got beam = %r, nbest = %r" % (beam, nbest))
    if not isinstance(lm, CharLM):
        raise ValueError("ctc_beam_lm_read_host: lm is a CharLM; got %r" % (type(lm).__name__,))
    T, B, C, rows = _beam_rows(logits, "ctc_beam_lm_read_host")
    if lm.n_classes != C:
        raise ValueError("ctc_beam_lm_read_host: the language model has %d classes, the logits %d" % (lm.n_classes, C))
    W = lm.increments(weight, bonus).tolist()
    real, exp, log, lse = _beam_real(real)
    neg, inf = real("-inf"), float("inf")
    out = []
    for row in rows:
        lps = [_log_softmax_row(x, real, exp, log) for x in row]
        if any(lp is None for lp in lps):
            out.append(BeamLMDecoded([], 1, inf, False, False) if details else BeamLMDecoded([], 1))
            continue
        cur, margin, reentry = [((), real(0.0), neg, real(0.0), 0.0)], inf, False    # (prefix, pb, pnb, tot, lm), by rank
        for lp in lps:
            where = {e[0]: r for r, e in enumerate(cur)}
            child = {}                                               # (rank of the parent, class) -> rank of that string in the beam
            for r, e in enumerate(cur):
                q = where.get(e[0][:-1]) if e[0] else None
                if q is not None:
                    child[(q, e[0][-1])] = r
            stay = [[e[3] + lp[0], e[2] + lp[e[0][-1]] if e[0] else neg] for e in cur]
            cands = []                                               # (score, key, pb', pnb', tot', lm')
            for r, (p, pb, pnb, tot, l) in enumerate(cur):
                last = p[-1] if p else -1
                w = _lm_row(W, p, lm.order)
                for c in range(1, C):
                    v = (pb if c == last else tot) + lp[c]
                    q = child.get((r, c))
                    if q is not None:
                        stay[q][1] = lse(stay[q][1], v)
                    elif v != neg:
                        l2 = l + w[c]
                        cands.append((v + l2, r * C + c, neg, v, v, l2))
            for r, (a, b) in enumerate(stay):
                v = lse(a, b)
                if v != neg:
                    cands.append((v + cur[r][4], r * C, a, b, v, cur[r][4]))
            cands.sort(key=lambda e: (-e[0], e[1]))
            if len(cands) > beam:
                margin = min(margin, float(cands[beam - 1][0] - cands[beam][0]))
            new = []
            for s, key, a, b, v, l in cands[:beam]:
                r, c = divmod(key, C)
                new.append((cur[r][0] + (c,) if c else cur[r][0], a, b, v, l))
            if details:
                for e in new:
                    p = e[0]
                    if p not in where and any(len(o) > len(p) and o[:len(p)] == p for o in where):
                        reentry = True
            cur = new
        ends = [_lm_row(W, e[0], lm.order)[0] for e in cur]
        final = [(e[3] + e[4]) + w for e, w in zip(cur, ends)]
        order = sorted(range(len(cur)), key=lambda i: (-final[i], i))
        for i in range(min(nbest, len(cur) - 1)):
            margin = min(margin, float(final[order[i]] - final[order[i + 1]]))
        entries = [(list(cur[i][0]), cur[i][3], cur[i][4] + ends[i]) for i in order[:nbest]]
        out.append(BeamLMDecoded(entries, 0, margin, reentry, order != list(range(len(cur)))) if details else BeamLMDecoded(entries, 0))
    return out


def ctc_lexicon_scores_host(logits, lexicon: Lexicon, real=None):
    """logits (T, B, C) -> per line the list score[k] = ctc_string_logp_host(logits[:, b], lexicon.classes[k], real), k in the caller's
    order (the log-soft-max of a line is worked out once); a line `ctc_beam_read_host` would flag gives None"""
    T, B, C, rows = _beam_rows(logits, "ctc_lexicon_scores_host")
    if lexicon.n_classes > C:
        raise ValueError("ctc_lexicon_scores_host: the lexicon's alphabet has %d classes, the logits %d" % (lexicon.n_classes, C))
    real, exp, log, lse = _beam_real(real)
    out = []
    for row in rows:
        lps = [_log_softmax_row(x, real, exp, log) for x in row]
        out.append(None if any(lp is None for lp in lps) else [_string_logp(lps, c, real, lse) for c in lexicon.classes])
    return out


def _lexicon_decode(scores, nbest: int = 4, details: bool = False, real=None) -> LexiconDecoded:
    """the scores of one line's words (None: a flagged line) -> LexiconDecoded, as `ctc_lexicon_read_host` states it"""
    real, exp, log, _ = _beam_real(real)
    inf = float("inf")
    if scores is None:
        return LexiconDecoded([], float("nan"), 1, inf) if details else LexiconDecoded([], float("nan"), 1)
    finite = sorted((k for k, v in enumerate(scores) if v == v and abs(v) != inf), key=lambda k: (-scores[k], k))
    entries = [(k, scores[k]) for k in finite[:nbest]]
    logz = real("-inf")
    if finite:
        m, z = scores[finite[0]], real(0.0)
        for v in scores:
            if v == v:
                z = z + exp(v - m)
        logz = m + log(z)
    if not details:
        return LexiconDecoded(entries, logz, 0)
    head = [scores[k] for k in finite[:nbest + 1]]
    return LexiconDecoded(entries, logz, 0, min([float(a - b) for a, b in zip(head, head[1:])], default=inf))


def ctc_lexicon_read_host(logits, lexicon: Lexicon, nbest: int = 4, details: bool = False, real=None, scores=None):
    """logits (T, B, C) -> one LexiconDecoded(entries, logz, flag[, margin]) per line: the line read against a closed list of words.

    score[k] = ctc_string_logp_host(logits[:, b], lexicon.classes[k], real), the exact CTC log-probability of word k.  `entries`: the
    `nbest` words of largest FINITE score as (word index, logp), descending, ties to the lower word index; shorter where fewer words
    have an alignment of T steps.  logz = m + log(sum_k exp(score[k] - m)), m the largest score and the sum taken in ascending word
    index: the log-probability that the line is one of the lexicon's words (-inf when no word has an alignment).  A line
    `ctc_beam_read_host` would flag (a NaN, a +inf, a step without a finite logit) gives entries = [], logz = nan, flag = 1.
    details=True adds `margin`: the smallest gap between neighbours among the first nbest + 1 finite scores (inf with one or none).
    `real` as in `ctc_beam_read_host`; `scores`: what `ctc_lexicon_scores_host(logits, lexicon, real)` gave, to save working it out again."""
    nbest = int(nbest)
    if nbest < 1:
        raise ValueError("ctc_lexicon_read_host: nbest >= 1 expected; got %r" % (nbest,))
    if scores is None:
        scores = ctc_lexicon_scores_host(logits, lexicon, real)
    return [_lexicon_decode(row, nbest, details, real) for row in scores]


def ctc_line_lexicons_read_host(logits, lexicons: LineLexicons, nbest: int = 4, details: bool = False, real=None):
    """logits (T, B, C), lexicons: one list per line -> one LexiconDecoded per line: line b read against ITS OWN list, exactly
    `_lexicon_decode` of [ctc_string_logp_host(logits[:, b], c, real) for c in lexicons.classes[b]].  Word indices are positions in
    line b's own list and logz runs over line b's own words.  A flagged line gives ([], nan, 1); an empty list on a clean line gives
    ([], -inf, 0).  ValueError where len(lexicons) != B or the alphabet has more classes than the logits."""
    nbest = int(nbest)
    if nbest < 1:
        raise ValueError("ctc_line_lexicons_read_host: nbest >= 1 expected; got %r" % (nbest,))
    T, B, C, rows = _beam_rows(logits, "ctc_line_lexicons_read_host")
    if len(lexicons) != B:
        raise ValueError("ctc_line_lexicons_read_host: %d lists for %d lines" % (len(lexicons), B))
    if lexicons.n_classes > C:
        raise ValueError("ctc_line_lexicons_read_host: the lexicons' alphabet has %d classes, the logits %d" % (lexicons.n_classes, C))
    real_, exp, log, lse = _beam_real(real)
    out = []
    for row, classes in zip(rows, lexicons.classes):
        lps = [_log_softmax_row(x, real_, exp, log) for x in row]
        scores = None if any(lp is None for lp in lps) else [_string_logp(lps, c, real_, lse) for c in classes]
        out.append(_lexicon_decode(scores, nbest, details, real))
    return out


def _check_penalty(what, word_penalty) -> float:
    if isinstance(word_penalty, bool) or not isinstance(word_penalty, (int, float)) or not math.isfinite(word_penalty):
        raise ValueError("%s: word_penalty must be a finite float; got %r" % (what, word_penalty))
    return float(word_penalty)


def ctc_words_host(lp, lexicon: Lexicon, word_penalty: float = 0.0) -> WordsDecoded:
    """ONE line's float64 log-probabilities lp[t][c] (T x C, blank 0) -> WordsDecoded(words, logp, flag): the best sequence of the
    lexicon's words the line spells, by token passing.  At word_penalty = 0 it is the most probable ALIGNMENT whose collapsed string is
    a concatenation of list words; `words` is [(k, first, last)] left to right, k the caller's word index, `first` the step at which
    the word's first character was entered and `last` the step at which it ended; `logp` the alignment's log-probability plus
    word_penalty per word.  Only additions, comparisons and copies of float64.

    Only words of length >= 1 take part ("" is ignored: the empty reading is always possible).  Word k with classes w[0 .. L - 1] has
    the states ch[j] (j < L) and the in-word blanks bl[j] between j and j + 1 (j < L - 1); a state holds a token (score, start).
    G[-1] = 0, X[-1][c] = -inf, all word states -inf.  "max in order": candidates are tried in the order given and only a STRICTLY
    greater score replaces the current one.  For t = 0 .. T - 1:
      enter[t][a], a >= 1   max in order of G[t - 1], then X[t - 1][c] for c = 1 .. C - 1, c != a; Esrc[t][a] the winner (0 for G);
      ch[t][j]              lp[t][w[j]] + max in order of ch[t - 1][j]; j >= 1: bl[t - 1][j - 1]; j >= 1 and w[j] != w[j - 1]:
                            ch[t - 1][j - 1]; j = 0: enter[t][w[0]] + word_penalty with start = t.  The token's start is the winner's;
      bl[t][j]              lp[t][0] + max in order of bl[t - 1][j], ch[t - 1][j];
      X[t][c]               the largest ch[t][L - 1] over the words whose last class is c, ties to the lower caller's word index;
                            Xrec[t][c] that word and its token's start;
      G[t]                  lp[t][0] + max in order of G[t - 1], X[t - 1][c] for c ascending; Gsrc[t] 0 (stay) or c.
    logp = max in order of G[T - 1], X[T - 1][c] for c ascending.  Back-trace: a word ending at step e in class c is (k, start) =
    Xrec[e][c], reported as (k, start, e); its predecessor is Esrc[start][w_k[0]]: a class c' is a word ending at start - 1 in c';
    0 means: walk Gsrc back from start - 1 while it says stay, then take the class it names; reaching t < 0 ends the walk.
    logp = -inf (no sequence of list words has an alignment of T steps) gives words = [], flag = 0.  So two words follow each other
    without a blank only if the first one's last class differs from the second one's first class, and among segmentations of ONE
    alignment (exact ties) the order of the list decides.  A negative word_penalty prefers fewer, longer words."""
    wp = _check_penalty("ctc_words_host", word_penalty)
    rows = lp.tolist() if hasattr(lp, "tolist") else [list(r) for r in lp]
    if not rows or not rows[0] or any(len(r) != len(rows[0]) for r in rows):
        raise ValueError("ctc_words_host takes the non-empty (T, C) log-probabilities of one line")
    T, C = len(rows), len(rows[0])
    if lexicon.n_classes > C:
        raise ValueError("ctc_words_host: the lexicon's alphabet has %d classes, the line %d" % (lexicon.n_classes, C))
    neg = float("-inf")
    words = [(k, w) for k, w in enumerate(lexicon.classes) if w]
    firsts = sorted({w[0] for _, w in words})
    chs, chst = [[neg] * len(w) for _, w in words], [[0] * len(w) for _, w in words]
    bls, blst = [[neg] * (len(w) - 1) for _, w in words], [[0] * (len(w) - 1) for _, w in words]
    G, X = 0.0, [neg] * C
    Xrec, Esrc, Gsrc = [], [], []
    for t, row in enumerate(rows):
        enter, esrc = {}, {}
        for a in firsts:
            m, src = G, 0
            for c in range(1, C):
                if c != a and X[c] > m:
                    m, src = X[c], c
            enter[a], esrc[a] = m, src
        gm, gs = G, 0
        for c in range(1, C):
            if X[c] > gm:
                gm, gs = X[c], c
        lp0 = row[0]
        Xn, rec = [neg] * C, [None] * C
        for i, (k, w) in enumerate(words):
            oc, ocs, ob, obs = chs[i], chst[i], bls[i], blst[i]
            nc, ncs, nb, nbs = [], [], [], []
            for j, c in enumerate(w):
                m, ms = oc[j], ocs[j]
                if j >= 1:
                    if ob[j - 1] > m:
                        m, ms = ob[j - 1], obs[j - 1]
                    if c != w[j - 1] and oc[j - 1] > m:
                        m, ms = oc[j - 1], ocs[j - 1]
                else:
                    e = enter[c] + wp
                    if e > m:
                        m, ms = e, t
                nc.append(row[c] + m)
                ncs.append(ms)
            for j in range(len(w) - 1):
                m, ms = ob[j], obs[j]
                if oc[j] > m:
                    m, ms = oc[j], ocs[j]
                nb.append(lp0 + m)
                nbs.append(ms)
            chs[i], chst[i], bls[i], blst[i] = nc, ncs, nb, nbs
            if nc[-1] > Xn[w[-1]]:
                Xn[w[-1]], rec[w[-1]] = nc[-1], (k, ncs[-1])
        G, X = lp0 + gm, Xn
        Xrec.append(rec)
        Esrc.append(esrc)
        Gsrc.append(gs)
    logp, c = G, 0
    for a in range(1, C):
        if X[a] > logp:
            logp, c = X[a], a
    if logp == neg:
        return WordsDecoded([], neg, 0)
    out, e, p = [], T - 1, T - 1
    while True:
        if c == 0:
            while p >= 0 and Gsrc[p] == 0:
                p -= 1
            if p < 0:
                break
            c, e = Gsrc[p], p - 1
        k, start = Xrec[e][c]
        out.append((k, start, e))
        c = Esrc[start][lexicon.classes[k][0]]
        e = p = start - 1
    return WordsDecoded(out[::-1], logp, 0)


def ctc_words_read_host(logits, lexicon: Lexicon, word_penalty: float = 0.0):
    """logits (T, B, C) -> one WordsDecoded per line: the log-soft-max of the other host decoders (`_log_softmax_row`, float64), then
    `ctc_words_host`.  A line they would flag (a NaN, a +inf, a step without a finite logit) gives words = [], logp = nan, flag = 1."""
    _check_penalty("ctc_words_read_host", word_penalty)
    T, B, C, rows = _beam_rows(logits, "ctc_words_read_host")
    if lexicon.n_classes > C:
        raise ValueError("ctc_words_read_host: the lexicon's alphabet has %d classes, the logits %d" % (lexicon.n_classes, C))
    real, exp, log, _ = _beam_real(None)
    out = []
    for row in rows:
        lps = [_log_softmax_row(x, real, exp, log) for x in row]
        out.append(WordsDecoded([], float("nan"), 1) if any(lp is None for lp in lps) else ctc_words_host(lps, lexicon, word_penalty))
    return out


def word_span_pixels(first: int, last: int, W: int, rw: int):
    """-> (x0, x1): the columns of the line the caller gets back (width W, read at width rw) that the steps first .. last stand for, by
    CONVENTION: a CTC step s sits at column 4 s of the rw-wide input and is given the 4 columns around it, x0 = max(0, (4 first - 2) W
    // rw), x1 = min(W, ceil((4 last + 2) W / rw)) in integers.  The CRNN's receptive field is wider than that: the span says where a
    word was read, not which pixels decided it."""
    first, last, W, rw = int(first), int(last), int(W), int(rw)
    return max(0, (4 * first - 2) * W // rw), min(W, -(-(4 * last + 2) * W // rw))


def _words_reading(dec: WordsDecoded, lexicon: Lexicon, rw: int, squeezed: bool, W: int) -> WordsReading:
    spans = [WordSpan(lexicon.words[k], k, first, last, *word_span_pixels(first, last, W, rw)) for k, first, last in dec.words]
    return WordsReading(" ".join(sp.text for sp in spans), dec.logp, spans, rw, squeezed)


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
    lines = [np.asarray(a) for a in lines_u8]
    plan = read_plan([a.shape[:2] for a in lines], scale, w)
    out = []
    for a, rw, sq in zip(lines, plan.rws, plan.squeezed):
        x = torch.from_numpy(line_luma_host(a, rw)).reshape(1, 1, READ_HEIGHT, rw)
        out.append(_reading(ctc_greedy_read_host(run_crnn(x))[0], rw, sq))
    return out


# ---- locating what was read: CTC forced alignment -------------------------------------------------------------------------------------
Aligned = namedtuple("Aligned", "spans char_logp logp flag")          # spans: [(first step, last step)] per character
CharSpan = namedtuple("CharSpan", "char cls first last x0 x1 logp")
LineLocation = namedtuple("LineLocation", "text logp chars rw squeezed flag")
ALIGN_STEPS, ALIGN_CLASSES, ALIGN_LENGTH = 256, 64, 127              # `align_limits` of the device entry (tests hold them equal)


def ctc_align_host(lp, classes) -> Aligned:
    """The specification of csrc/ctcalign.hip on ONE line.  lp: the (T, C) float64 log-soft-max rows (lists), classes: L ints in
    1 .. C - 1 (blank 0) -> Aligned(spans, char_logp, logp, flag = 0): the most probable alignment that spells the string.

    States s = 0 .. 2 L: an even state is a blank, an odd state the character classes[s // 2]; c(s) its class.  Start: v[0] = lp[0][0],
    v[1] = lp[0][c(1)] (L >= 1), every other state -inf.  Step t >= 1: the candidate for state s is v[s]; then v[s - 1] is tried
    (s >= 1); then v[s - 2] (s odd, s >= 3, c(s) != c(s - 2)); only a STRICTLY greater value replaces; the new v[s] is that value +
    lp[t][c(s)] and the back-pointer 0, 1 or 2.  End: state 2 L; state 2 L - 1 only if strictly greater.  A best value of -inf: the
    string cannot be spelled (T too short, repeats without room for the blank, -inf columns): logp = -inf, no spans.  Otherwise the
    back-pointers are walked; character k has `first` / `last`, the first and last step in state 2 k + 1, and char_logp[k], the sum of
    lp[t][classes[k]] over t = first .. last added left to right; logp is the best value itself.  Float64 additions and comparisons
    only, no multiply."""
    neg = float("-inf")
    T, L = len(lp), len(classes)
    if T < 1:
        raise ValueError("ctc_align_host takes at least one step")
    C = len(lp[0])
    if any(not (isinstance(c, int) and 1 <= c < C) for c in classes):
        raise ValueError("ctc_align_host: classes are ints in 1 .. %d; got %r" % (C - 1, list(classes)))
    S = 2 * L + 1
    cls = [classes[s // 2] if s & 1 else 0 for s in range(S)]
    v = [neg] * S
    v[0] = lp[0][0]
    if L >= 1:
        v[1] = lp[0][cls[1]]
    back = [None]
    for t in range(1, T):
        row, nv, nb = lp[t], [neg] * S, [0] * S
        for s in range(S):
            best, p = v[s], 0
            if s >= 1 and v[s - 1] > best:
                best, p = v[s - 1], 1
            if s & 1 and s >= 3 and cls[s] != cls[s - 2] and v[s - 2] > best:
                best, p = v[s - 2], 2
            nv[s], nb[s] = best + row[cls[s]], p
        v = nv
        back.append(nb)
    logp, state = v[S - 1], S - 1
    if L >= 1 and v[S - 2] > logp:
        logp, state = v[S - 2], S - 2
    if logp == neg:
        return Aligned([], [], neg, 0)
    first, last = [0] * L, [-1] * L
    for t in range(T - 1, -1, -1):
        if state & 1:
            k = state // 2
            if last[k] < 0:
                last[k] = t
            first[k] = t
        if t >= 1:
            state -= back[t][state]
    sums = []
    for k in range(L):
        acc = lp[first[k]][classes[k]]
        for t in range(first[k] + 1, last[k] + 1):
            acc = acc + lp[t][classes[k]]
        sums.append(acc)
    return Aligned(list(zip(first, last)), sums, logp, 0)


def ctc_align_read_host(logits, strings):
    """logits (T, B, C) fp32, strings: one list of classes per line -> one Aligned per line: the log-soft-max of the other host decoders
    (`_log_softmax_row`, float64), then `ctc_align_host`.  A line they would flag (a NaN, a +inf, a step without a finite logit) gives
    spans = [], logp = nan, flag = 1."""
    T, B, C, rows = _beam_rows(logits, "ctc_align_read_host")
    if len(strings) != B:
        raise ValueError("ctc_align_read_host: %d strings for %d lines" % (len(strings), B))
    real, exp, log, _ = _beam_real(None)
    out = []
    for row, classes in zip(rows, strings):
        lps = [_log_softmax_row(x, real, exp, log) for x in row]
        out.append(Aligned([], [], float("nan"), 1) if any(lp is None for lp in lps) else ctc_align_host(lps, list(classes)))
    return out


def align_record_words(cap_len: int) -> int:
    """32-bit words of the alignment part of a record row for strings of at most `cap_len` characters: [0] characters located, [1] flag,
    [2:4] logp, cap_len pairs (first, last), cap_len float64 char_logp"""
    return 4 + 4 * int(cap_len)


def pack_strings(strings, cap_len: int):
    """strings: one list of classes per line -> the (n, 2 + cap_len) int32 numpy table tatt_ctc_align reads them from with len_at = 0,
    cls_at = 2, gate_at = -1: [0] the length, [1] 0, then the classes padded with -1.  ValueError for a cap_len outside
    0 .. ALIGN_LENGTH and for a string longer than cap_len; the classes themselves are judged on the device (flag 2)."""
    if not (isinstance(cap_len, int) and 0 <= cap_len <= ALIGN_LENGTH):
        raise ValueError("pack_strings: cap_len is an int in 0 .. %d; got %r" % (ALIGN_LENGTH, cap_len))
    out = np.full((len(strings), 2 + cap_len), -1, np.int32)
    for i, s in enumerate(strings):
        s = [int(c) for c in s]
        if len(s) > cap_len:
            raise ValueError("pack_strings: line %d: %d characters, cap_len = %d" % (i, len(s), cap_len))
        out[i, 0], out[i, 1] = len(s), 0
        out[i, 2:2 + len(s)] = s
    return out


def parse_align_records(record, cap_len: int):
    """record: the (n, >= align_record_words(cap_len)) int32 HOST tensor (or numpy array) holding the alignment parts tatt_ctc_align
    wrote, from word 0 of every row -> one Aligned per row (flag 1 / 2: spans = [], logp = nan)."""
    rows = record.tolist()
    out = []
    for row in rows:
        n, flag = row[0], row[1]
        if not 0 <= n <= cap_len or flag not in (0, 1, 2) or len(row) < align_record_words(cap_len):
            raise ValueError("parse_align_records: no alignment record row: characters = %r, flag = %r" % (n, flag))
        logp = struct.unpack("<d", struct.pack("<ii", row[2], row[3]))[0]
        at = 4 + 2 * cap_len
        sums = list(struct.unpack("<%dd" % n, struct.pack("<%di" % (2 * n), *row[at:at + 2 * n])))
        out.append(Aligned([(row[4 + 2 * k], row[5 + 2 * k]) for k in range(n)], sums, logp, flag))
    return out


def _location(al: Aligned, classes, alphabet, rw: int, squeezed: bool, W: int) -> LineLocation:
    """an Aligned of the string `classes` -> the LineLocation of a line of width W read at width rw"""
    text = "".join(alphabet[c] for c in classes)
    chars = [CharSpan(alphabet[c], c, f, l, *word_span_pixels(f, l, W, rw), lp) for c, (f, l), lp in zip(classes, al.spans, al.char_logp)]
    return LineLocation(text, al.logp, chars, rw, squeezed, al.flag)


# ---- reading against a format --------------------------------------------------------------------------------------------------------------
PatternMass =namedtuple("PatternMass", "mass flag")
PatternDecoded = namedtuple("PatternDecoded", "entries mass flag margin reentry", defaults=(None, None))
PatternReading = namedtuple("PatternReading", "text logp mass posterior alternatives rw squeezed")
PATTERN_DEAD = 255        # table entry: no string of the format continues this way
_PATTERN_SUBSETS = 4096   # most subsets the subset construction may make before minimisation


class Pattern:
    """A FORMAT to read lines against (`ctc_pattern_mass_host`, `ctc_beam_pattern_read_host`, `LineReader(decode="beam", pattern=...)`):
    a regular expression over the reader's characters, compiled to a small DFA.  Registration plates, dates, prices, container codes:
    open sets with a rigid shape, which no word list holds.

    The characters are alphabet[1:]; alphabet[0] stands for the blank; the default is the reader's, "-" + io.ALPHABET.  The WHOLE line
    must match (`re.fullmatch`).  The syntax is a strict subset of Python's `re`: literal alphabet characters, `.` (any alphabet
    character), `[...]` with ranges and a leading `^`, `\\d`, `( )` and `(?: )`, `|`, and the quantifiers `?`, `*`, `+`, `{m}`, `{m,n}`
    with n <= 256.  Upper-case letters are lower-cased.  Everything else -- anchors, back-references, look-around, lazy or possessive
    quantifiers, flags, other escapes, a character outside the alphabet -- is a ValueError that names the position.
    Compiled in four steps: an NFA, the subset construction, removal of every state from which no accepting state can be reached,
    minimisation.  State 0 is the start state.  `n_states`; `table` (S, C) uint8: [q, c] the next state or 255 ("no string of the
    format continues this way"; column 0 is all 255 and never read); `accept` (S,) uint8; `accepts(text)`; `device(device)` the one
    upload.  ValueError for an empty language, a DFA of more than STATES states and an alphabet of more than CLASSES classes."""
    STEPS, CLASSES, STATES, BEAM = 256, 64, 64, 16                   # tatt_pattern_limits, stated here so that a pattern needs no library
    REPEAT = 256                                                     # the largest n of {m,n}

    def __init__(self, spec, alphabet=None):
        if not isinstance(spec, str):
            raise ValueError("Pattern takes a regular expression as a string; got %r" % (type(spec).__name__,))
        self.spec, self.alphabet = spec, _alphabet() if alphabet is None else str(alphabet)
        C = len(self.alphabet)
        if not 2 <= C <= self.CLASSES:
            raise ValueError("Pattern: an alphabet of 2 .. %d classes (the blank and the characters) expected; got %d" % (self.CLASSES, C))
        if len(set(self.alphabet[1:])) != C - 1:
            raise ValueError("Pattern: the alphabet %r names a character twice" % (self.alphabet[1:],))
        self.n_classes = C
        self._a2d = {ch: i for i, ch in enumerate(self.alphabet) if i >= 1}
        ast = _PatternParser(spec, self._a2d).parse()
        table, accept = _pattern_dfa(ast, C, spec)
        if len(accept) > self.STATES:
            raise ValueError("Pattern: %r needs a DFA of %d states; at most %d" % (spec, len(accept), self.STATES))
        self.n_states = len(accept)
        self.table, self.accept = np.asarray(table, np.uint8).reshape(self.n_states, C), np.asarray(accept, np.uint8)
        self.table.setflags(write=False)
        self.accept.setflags(write=False)
        self._wide, self._dev = {C: self.table}, {}

    def accepts(self, text) -> bool:
        """whether the format holds `text` (lower-cased, as the spec was); a character outside the alphabet: no"""
        q = 0
        for ch in str(text).lower():
            c = self._a2d.get(ch)
            if c is None:
                return False
            q = int(self.table[q, c])
            if q == PATTERN_DEAD:
                return False
        return bool(self.accept[q])

    def table_for(self, classes: int):
        """the table for logits of `classes` >= n_classes classes: the classes beyond the alphabet continue no string"""
        classes = int(classes)
        if classes < self.n_classes:
            raise ValueError("Pattern: the alphabet has %d classes, the logits %d" % (self.n_classes, classes))
        if classes not in self._wide:
            t = np.full((self.n_states, classes), PATTERN_DEAD, np.uint8)
            t[:, :self.n_classes] = self.table
            self._wide[classes] = t
        return self._wide[classes]

    def device(self, device, classes=None):
        """-> (table, accept) uint8 tensors on `device`, uploaded once (per class count of the logits)"""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:           # ("cuda" and "cuda:0" are one upload)
            device = torch.device("cuda", torch.cuda.current_device())
        key = (device, self.n_classes if classes is None else int(classes))
        if key not in self._dev:
            self._dev[key] = (torch.from_numpy(self.table_for(key[1]).copy()).to(device), torch.from_numpy(self.accept.copy()).to(device))
        return self._dev[key]


class _PatternParser:
    """recursive descent over the spec -> a tree of ("set", frozenset of classes), ("cat", [..]), ("alt", [..]), ("rep", node, m, n)
    (n None: unbounded); ValueError with the position for everything outside the subset `Pattern` states"""

    def __init__(self, spec, a2d):
        self.s, self.i, self.a2d = spec, 0, a2d
        self.all = frozenset(a2d.values())

    def fail(self, what, at=None):
        at = self.i if at is None else at
        raise ValueError("Pattern: %s at position %d of %r" % (what, at, self.s))

    def parse(self):
        node = self.alt()
        if self.i < len(self.s):
            self.fail("an unbalanced ')'")
        return node

    def alt(self):
        parts = [self.cat()]
        while self.i < len(self.s) and self.s[self.i] == "|":
            self.i += 1
            parts.append(self.cat())
        return parts[0] if len(parts) == 1 else ("alt", parts)

    def cat(self):
        parts = []
        while self.i < len(self.s) and self.s[self.i] not in "|)":
            parts.append(self.repeat())
        return ("cat", parts)

    def literal(self, ch, at):
        c = self.a2d.get(ch.lower())
        if c is None:
            self.fail("the character %r, which the alphabet lacks," % ch, at)
        return c

    def repeat(self):
        at, ch = self.i, self.s[self.i]
        if ch in "*+?{":
            self.fail("a quantifier with nothing to repeat")
        if ch in "^$":
            self.fail("an anchor (the whole line must match anyway)")
        if ch in "]}":
            self.fail("an unbalanced %r" % ch)
        self.i += 1
        if ch == ".":
            node = ("set", self.all)
        elif ch == "[":
            node = ("set", self.char_class(at))
        elif ch == "\\":
            node = ("set", self.escape(at))
        elif ch == "(":
            if self.s.startswith("?", self.i):
                if not self.s.startswith("?:", self.i):
                    self.fail("a group extension other than (?: ) (look-around, flags and named groups are not taken)", at)
                self.i += 2
            node = self.alt()
            if not self.s.startswith(")", self.i):
                self.fail("a '(' that is never closed", at)
            self.i += 1
        else:
            node = ("set", frozenset([self.literal(ch, at)]))
        if self.i < len(self.s) and self.s[self.i] in "*+?{":
            node = self.quantifier(node)
            if self.i < len(self.s) and self.s[self.i] in "*+?{":
                self.fail("a second quantifier (lazy, possessive and stacked quantifiers are not taken)")
        return node

    def escape(self, at):
        if self.s.startswith("d", self.i):
            self.i += 1
            return frozenset(c for ch, c in self.a2d.items() if ch.isdecimal())
        self.fail("an escape other than \\d", at)

    def number(self):
        j = self.i
        while j < len(self.s) and self.s[j] in "0123456789":
            j += 1
        if j == self.i:
            return None
        v, self.i = int(self.s[self.i:j]), j
        return v

    def quantifier(self, node):
        at, ch = self.i, self.s[self.i]
        self.i += 1
        if ch == "?":
            return ("rep", node, 0, 1)
        if ch == "*":
            return ("rep", node, 0, None)
        if ch == "+":
            return ("rep", node, 1, None)
        m = self.number()
        n = m
        if m is not None and self.s.startswith(",", self.i):
            self.i += 1
            n = self.number()
        if m is None or n is None or not self.s.startswith("}", self.i):
            self.fail("a quantifier that is neither {m} nor {m,n}", at)
        self.i += 1
        if n < m or n > Pattern.REPEAT:
            self.fail("a quantifier {m,n} without m <= n <= %d" % Pattern.REPEAT, at)
        return ("rep", node, m, n)

    def char_class(self, at):
        negate = self.s.startswith("^", self.i)
        self.i += negate
        members, first = set(), True
        while True:
            if self.i >= len(self.s):
                self.fail("a '[' that is never closed", at)
            j, ch = self.i, self.s[self.i]
            self.i += 1
            if ch == "]":
                if first:
                    self.fail("an empty character class", at)
                break
            first = False
            if ch == "\\":
                members |= self.escape(j)
                continue
            if ch in "[-":
                self.fail("%r inside a character class (a range needs both ends)" % ch, j)
            lo = self.literal(ch, j)
            if self.s.startswith("-", self.i) and not self.s.startswith("-]", self.i):
                k = self.i + 1
                if k >= len(self.s) or self.s[k] in "\\[-":
                    self.fail("a range without an end", self.i)
                self.literal(self.s[k], k)
                a, b = ch.lower(), self.s[k].lower()
                if b < a:
                    self.fail("a range that runs backwards", j)
                members |= {c for x, c in self.a2d.items() if a <= x <= b}
                self.i = k + 1
            elif self.s.startswith("-]", self.i):
                self.fail("'-' inside a character class (a range needs both ends)", self.i)
            else:
                members.add(lo)
        return frozenset(self.all - members if negate else members)


def _pattern_dfa(ast, C, spec):
    """the tree of `_PatternParser` -> (table rows [S][C], accept [S]) of the minimal DFA without dead states, state 0 the start"""
    eps, moves = [], []                                              # per NFA state: its epsilon targets, its (set, target) moves
    limit = 1 << 16

    def state():
        if len(eps) >= limit:
            raise ValueError("Pattern: %r unrolls into more than %d NFA states" % (spec, limit))
        eps.append([])
        moves.append([])
        return len(eps) - 1

    def build(node):                                                 # -> (entry, exit)
        kind = node[0]
        if kind == "set":
            a, b = state(), state()
            moves[a].append((node[1], b))
            return a, b
        if kind == "cat":
            a = b = state()
            for part in node[1]:
                x, y = build(part)
                eps[b].append(x)
                b = y
            return a, b
        if kind == "alt":
            a, b = state(), state()
            for part in node[1]:
                x, y = build(part)
                eps[a].append(x)
                eps[y].append(b)
            return a, b
        _, sub, m, n = node
        a = b = state()
        for _ in range(m):
            x, y = build(sub)
            eps[b].append(x)
            b = y
        if n is None:
            x, y = build(sub)
            z = state()
            eps[b] += [x, z]
            eps[y] += [x, z]
            return a, z
        z = state()
        for _ in range(n - m):
            x, y = build(sub)
            eps[b] += [x, z]
            b = y
        eps[b].append(z)
        return a, z

    start, final = build(ast)

    def closure(states):
        seen, todo = set(states), list(states)
        while todo:
            for v in eps[todo.pop()]:
                if v not in seen:
                    seen.add(v)
                    todo.append(v)
        return frozenset(seen)

    # the subset construction: only subsets reachable from the start are made
    first = closure([start])
    ids, rows, todo = {first: 0}, [], [first]
    while todo:
        sub = todo.pop(0)
        row = [-1] * C
        for c in range(1, C):
            to = {t for s in sub for chars, t in moves[s] if c in chars}
            if not to:
                continue
            to = closure(to)
            if to not in ids:
                if len(ids) >= _PATTERN_SUBSETS:
                    raise ValueError("Pattern: %r needs more than %d DFA states before minimisation" % (spec, _PATTERN_SUBSETS))
                ids[to] = len(ids)
                todo.append(to)
            row[c] = ids[to]
        rows.append(row)                                             # (subsets are numbered in the order they are taken up)
    acc = [final in sub for sub in ids]
    # states from which no accepting state can be reached are removed
    alive, grew = set(i for i, a in enumerate(acc) if a), True
    while grew:
        grew = False
        for i, row in enumerate(rows):
            if i not in alive and any(t in alive for t in row):
                alive.add(i)
                grew = True
    if 0 not in alive:
        raise ValueError("Pattern: %r matches no string over the alphabet" % (spec,))
    rows = [[t if t in alive else -1 for t in row] for row in rows]
    # minimisation: refine {accepting, not} by the blocks the moves lead to, until nothing splits (-1, "no move", is a block of its own)
    block = {i: int(acc[i]) for i in alive}
    while True:
        sig = {i: (block[i],) + tuple(block[t] if t >= 0 else -1 for t in rows[i]) for i in alive}
        names = {}
        for i in sorted(alive):
            names.setdefault(sig[i], len(names))
        new = {i: names[sig[i]] for i in alive}
        if len(names) == len(set(block.values())):
            break
        block = new
    # the blocks are numbered in the order a breadth-first walk from the start meets them: state 0 is the start
    rep = {}
    for i in sorted(alive):
        rep.setdefault(block[i], i)
    number, todo = {block[0]: 0}, [block[0]]
    while todo:
        for t in rows[rep[todo.pop(0)]]:
            if t >= 0 and block[t] not in number:
                number[block[t]] = len(number)
                todo.append(block[t])
    order = sorted(number, key=number.get)
    table = [[PATTERN_DEAD if t < 0 else number[block[t]] for t in rows[rep[b]]] for b in order]
    return table, [int(acc[rep[b]]) for b in order]


def pattern_limits():
    """tatt_pattern_limits: {'steps', 'classes', 'states', 'beam'}: most steps T and classes C of tatt_ctc_pattern_mass and
    tatt_ctc_beam_pattern_read, most states of a `Pattern`'s DFA, most beam entries.  A host-only entry: needs no GPU."""
    return _limits("tatt_pattern_limits", ("steps", "classes", "states", "beam"))


def _as_pattern(what, pattern, alphabet=None) -> "Pattern":
    if isinstance(pattern, Pattern):
        return pattern
    if isinstance(pattern, str):
        return Pattern(pattern, alphabet)
    raise ValueError("%s: pattern is a Pattern or a regular expression as a string; got %r" % (what, type(pattern).__name__))


def ctc_pattern_mass_host(logits, pattern, real=None):
    """logits (T, B, C) -> one PatternMass(mass, flag) per line: mass = the log of the summed probability of ALL alignments whose
    collapsed string the pattern's DFA accepts -- the exact probability that the line reads as any member of the format.  It is to a
    format what `logz` is to a lexicon.  The specification of tatt_ctc_pattern_mass.

    The arithmetic never subtracts.  A[q, e]: the mass of the alignments so far whose string has driven the DFA to q and that end in
    the blank (e = 0) or in the class e; A[0, 0] = 1.  Per step, p = exp(x - max) / sum(exp(x - max)) (the sum class by class):
      A'[q, 0] += p_0 sum_e A[q, e];   A'[q, c] += p_c A[q, c] for c >= 1 (the class repeats: same string, same state);
      A'[table[q, c], c] += p_c sum_{e != c} A[q, e] where the target is not 255 (the sum is A @ (1 - I): non-negative terms).
    After a step A is divided by the power of two 2^k, m = f 2^k the largest entry with 0.5 <= f < 1 (exact but for underflow), and k
    is added to an integer exponent.  mass = log(sum over accepting q and all e of A[q, e]) + exponent log(2); -inf where nothing is
    accepted in T steps.  A line with a NaN, a +inf or a step without a finite logit gives (nan, 1).
    Classes of the logits beyond the pattern's alphabet continue no string.  `real` as in `ctc_beam_read_host`."""
    pattern = _as_pattern("ctc_pattern_mass_host", pattern)
    x = logits.detach().cpu() if isinstance(logits, torch.Tensor) else torch.as_tensor(logits)
    if x.dim() != 3 or x.shape[0] < 1 or x.shape[1] < 1 or x.shape[2] < 1:
        raise ValueError("ctc_pattern_mass_host takes non-empty (T, B, C) logits; got %s" % (tuple(x.shape),))
    x = x.to(torch.float32).numpy()
    T, B, C = x.shape
    table = pattern.table_for(C)
    real = np.float64 if real is None else real
    S, acc = pattern.n_states, pattern.accept.astype(bool)
    qs, cs = np.nonzero(table[:, 1:] != PATTERN_DEAD)
    cs = cs + 1
    to = table[qs, cs].astype(np.int64)
    others = (np.ones((C, C)) - np.eye(C)).astype(real)
    out = []
    with np.errstate(under="ignore", divide="ignore"):
        for b in range(B):
            row = x[:, b, :]
            if bool(np.isnan(row).any()) or bool((row == np.inf).any()) or bool((row.max(1) == -np.inf).any()):
                out.append(PatternMass(float("nan"), 1))
                continue
            A, expo = np.zeros((S, C), real), 0
            A[0, 0] = 1
            for t in range(T):
                e = np.exp(row[t].astype(real) - real(row[t].max()))
                s = real(0.0)
                for v in e:
                    s = s + v
                p = e / s
                N = np.zeros((S, C), real)
                N[:, 0] = p[0] * A.sum(1)
                N[:, 1:] = p[1:] * A[:, 1:]
                np.add.at(N, (to, cs), (p * (A @ others))[qs, cs])
                m = N.max()
                if m > 0:
                    k = int(np.frexp(m)[1])
                    N = np.ldexp(N, -k)
                    expo += k
                A = N
            total = A[acc].sum()
            out.append(PatternMass(np.log(total) + real(expo) * np.log(real(2.0)) if total > 0 else real("-inf"), 0))
    if real is np.float64:
        out = [PatternMass(float(m.mass), m.flag) for m in out]
    return out


def ctc_beam_pattern_read_host(logits, pattern, beam: int = 8, nbest: int = 4, details: bool = False, real=None):
    """`ctc_beam_read_host` held to a format, the specification of tatt_ctc_beam_pattern_read: every beam entry carries one more number,
    the DFA state of its prefix (the root: 0).  The extension of the entry of rank r by c is a candidate only where
    table[state_r, c] != 255; stay candidates and merged extensions are as before; keys, tie rule and order are unchanged.  After the
    last step the entries in a non-accepting state are dropped, the rest keep their order, and the first `nbest` are the entries: there
    may be fewer, or none.  -> one PatternDecoded(entries=[(classes, logp)], mass, flag[, margin, reentry]) per line; `mass` is
    `ctc_pattern_mass_host`'s, so every logp <= mass.  A flagged line gives ([], nan, 1).  details, real: as in the plain search (the
    margin over the final list runs over the entries that are left)."""
    beam, nbest = int(beam), int(nbest)
    if not 1 <= nbest <= beam:
        raise ValueError("ctc_beam_pattern_read_host: 1 <= nbest <= beam expected; got beam = %r, nbest = %r" % (beam, nbest))
    pattern = _as_pattern("ctc_beam_pattern_read_host", pattern)
    T, B, C, rows = _beam_rows(logits, "ctc_beam_pattern_read_host")
    table, accept = pattern.table_for(C).tolist(), pattern.accept.tolist()
    masses = ctc_pattern_mass_host(logits, pattern, real)
    real, exp, log, lse = _beam_real(real)
    out = []
    for row, m in zip(rows, masses):
        lps = [_log_softmax_row(x, real, exp, log) for x in row]
        if any(lp is None for lp in lps):
            out.append(PatternDecoded([], float("nan"), 1, float("inf"), False) if details else PatternDecoded([], float("nan"), 1))
            continue
        entries, margin, reentry = _beam_search(lps, C, beam, nbest, real, lse, details, table, accept)
        out.append(PatternDecoded(entries, m.mass, 0, margin, reentry) if details else PatternDecoded(entries, m.mass, 0))
    return out


# ---- device entry points ----------------------------------------------------------------------------------------------------------------
def read_limits():
    """tatt_read_limits: {'height', 'rw', 'down', 'width', 'lines', 'steps', 'classes', 'desc'}.  A host-only entry: needs no GPU."""
    return _limits("tatt_read_limits", ("height", "rw", "down", "width", "lines", "steps", "classes", "desc"))


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


def _launched(entry: str, rc: int, what: str, *values):
    """the return code of a launch entry: ValueError for what the entry refuses (1, before any launch), RuntimeError for any other"""
    if rc == 1:
        raise ValueError("%s refuses %s" % (entry, what % values))
    if rc != 0:
        raise RuntimeError("%s failed with code %d" % (entry, rc))


def _check_record(what, record, index, B):
    """the record / index refusal every decode wrapper makes, under the wrapper's own name"""
    if record.dtype != torch.int32 or record.dim() != 2 or record.stride(1) != 1 or index.dtype != torch.int32 or index.numel() < B:
        raise ValueError("%s: record must be a 2-D int32 tensor with contiguous rows, index an int32 tensor of B entries" % what)


def _greedy_best_at(cap: int):
    """(len_at, cls_at, gate_at) of the string in a greedy record row: `cap` classes, `cap` steps, `cap` confidences, then the length;
    no gate word (-1).  `parse_records` and the alignment behind a greedy launch both read the row through it."""
    return 3 * int(cap), 0, -1


def ctc_greedy_read(logits, index, record, cap: int):
    """ONE tatt_ctc_greedy_read launch: logits (T, B, C) fp32 on the device (any strides), index (B,) int32 on the device: the record row
    of every image, record (n_rows, >= 3 cap + 2) int32 on the device, rows contiguous, cap >= T (see `parse_records`)."""
    from . import ops
    ops._check_dev(logits)
    T, B, C = logits.shape
    _check_record("ctc_greedy_read", record, index, B)
    ops.call("tatt_ctc_greedy_read", ops.P(logits), *logits.stride(), T, B, C, ops.P(index), ops.P(record), record.shape[0], int(cap),
             record.stride(0), ops.stream())
    return record


def parse_records(record, cap: int):
    """record: the (n, 3 cap + 2) int32 HOST tensor tatt_ctc_greedy_read filled -> one Decoded per row"""
    ints = record.tolist()
    flts = record.view(torch.float32).tolist()
    len_at, cls_at, _ = _greedy_best_at(cap)
    out = []
    for ri, rf in zip(ints, flts):
        n = ri[len_at]
        out.append(Decoded(ri[cls_at:cls_at + n], ri[cap:cap + n], rf[2 * cap:2 * cap + n], rf[len_at + 1]))
    return out


def beam_limits():
    """tatt_beam_limits: {'steps', 'classes', 'beam', 'nodes', 'table'}: most steps T, classes C and beam entries of
    tatt_ctc_beam_read, the nodes of a line's prefix trie and the slots of its lookup table.  A host-only entry: needs no GPU."""
    return _limits("tatt_beam_limits", ("steps", "classes", "beam", "nodes", "table"))


def _beam_best_at(doubles: int):
    """(len_at, cls_at, gate_at) of entry 0 of a beam record row whose entries begin with `doubles` float64s (1: the logp; 2: with a
    language model, the logp and the lm): [0] entries written (the gate), [1] flag, then per entry the float64s, the length, a pad
    word, the classes.  The entry sizes, the row parser and the alignment behind a beam launch all read the layout from here."""
    return 2 + 2 * doubles, 2 + 2 * doubles + 2, 0


def _beam_entry_words(cap: int, doubles: int) -> int:
    return _beam_best_at(doubles)[1] - 2 + int(cap) + (int(cap) & 1)


def _parse_beam_rows(what, record, cap: int, nbest: int, doubles: int, decoded):
    """the rows of a beam record (see `parse_beam_records`), `doubles` float64s in front of every entry -> one `decoded` per row, its
    entries (classes, the float64s...)"""
    es, (len_at, cls_at, gate_at), out = _beam_entry_words(cap, doubles), _beam_best_at(doubles), []
    for row in record.tolist():
        n, flag = row[gate_at], row[1]
        if not 0 <= n <= nbest or flag not in (0, 1):
            raise ValueError("%s: no beam record row: entries = %r, flag = %r" % (what, n, flag))
        entries = []
        for i in range(n):
            e = row[2 + i * es:2 + (i + 1) * es]                     # (the offsets are entry 0's in the row: 2 words further)
            entries.append((e[cls_at - 2:cls_at - 2 + e[len_at - 2]],) +
                           struct.unpack("<%dd" % doubles, struct.pack("<%di" % (2 * doubles), *e[:2 * doubles])))
        out.append(decoded(entries, flag))
    return out


def beam_entry_words(cap: int) -> int:
    """32-bit words of one entry of a beam record row: the float64 logp (2), the length, a pad word, then `cap` classes, rounded up to
    an even count so that every entry's logp is 8-byte aligned within the row"""
    return _beam_entry_words(cap, 1)


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
    _check_record("ctc_beam_read", record, index, B)
    _check_beam("ctc_beam_read", beam, nbest, beam_limits()["beam"])
    if record.shape[1] < beam_record_words(cap, nbest):
        raise ValueError("ctc_beam_read: rows of %d words; cap = %d and nbest = %d need %d" % (record.shape[1], cap, nbest,
                                                                                             beam_record_words(cap, nbest)))
    rc = LIB.tatt_ctc_beam_read(ops.P(logits), *logits.stride(), T, B, C, beam, nbest, ops.P(index), ops.P(record), record.shape[0],
                                int(cap), record.stride(0), ops.stream())
    _launched("tatt_ctc_beam_read", rc, "T = %d, C = %d, beam = %d, nbest = %d, cap = %d, rows of %d words",
              T, C, beam, nbest, cap, record.stride(0))
    return record


def parse_beam_records(record, cap: int, nbest: int):
    """record: the (n, >= beam_record_words(cap, nbest)) int32 HOST tensor tatt_ctc_beam_read filled -> one BeamDecoded per row.  Row, in
    32-bit words: [0] entries written (<= nbest)  [1] flag  then per entry, beam_entry_words(cap) words: the float64 logp as it is (low
    word first), the length, a pad word, `cap` classes padded with -1."""
    return _parse_beam_rows("parse_beam_records", record, cap, nbest, 1, BeamDecoded)


def _beam_reading(dec: BeamDecoded, rw: int, squeezed: bool) -> BeamReading:
    d2a = _alphabet()
    alts = [("".join(d2a[c] for c in classes), logp) for classes, logp in dec.entries]
    text, logp = alts[0] if alts else ("", float("nan"))
    return BeamReading(text, logp, alts, rw, squeezed)


def beam_lm_entry_words(cap: int) -> int:
    """32-bit words of one entry of a beam record row with a language model: the float64 logp (2), the float64 lm (2), the length, a
    pad word, then `cap` classes, rounded up to an even count"""
    return _beam_entry_words(cap, 2)


def beam_lm_record_words(cap: int, nbest: int) -> int:
    """32-bit words of such a row for `nbest` entries: [0] entries written, [1] flag, then the entries"""
    return 2 + int(nbest) * beam_lm_entry_words(cap)


def ctc_beam_lm_read(logits, table_dev, order: int, index, record, cap: int, beam: int = 8, nbest: int = 4):
    """ONE tatt_ctc_beam_lm_read launch: `ctc_beam_read` with the increments table of a `CharLM` on the device: table_dev a contiguous
    float64 tensor of C^order entries (`torch.from_numpy(lm.increments(weight, bonus))`, flat or in its own shape), record
    (n_rows, >= beam_lm_record_words(cap, nbest)) int32 (see `parse_beam_lm_records`).  ValueError for what the entry refuses (what
    `ctc_beam_read` refuses, an order outside lm_limits(), a table whose class count differs from the logits', the row width), before
    any launch."""
    from . import ops
    from ._lib import LIB
    ops._check_dev(logits)
    T, B, C = logits.shape
    _check_record("ctc_beam_lm_read", record, index, B)
    _check_beam("ctc_beam_lm_read", beam, nbest, beam_limits()["beam"])
    lim = lm_limits()
    if not (isinstance(order, int) and 1 <= order <= lim["order"]):
        raise ValueError("ctc_beam_lm_read: an order of 1 .. %d expected; got %r" % (lim["order"], order))
    if not (isinstance(table_dev, torch.Tensor) and table_dev.dtype == torch.float64 and table_dev.is_contiguous() and
            table_dev.device == logits.device and table_dev.numel() > 0):
        raise ValueError("ctc_beam_lm_read: the table is a contiguous float64 tensor on %s" % (logits.device,))
    classes = next((k for k in range(1, lim["classes"] + 1) if k ** order == table_dev.numel()), 0)
    if classes != C or (table_dev.dim() > 1 and tuple(table_dev.shape) != (C,) * order):
        raise ValueError("ctc_beam_lm_read: a table of %s entries at order %d is none for the %d classes of the logits"
                         % (tuple(table_dev.shape), order, C))
    if record.shape[1] < beam_lm_record_words(cap, nbest):
        raise ValueError("ctc_beam_lm_read: rows of %d words; cap = %d and nbest = %d need %d" % (record.shape[1], cap, nbest,
                                                                                                beam_lm_record_words(cap, nbest)))
    rc = LIB.tatt_ctc_beam_lm_read(ops.P(logits), *logits.stride(), T, B, C, beam, nbest, ops.P(table_dev), order, classes, ops.P(index),
                                   ops.P(record), record.shape[0], int(cap), record.stride(0), ops.stream())
    _launched("tatt_ctc_beam_lm_read", rc, "T = %d, C = %d, beam = %d, nbest = %d, order = %d, cap = %d, rows of %d words",
              T, C, beam, nbest, order, cap, record.stride(0))
    return record


def parse_beam_lm_records(record, cap: int, nbest: int):
    """record: the (n, >= beam_lm_record_words(cap, nbest)) int32 HOST tensor tatt_ctc_beam_lm_read filled -> one BeamLMDecoded per row.
    Row, in 32-bit words: [0] entries written (<= nbest)  [1] flag  then per entry, beam_lm_entry_words(cap) words: the float64 logp
    (the acoustic mass) and the float64 lm (the LM term with the end term) as they are, low word first, the length, a pad word, `cap`
    classes padded with -1."""
    return _parse_beam_rows("parse_beam_lm_records", record, cap, nbest, 2, BeamLMDecoded)


def _beam_lm_reading(dec: BeamLMDecoded, rw: int, squeezed: bool) -> BeamLMReading:
    d2a = _alphabet()
    alts = [("".join(d2a[c] for c in classes), logp, lm) for classes, logp, lm in dec.entries]
    text, logp, lm = alts[0] if alts else ("", float("nan"), float("nan"))
    return BeamLMReading(text, logp, lm, logp + lm, alts, rw, squeezed)


PATTERN_MASS_WORDS = 4    # 32-bit words tatt_ctc_pattern_mass writes per line: the float64 mass (2), the flag, 0


def pattern_record_words(cap: int, nbest: int) -> int:
    """32-bit words of a record row of `LineReader(pattern=...)`: the beam record row (an even count of words: the plain search's) and
    the PATTERN_MASS_WORDS of the mass behind it"""
    return beam_record_words(cap, nbest) + PATTERN_MASS_WORDS


def _check_pattern(what, pattern, C):
    if not isinstance(pattern, Pattern):
        raise ValueError("%s: pattern is a Pattern; got %r" % (what, type(pattern).__name__))
    lim = pattern_limits()
    if pattern.n_states > lim["states"] or pattern.n_classes > lim["classes"]:
        raise ValueError("%s: a pattern of %d states over %d classes; at most %d and %d" % (what, pattern.n_states, pattern.n_classes,
                                                                                            lim["states"], lim["classes"]))
    if pattern.n_classes > C:
        raise ValueError("%s: the pattern's alphabet has %d classes, the logits %d" % (what, pattern.n_classes, C))


def ctc_beam_pattern_read(logits, pattern: Pattern, index, record, cap: int, beam: int = 8, nbest: int = 4):
    """ONE tatt_ctc_beam_pattern_read launch: `ctc_beam_read` held to the format `pattern` (its table and accepting states are uploaded
    once per device); record and index as `ctc_beam_read` takes them, the rows are read by `parse_beam_records`.  Specification
    `ctc_beam_pattern_read_host`.  ValueError for what the entry refuses and for an alphabet with more classes than the logits, before
    any launch."""
    from . import ops
    from ._lib import LIB
    ops._check_dev(logits)
    T, B, C = logits.shape
    _check_record("ctc_beam_pattern_read", record, index, B)
    _check_beam("ctc_beam_pattern_read", beam, nbest, pattern_limits()["beam"])
    _check_pattern("ctc_beam_pattern_read", pattern, C)
    if record.shape[1] < beam_record_words(cap, nbest):
        raise ValueError("ctc_beam_pattern_read: rows of %d words; cap = %d and nbest = %d need %d" % (record.shape[1], cap, nbest,
                                                                                                     beam_record_words(cap, nbest)))
    table, accept = pattern.device(logits.device, C)
    rc = LIB.tatt_ctc_beam_pattern_read(ops.P(logits), *logits.stride(), T, B, C, beam, nbest, ops.P(table), ops.P(accept), pattern.n_states,
                                        ops.P(index), ops.P(record), record.shape[0], int(cap), record.stride(0), ops.stream())
    _launched("tatt_ctc_beam_pattern_read", rc, "T = %d, C = %d, beam = %d, nbest = %d, S = %d, cap = %d, rows of %d words",
              T, C, beam, nbest, pattern.n_states, cap, record.stride(0))
    return record


def ctc_pattern_mass(logits, pattern: Pattern, index, out):
    """ONE tatt_ctc_pattern_mass launch: logits (T, B, C) fp32 on the device (any strides), index (B,) int32 on the device: the row of
    every line, out (n_rows, >= PATTERN_MASS_WORDS) int32 on the device, its rows contiguous (a view of the columns of a wider buffer
    will do): line b writes the float64 mass, its flag and a 0 (see `parse_pattern_mass`).  Specification `ctc_pattern_mass_host`.
    ValueError for what the entry refuses and for an alphabet with more classes than the logits, before any launch."""
    from . import ops
    from ._lib import LIB
    ops._check_dev(logits)
    T, B, C = logits.shape
    if out.dtype != torch.int32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[1] < PATTERN_MASS_WORDS or out.device != logits.device \
            or index.dtype != torch.int32 or index.numel() < B:
        raise ValueError("ctc_pattern_mass: out must be a 2-D int32 tensor with contiguous rows of at least %d words on %s, index an "
                         "int32 tensor of B entries" % (PATTERN_MASS_WORDS, logits.device))
    _check_pattern("ctc_pattern_mass", pattern, C)
    table, accept = pattern.device(logits.device, C)
    rc = LIB.tatt_ctc_pattern_mass(ops.P(logits), *logits.stride(), T, B, C, ops.P(table), ops.P(accept), pattern.n_states, ops.P(index),
                                   ops.P(out), out.shape[0], out.stride(0), ops.stream())
    _launched("tatt_ctc_pattern_mass", rc, "T = %d, B = %d, C = %d, S = %d, rows of %d words", T, B, C, pattern.n_states, out.stride(0))
    return out


def parse_pattern_mass(out):
    """out: the (n, >= PATTERN_MASS_WORDS) int32 HOST tensor tatt_ctc_pattern_mass filled -> one PatternMass per row"""
    res = []
    for row in out.tolist():
        if row[2] not in (0, 1):
            raise ValueError("parse_pattern_mass: no mass row: flag = %r" % (row[2],))
        res.append(PatternMass(struct.unpack("<d", struct.pack("<ii", row[0], row[1]))[0], row[2]))
    return res


def _pattern_reading(dec: BeamDecoded, mass: PatternMass, alphabet, rw: int, squeezed: bool) -> PatternReading:
    nan = float("nan")
    m = nan if mass.flag or dec.flag else mass.mass
    alts = [("".join(alphabet[c] for c in classes), logp, math.exp(logp - m)) for classes, logp in dec.entries]
    text, logp, post = alts[0] if alts else ("", nan, nan)
    return PatternReading(text, logp, m, post, alts, rw, squeezed)


def lexicon_limits():
    """tatt_lexicon_limits: {'steps', 'classes', 'length', 'words', 'nbest'}: most steps T and classes C of tatt_ctc_lexicon_score, the
    longest word and most words of a lexicon, most entries of tatt_ctc_lexicon_select.  A host-only entry: needs no GPU."""
    return _limits("tatt_lexicon_limits", ("steps", "classes", "length", "words", "nbest"))


def lexicon_record_words(nbest: int) -> int:
    """32-bit words of a lexicon record row for `nbest` entries: [0] entries written, [1] flag, [2:4] logz, then 4 words per entry"""
    return 4 + 4 * int(nbest)


def _check_nbest(what, nbest):
    if not (isinstance(nbest, int) and 1 <= nbest <= lexicon_limits()["nbest"]):
        raise ValueError("%s: 1 <= nbest <= %d expected; got nbest = %r" % (what, lexicon_limits()["nbest"], nbest))


def ctc_lexicon_score(logits, lexicon: Lexicon, scores):
    """The tatt_ctc_lexicon_score launches (one per non-empty segment class of the lexicon, at most three): logits (T, B, C) fp32 on
    the device (any strides), scores (B, K) float64 on the device with contiguous rows: scores[b][k] = the exact CTC log-probability
    of lexicon.words[k] on line b (specification `ctc_lexicon_scores_host`; NaN on every word of a flagged line).  ValueError for what
    the entry refuses (T, C, B), before any launch."""
    from . import ops
    from ._lib import LIB
    ops._check_dev(logits)
    T, B, C = logits.shape
    K = len(lexicon)
    if scores.dtype != torch.float64 or scores.dim() != 2 or scores.stride(1) != 1 or tuple(scores.shape) != (B, K) or \
            scores.device != logits.device:
        raise ValueError("ctc_lexicon_score: scores must be a (%d, %d) float64 tensor with contiguous rows on %s" % (B, K, logits.device))
    if lexicon.n_classes > C:
        raise ValueError("ctc_lexicon_score: the lexicon's alphabet has %d classes, the logits %d" % (lexicon.n_classes, C))
    codes, table = lexicon.device(logits.device)
    rc = LIB.tatt_ctc_lexicon_score(ops.P(logits), *logits.stride(), T, B, C, ops.P(codes), lexicon.n_codes, ops.P(table), K,
                                    *lexicon.counts, ops.P(scores), scores.stride(0), ops.stream())
    _launched("tatt_ctc_lexicon_score", rc, "T = %d, B = %d, C = %d, K = %d", T, B, C, K)
    return scores


def _check_select(what, scores, index, record, nbest, counts=None):
    """the argument checks of `ctc_lexicon_select` and, given counts, of `ctc_lexicon_select_rows` -> scores.shape"""
    if not scores.is_cuda:
        raise RuntimeError("tatt_amd kernels need tensors on an AMD GPU (HIP device); got %s. There is no CPU fallback in the product "
                           "path." % scores.device)
    if scores.dtype != torch.float64 or scores.dim() != 2 or scores.stride(1) != 1 or (counts is not None and scores.shape[1] < 1):
        raise ValueError("%s: scores must be a 2-D float64 tensor with contiguous%s rows" % (what, "" if counts is None else ", non-empty"))
    B = scores.shape[0]
    if counts is not None:
        _int32_on(what, "counts", counts, scores.device)
        if counts.numel() != B:
            raise ValueError("%s: %d counts for %d lines" % (what, counts.numel(), B))
    _check_record(what, record, index, B)
    _check_nbest(what, nbest)
    if record.shape[1] < lexicon_record_words(nbest):
        raise ValueError("%s: rows of %d words; nbest = %d needs %d" % (what, record.shape[1], nbest, lexicon_record_words(nbest)))
    return scores.shape


def ctc_lexicon_select(scores, index, record, nbest: int = 4):
    """ONE tatt_ctc_lexicon_select launch: scores (B, K) float64 on the device with contiguous rows, index (B,) int32 on the device:
    the record row of every line, record (n_rows, >= lexicon_record_words(nbest)) int32 on the device, rows contiguous (see
    `parse_lexicon_records`).  ValueError for what the entry refuses, before any launch."""
    from . import ops
    from ._lib import LIB
    B, K = _check_select("ctc_lexicon_select", scores, index, record, nbest)
    rc = LIB.tatt_ctc_lexicon_select(ops.P(scores), scores.stride(0), B, K, nbest, ops.P(index), ops.P(record), record.shape[0],
                                     record.stride(0), ops.stream())
    _launched("tatt_ctc_lexicon_select", rc, "B = %d, K = %d, nbest = %d, rows of %d words", B, K, nbest, record.stride(0))
    return record


def parse_lexicon_records(record, nbest: int):
    """record: the (n, >= lexicon_record_words(nbest)) int32 HOST tensor tatt_ctc_lexicon_select filled -> one LexiconDecoded per row.
    Row, in 32-bit words: [0] entries written (<= nbest)  [1] flag  [2:4] the float64 logz as it is (low word first)  then per entry 4
    words: the float64 logp, the word's index, 0."""
    f64 = lambda lo, hi: struct.unpack("<d", struct.pack("<ii", lo, hi))[0]
    out = []
    for row in record.tolist():
        n, flag = row[0], row[1]
        if not 0 <= n <= nbest or flag not in (0, 1) or len(row) < lexicon_record_words(nbest):
            raise ValueError("parse_lexicon_records: no lexicon record row: entries = %r, flag = %r" % (n, flag))
        out.append(LexiconDecoded([(row[6 + 4 * i], f64(row[4 + 4 * i], row[5 + 4 * i])) for i in range(n)], f64(row[2], row[3]), flag))
    return out


def _lexicon_reading(dec: LexiconDecoded, lexicon: Lexicon, rw: int, squeezed: bool) -> LexiconReading:
    return _line_lexicon_reading(dec, lexicon.words, rw, squeezed)


def _line_lexicon_reading(dec: LexiconDecoded, words, rw: int, squeezed: bool) -> LexiconReading:
    """a decoded line as the caller sees it; words: the list the line was read against (a `Lexicon`'s, or the line's own)"""
    alts = [(words[k], logp, math.exp(logp - dec.logz)) for k, logp in dec.entries]
    text, logp, post = alts[0] if alts else ("", float("nan"), float("nan"))
    return LexiconReading(text, logp, post, alts, rw, squeezed)


def line_lexicons_limits():
    """tatt_line_lexicons_limits: {'steps', 'classes', 'length', 'words', 'union', 'nbest'}: `lexicon_limits()` with `words` the most
    words of ONE line's list and `union` the most distinct words of all lists.  A host-only entry: needs no GPU."""
    return _limits("tatt_line_lexicons_limits", ("steps", "classes", "length", "words", "union", "nbest"))


def _int32_on(what, name, t, device, cols=None):
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.int32 and t.device == device and t.is_contiguous() and
            (t.dim() == 1 if cols is None else t.dim() == 2 and t.shape[1] == cols)):
        raise ValueError("%s: %s must be a contiguous int32 tensor%s on %s" % (what, name, "" if cols is None else " of %d columns" % cols,
                                                                               device))


def ctc_lexicon_score_pairs(logits, codes, n_codes: int, table, tiles, pairs, counts, scores, max_count: int):
    """ONE tatt_ctc_lexicon_score_pairs launch: logits (T, B, C) fp32 on the device (any strides); codes, table: the packed union of a
    `LineLexicons` on the device (n_codes its code count); tiles (n_tiles, 4), pairs (n_pairs, 2), counts (B,): what
    `LineLexicons.pack` gave for the B lines, on the device; scores (B, >= max_count) float64 on the device with contiguous rows,
    max_count >= every count: scores[b][j] = the exact CTC log-probability of word j of line b's own list (NaN on a flagged line).
    Only the listed pairs are written.  ValueError for what the entry refuses, before any launch."""
    from . import ops
    from ._lib import LIB
    what = "ctc_lexicon_score_pairs"
    ops._check_dev(logits)
    if logits.dim() != 3:
        raise ValueError("%s takes (T, B, C) logits; got %s" % (what, tuple(logits.shape)))
    T, B, C = logits.shape
    dev = logits.device
    _int32_on(what, "codes", codes, dev)
    _int32_on(what, "table", table, dev, 4)
    _int32_on(what, "tiles", tiles, dev, 4)
    _int32_on(what, "pairs", pairs, dev, 2)
    _int32_on(what, "counts", counts, dev)
    if not (isinstance(n_codes, int) and 0 <= n_codes <= codes.numel() and codes.numel() >= 1 and table.shape[0] >= 1):
        raise ValueError("%s: n_codes = %r for %d codes" % (what, n_codes, codes.numel()))
    if counts.numel() != B:
        raise ValueError("%s: %d counts for %d lines" % (what, counts.numel(), B))
    if not (isinstance(max_count, int) and max_count >= 1):
        raise ValueError("%s: max_count >= 1 expected; got %r" % (what, max_count))
    if scores.dtype != torch.float64 or scores.dim() != 2 or scores.stride(1) != 1 or scores.shape[0] != B or scores.shape[1] < max_count \
            or scores.device != dev:
        raise ValueError("%s: scores must be a (%d, >= %d) float64 tensor with contiguous rows on %s" % (what, B, max_count, dev))
    rc = LIB.tatt_ctc_lexicon_score_pairs(ops.P(logits), *logits.stride(), T, B, C, ops.P(codes), n_codes, ops.P(table), table.shape[0],
                                          ops.P(tiles), tiles.shape[0], ops.P(pairs), pairs.shape[0], ops.P(counts), max_count,
                                          ops.P(scores), scores.stride(0), ops.stream())
    _launched("tatt_ctc_lexicon_score_pairs", rc, "T = %d, B = %d, C = %d, U = %d, %d tiles, %d pairs, max_count = %d",
              T, B, C, table.shape[0], tiles.shape[0], pairs.shape[0], max_count)
    return scores


def ctc_lexicon_select_rows(scores, counts, index, record, nbest: int = 4):
    """ONE tatt_ctc_lexicon_select_rows launch: `ctc_lexicon_select` with counts (B,) int32 on the device: line b has counts[b] <=
    scores.shape[1] scores.  A line without words writes entries = 0, flag = 0, logz = -inf.  ValueError for what the entry refuses,
    before any launch."""
    from . import ops
    from ._lib import LIB
    B = _check_select("ctc_lexicon_select_rows", scores, index, record, nbest, counts)[0]
    rc = LIB.tatt_ctc_lexicon_select_rows(ops.P(scores), scores.stride(0), B, ops.P(counts), nbest, ops.P(index), ops.P(record),
                                          record.shape[0], record.stride(0), ops.stream())
    _launched("tatt_ctc_lexicon_select_rows", rc, "B = %d, nbest = %d, rows of %d words", B, nbest, record.stride(0))
    return record


def words_limits():
    """tatt_words_limits: {'steps', 'classes', 'lanes', 'threads', 'slots'}: most steps T and classes C of tatt_ctc_words_read, the most
    packed lanes of a lexicon (`words_lanes`), the threads of a work-group and the lanes a thread holds at that limit.  A host-only
    entry: needs no GPU."""
    return _limits("tatt_words_limits", ("steps", "classes", "lanes", "threads", "slots"))


def words_lanes(lexicon: Lexicon) -> int:
    """the packed lanes tatt_ctc_words_read lays the lexicon over: 16, 32 or 64 per word by its segment class, every class starting at
    a multiple of 64 (a word's 2 L - 1 states run in the segment that holds the 2 L + 1 of lexicon decoding)"""
    k16, k32, k64 = lexicon.counts
    return -(-16 * k16 // 64) * 64 + -(-32 * k32 // 64) * 64 + 64 * k64


def _check_lanes(what, lexicon: Lexicon):
    lanes, limit = words_lanes(lexicon), words_limits()["lanes"]
    if lanes > limit:
        raise ValueError("%s: the lexicon needs %d lanes (%d, %d, %d words in segments of 16, 32, 64); decode='words' takes at most %d"
                         % ((what, lanes) + tuple(lexicon.counts) + (limit,)))


def words_record_words(cap: int) -> int:
    """32-bit words of a words record row for lines of at most `cap` steps: [0] words written, [1] flag, [2:4] logp, then 2 per word"""
    return 4 + 2 * int(cap)


def ctc_words_read(logits, lexicon: Lexicon, index, record, cap: int, word_penalty: float = 0.0, lp_out=None):
    """ONE tatt_ctc_words_read launch: logits (T, B, C) fp32 on the device (any strides), index (B,) int32 on the device: the record
    row of every line, record (n_rows, >= words_record_words(cap)) int32 on the device, rows contiguous, cap >= T (see
    `parse_words_records`); lp_out: None or a (B, T, C) float64 tensor on the device, every line contiguous, which receives the
    log-soft-max the decoding ran on.  Specification `ctc_words_read_host`.  ValueError for what the entry refuses, before any launch."""
    from . import ops
    from ._lib import LIB
    ops._check_dev(logits)
    T, B, C = logits.shape
    _check_record("ctc_words_read", record, index, B)
    wp = _check_penalty("ctc_words_read", word_penalty)
    if lexicon.n_classes > C:
        raise ValueError("ctc_words_read: the lexicon's alphabet has %d classes, the logits %d" % (lexicon.n_classes, C))
    _check_lanes("ctc_words_read", lexicon)
    if record.shape[1] < words_record_words(cap):
        raise ValueError("ctc_words_read: rows of %d words; cap = %d needs %d" % (record.shape[1], cap, words_record_words(cap)))
    st_lp = 0
    if lp_out is not None:
        if lp_out.dtype != torch.float64 or tuple(lp_out.shape) != (B, T, C) or lp_out.stride(2) != 1 or lp_out.stride(1) != C or \
                lp_out.device != logits.device:
            raise ValueError("ctc_words_read: lp_out must be a (%d, %d, %d) float64 tensor with contiguous lines on %s"
                             % (B, T, C, logits.device))
        st_lp = lp_out.stride(0)
    codes, table = lexicon.device(logits.device)
    rc = LIB.tatt_ctc_words_read(ops.P(logits), *logits.stride(), T, B, C, ops.P(codes), lexicon.n_codes, ops.P(table), len(lexicon),
                                 *lexicon.counts, wp, ops.P(index), ops.P(record), record.shape[0], int(cap), record.stride(0),
                                 ops.P(lp_out), st_lp, ops.stream())
    _launched("tatt_ctc_words_read", rc, "T = %d, B = %d, C = %d, K = %d, cap = %d, rows of %d words",
              T, B, C, len(lexicon), cap, record.stride(0))
    return record


def parse_words_records(record, cap: int):
    """record: the (n, >= words_record_words(cap)) int32 HOST tensor tatt_ctc_words_read filled -> one WordsDecoded per row.  Row, in
    32-bit words: [0] words written (<= cap)  [1] flag  [2:4] the float64 logp as it is (low word first)  then per word 2 words: the
    caller's word index, first | last << 16."""
    out = []
    for row in record.tolist():
        n, flag = row[0], row[1]
        if not 0 <= n <= cap or flag not in (0, 1) or len(row) < words_record_words(cap):
            raise ValueError("parse_words_records: no words record row: words = %r, flag = %r" % (n, flag))
        logp = struct.unpack("<d", struct.pack("<ii", row[2], row[3]))[0]
        out.append(WordsDecoded([(row[4 + 2 * i], row[5 + 2 * i] & 0xffff, (row[5 + 2 * i] >> 16) & 0xffff) for i in range(n)], logp, flag))
    return out


def align_limits():
    """tatt_align_limits: {'steps', 'classes', 'length'}: most steps T and classes C of tatt_ctc_align and the longest string it
    aligns (2 length + 1 states, one thread each).  A host-only entry: needs no GPU."""
    return _limits("tatt_align_limits", ("steps", "classes", "length"))


def ctc_align(logits, index, src, len_at: int, cls_at: int, gate_at: int, record, rec_at: int, cap_len: int, lp_out=None):
    """ONE tatt_ctc_align launch: logits (T, B, C) fp32 on the device (any strides), index (B,) int32 on the device: the row of every
    line in `src` AND in `record`.  src: a 2-D int32 tensor on the device with contiguous rows, at least as many as `record`; line j's
    string has its length at word len_at of row index[j], its classes from word cls_at, and -- gate_at >= 0 -- a word that must be >= 1
    for a string to exist (-1: none).  src may be `record` itself (the row a decode launch wrote) or a table of `pack_strings`
    (len_at = 0, cls_at = 2, gate_at = -1).  record: (n_rows, >= rec_at + align_record_words(cap_len)) int32 on the device, rows
    contiguous with an even stride, rec_at even (see `parse_align_records`); lp_out: None or a contiguous (B, T, C) float64 tensor on the
    device, which receives the log-soft-max the alignment ran on.  Specification `ctc_align_read_host`.  ValueError for what the entry
    refuses (T, C or cap_len beyond align_limits() included: never truncated), before any launch."""
    from . import ops
    from ._lib import LIB
    ops._check_dev(logits)
    T, B, C = logits.shape
    _check_record("ctc_align", record, index, B)
    if not (isinstance(src, torch.Tensor) and src.dtype == torch.int32 and src.dim() == 2 and src.stride(1) == 1 and
            src.device == logits.device and record.device == logits.device and index.device == logits.device):
        raise ValueError("ctc_align: src must be a 2-D int32 tensor with contiguous rows on %s, like record and index" % (logits.device,))
    lim = align_limits()
    if not all(isinstance(v, int) for v in (len_at, cls_at, gate_at, rec_at, cap_len)):
        raise ValueError("ctc_align: len_at, cls_at, gate_at, rec_at and cap_len are ints")
    if not 0 <= cap_len <= lim["length"]:
        raise ValueError("ctc_align: cap_len = %d; strings of at most %d characters are aligned" % (cap_len, lim["length"]))
    if T > lim["steps"] or C > lim["classes"] or C < 2:
        raise ValueError("ctc_align: T = %d, C = %d; at most %d steps and 2 .. %d classes" % (T, C, lim["steps"], lim["classes"]))
    if rec_at < 0 or rec_at % 2 or record.stride(0) % 2 or record.shape[1] < rec_at + align_record_words(cap_len):
        raise ValueError("ctc_align: rows of %d words (stride %d); an even rec_at = %d and cap_len = %d need %d and an even stride"
                         % (record.shape[1], record.stride(0), rec_at, cap_len, rec_at + align_record_words(cap_len)))
    if src.shape[0] < record.shape[0] or not 0 <= len_at < src.shape[1] or not -1 <= gate_at < src.shape[1] or cls_at < 0 or \
            cls_at + cap_len > src.shape[1]:
        raise ValueError("ctc_align: src of %s; len_at = %d, cls_at = %d, gate_at = %d, cap_len = %d and %d record rows do not fit it"
                         % (tuple(src.shape), len_at, cls_at, gate_at, cap_len, record.shape[0]))
    if lp_out is not None and (lp_out.dtype != torch.float64 or tuple(lp_out.shape) != (B, T, C) or not lp_out.is_contiguous() or
                               lp_out.device != logits.device):
        raise ValueError("ctc_align: lp_out must be a contiguous (%d, %d, %d) float64 tensor on %s" % (B, T, C, logits.device))
    rc = LIB.tatt_ctc_align(ops.P(logits), *logits.stride(), T, B, C, ops.P(index), ops.P(src), src.shape[0], src.stride(0), len_at,
                            cls_at, gate_at, ops.P(record), record.shape[0], record.stride(0), rec_at, cap_len, ops.P(lp_out),
                            ops.stream())
    _launched("tatt_ctc_align", rc, "T = %d, B = %d, C = %d, cap_len = %d, rec_at = %d, rows of %d words",
              T, B, C, cap_len, rec_at, record.stride(0))
    return record


# ---- the decodings of a LineReader ------------------------------------------------------------------------------------------------------
class _ReadState:
    """What one `read` holds for its decoding besides the record: `scores` / `lp`: the score and log-soft-max buffers of its chunks
    (None: not kept); decode="lexicons" only: `lexicons` the call's LineLexicons, `union` its codes and table on the device, `chunks`
    an iterator over (tiles, pairs, counts, most words of a line) per chunk, in the order the chunks are launched."""

    def __init__(self, scores=None, lp=None):
        self.scores, self.lp, self.lexicons, self.union, self.chunks = scores, lp, None, None, None


def _lp_buffer(kept_lp, lines, logits):
    """the (n, T, C) float64 buffer a launch leaves its log-soft-max in, kept with the chunk's line indices; None where none is kept"""
    if kept_lp is None:
        return None
    T, n, C = logits.shape
    lp = torch.empty(n, T, C, dtype=torch.float64, device=logits.device)
    kept_lp.append((lines, lp))
    return lp


class _Decoding:
    """One decoding of `LineReader`: what it was made with, the layout of its record row, its launches and its parser, in one place.
    `_reader_decoding` makes it from the reader's keywords.  Every launch goes through this module's globals at call time.
    record_words(cap): 32-bit words of its record row for lines of at most `cap` steps.  align_source(cap): (len_at, cls_at, gate_at)
    of the best string in that row; None: the row holds word indices, nothing to locate.  upload(device, emits): the one upload of what
    its launches read on the device (no `read` makes it).  launch(logits (T, n, C), index: the record rows of the chunk's lines, record,
    cap, lines: their input indices, state): the decode launch(es) of one chunk.  readings(host, cap, plan, state): the host record of a
    call -> one reading per line, in input order."""
    keeps_scores = keeps_lp = False
    alphabet = property(lambda self: _alphabet())                    # of the classes in its record: what `locations()` spells with
    align_source = upload = lambda self, *args: None

    def __init__(self, beam, nbest, lexicon=None, word_penalty=0.0, lm=None, lm_weight=None, lm_bonus=None, lm_table=None, pattern=None):
        self.beam, self.nbest, self.lexicon, self.word_penalty, self.pattern = beam, nbest, lexicon, word_penalty, pattern
        self.lm, self.lm_weight, self.lm_bonus, self.lm_table = lm, lm_weight, lm_bonus, lm_table

    def begin(self, reader, plan, chunk: int, lexicons) -> _ReadState:
        """the state of one call, made after the luma launch and before the first chunk"""
        return _ReadState([] if self.keeps_scores and reader.keep_scores else None,
                          [] if (self.keeps_lp or reader.locate) and reader.keep_lp else None)


class _Greedy(_Decoding):
    record_words = lambda self, cap: 3 * int(cap) + 2
    align_source = lambda self, cap: _greedy_best_at(cap)

    def launch(self, logits, index, record, cap, lines, state):
        ctc_greedy_read(logits, index, record, cap)

    def readings(self, host, cap, plan, state):
        return [_reading(d, rw, sq) for d, rw, sq in zip(parse_records(host, cap), plan.rws, plan.squeezed)]


class _Beam(_Decoding):
    record_words = lambda self, cap: beam_record_words(cap, self.nbest)
    align_source = lambda self, cap: _beam_best_at(1)

    def launch(self, logits, index, record, cap, lines, state):
        ctc_beam_read(logits, index, record, cap, self.beam, self.nbest)

    def readings(self, host, cap, plan, state):
        return [_beam_reading(d, rw, sq) for d, rw, sq in zip(parse_beam_records(host, cap, self.nbest), plan.rws, plan.squeezed)]


class _BeamLM(_Decoding):
    record_words = lambda self, cap: beam_lm_record_words(cap, self.nbest)
    align_source = lambda self, cap: _beam_best_at(2)

    def upload(self, device, emits):
        self.lm_table = torch.from_numpy(self.lm_table).to(device)

    def launch(self, logits, index, record, cap, lines, state):
        ctc_beam_lm_read(logits, self.lm_table, self.lm.order, index, record, cap, self.beam, self.nbest)

    def readings(self, host, cap, plan, state):
        return [_beam_lm_reading(d, rw, sq) for d, rw, sq in zip(parse_beam_lm_records(host, cap, self.nbest), plan.rws, plan.squeezed)]


class _BeamPattern(_Beam):
    """the beam row of `_Beam`, held to the format, and the format's mass behind it"""
    alphabet = property(lambda self: self.pattern.alphabet)
    record_words = lambda self, cap: pattern_record_words(cap, self.nbest)
    upload = lambda self, device, emits: self.pattern.device(device, emits)

    def launch(self, logits, index, record, cap, lines, state):
        ctc_beam_pattern_read(logits, self.pattern, index, record, cap, self.beam, self.nbest)
        ctc_pattern_mass(logits, self.pattern, index, record[:, beam_record_words(cap, self.nbest):])

    def readings(self, host, cap, plan, state):
        at = beam_record_words(cap, self.nbest)
        return [_pattern_reading(d, m, self.pattern.alphabet, rw, sq) for d, m, rw, sq in zip(
            parse_beam_records(host, cap, self.nbest), parse_pattern_mass(host[:, at:]), plan.rws, plan.squeezed)]


class _Lexicon(_Decoding):
    keeps_scores = True
    record_words = lambda self, cap: lexicon_record_words(self.nbest)
    upload = lambda self, device, emits: self.lexicon.device(device)

    def launch(self, logits, index, record, cap, lines, state):
        scores = torch.empty(logits.shape[1], len(self.lexicon), dtype=torch.float64, device=logits.device)
        ctc_lexicon_score(logits, self.lexicon, scores)
        ctc_lexicon_select(scores, index, record, self.nbest)
        if state.scores is not None:
            state.scores.append((lines, scores))

    def readings(self, host, cap, plan, state):
        return [_lexicon_reading(d, self.lexicon, rw, sq) for d, rw, sq in zip(parse_lexicon_records(host, self.nbest), plan.rws,
                                                                                plan.squeezed)]


class _Words(_Decoding):
    keeps_lp = True
    record_words = lambda self, cap: words_record_words(cap)
    upload = lambda self, device, emits: self.lexicon.device(device)

    def launch(self, logits, index, record, cap, lines, state):
        ctc_words_read(logits, self.lexicon, index, record, cap, self.word_penalty, _lp_buffer(state.lp, lines, logits))

    def readings(self, host, cap, plan, state):
        return [_words_reading(d, self.lexicon, rw, sq, int(W)) for d, rw, sq, W in zip(parse_words_records(host, cap), plan.rws,
                                                                                         plan.squeezed, plan.desc[:, 2])]


class _LineLexicons(_Decoding):
    keeps_scores = True
    record_words = lambda self, cap: lexicon_record_words(self.nbest)

    def begin(self, reader, plan, chunk, lexicons):
        """the union and every chunk's tile table, pairs and counts: ONE int32 blob, one copy from pinned memory"""
        state = super().begin(reader, plan, chunk, lexicons)
        parts, spans, at = [lexicons.codes, lexicons.table.reshape(-1)], [], lexicons.codes.size + lexicons.table.size
        for _, idx in plan.buckets:                                  # (lists go by INPUT index, chunks in bucket order)
            for i in range(0, len(idx), chunk):
                tiles, pairs, counts = lexicons.pack(idx[i:i + chunk])
                spans.append((at, at + tiles.size, at + tiles.size + pairs.size, at + tiles.size + pairs.size + counts.size,
                              max(1, int(counts.max()))))
                parts += [tiles.reshape(-1), pairs.reshape(-1), counts]
                at = spans[-1][3]
        blob = torch.empty(at, dtype=torch.int32, pin_memory=True)
        blob.numpy()[:] = np.concatenate(parts)
        dev = torch.empty(at, dtype=torch.int32, device=reader.device)
        dev.copy_(blob, non_blocking=True)
        state.lexicons = lexicons
        state.union = dev[:lexicons.codes.size], dev[lexicons.codes.size:spans[0][0]].view(-1, 4)
        state.chunks = iter([(dev[a:b].view(-1, 4), dev[b:c].view(-1, 2), dev[c:d], most) for a, b, c, d, most in spans])
        return state

    def launch(self, logits, index, record, cap, lines, state):
        tiles, pairs, counts, most = next(state.chunks)
        scores = torch.empty(logits.shape[1], most, dtype=torch.float64, device=logits.device)
        if tiles.shape[0]:                                           # (a chunk of empty lists has nothing to score)
            codes, table = state.union
            ctc_lexicon_score_pairs(logits, codes, state.lexicons.n_codes, table, tiles, pairs, counts, scores, most)
        ctc_lexicon_select_rows(scores, counts, index, record, self.nbest)
        if state.scores is not None:
            state.scores.append((lines, scores, counts))

    def readings(self, host, cap, plan, state):
        return [_line_lexicon_reading(d, ws, rw, sq) for d, ws, rw, sq in zip(parse_lexicon_records(host, self.nbest), state.lexicons.lists,
                                                                              plan.rws, plan.squeezed)]


def _reader_decoding(decode, beam, nbest, lexicon, word_penalty, lm, lm_weight, lm_bonus, pattern, locate, emits) -> _Decoding:
    """The keywords of `LineReader` and `emits`, the classes its CRNN emits (None: it does not say) -> the decoding; ValueError for
    every combination the reader refuses.  Touches no device.  A new decoding is one subclass of `_Decoding` and one line here."""
    if decode not in ("greedy", "beam", "lexicon", "words", "lexicons"):
        raise ValueError("LineReader: decode is 'greedy', 'beam', 'lexicon', 'words' or 'lexicons'; got %r" % (decode,))
    if locate and decode not in ("greedy", "beam"):
        raise ValueError("LineReader: locate=True goes with decode='greedy' or decode='beam' (their records hold the classes of "
                         "the string; those of %r hold word indices)" % (decode,))
    word_penalty = _check_penalty("LineReader", word_penalty)
    if decode != "words" and word_penalty != 0.0:
        raise ValueError("LineReader: word_penalty= goes with decode='words'; got decode = %r" % (decode,))
    if decode == "lexicons":
        _check_nbest("LineReader", nbest)
        if lexicon is not None:
            raise ValueError("LineReader: lexicon= goes with decode='lexicon' or decode='words'; decode='lexicons' takes the lists "
                             "of a call as read(..., lexicons=)")
    elif decode in ("lexicon", "words"):
        if decode == "lexicon":
            _check_nbest("LineReader", nbest)
        if lexicon is None:
            raise ValueError("LineReader: decode=%r needs lexicon=, a Lexicon or a list of words" % (decode,))
        lexicon = lexicon if isinstance(lexicon, Lexicon) else Lexicon(lexicon)
        if emits is not None and lexicon.n_classes > emits:
            raise ValueError("LineReader: the lexicon's alphabet has %d classes, the CRNN emits %d" % (lexicon.n_classes, emits))
        if decode == "words":
            _check_lanes("LineReader", lexicon)
    else:
        _check_beam("LineReader", beam, nbest, beam_limits()["beam"])
        if lexicon is not None:
            raise ValueError("LineReader: lexicon= goes with decode='lexicon' or decode='words'; got decode = %r" % (decode,))
    table = None
    if lm is None:
        if lm_weight is not None or lm_bonus is not None:
            raise ValueError("LineReader: lm_weight= and lm_bonus= go with lm=, a CharLM")
    else:
        if decode != "beam":
            raise ValueError("LineReader: lm= goes with decode='beam'; got decode = %r" % (decode,))
        if not isinstance(lm, CharLM):
            raise ValueError("LineReader: lm is a CharLM; got %r" % (type(lm).__name__,))
        if emits is not None and lm.n_classes != emits:
            raise ValueError("LineReader: the language model has %d classes, the CRNN emits %d" % (lm.n_classes, emits))
        try:
            weight, bonus = 0.5 if lm_weight is None else float(lm_weight), 0.0 if lm_bonus is None else float(lm_bonus)
            table = lm.increments(weight, bonus)
        except (TypeError, ValueError):
            raise ValueError("LineReader: lm_weight and lm_bonus are finite floats; got %r, %r" % (lm_weight, lm_bonus)) from None
        lm_weight, lm_bonus = weight, bonus
    if pattern is not None:
        if decode != "beam":
            raise ValueError("LineReader: pattern= goes with decode='beam'; got decode = %r" % (decode,))
        if lm is not None:
            raise ValueError("LineReader: pattern= and lm= do not go together")
        pattern = _as_pattern("LineReader", pattern)                 # (a pattern beyond the limits is refused where it is compiled)
        if emits is None:                                            # (the table is uploaded once, for the classes of the logits)
            raise ValueError("LineReader: pattern= needs a CRNN that states the classes it emits (rnn[-1].embedding.out_features)")
        if pattern.n_classes > emits:
            raise ValueError("LineReader: the pattern's alphabet has %d classes, the CRNN emits %d" % (pattern.n_classes, emits))
        _check_pattern("LineReader", pattern, pattern.n_classes)
    made = {"greedy": _Greedy, "lexicon": _Lexicon, "words": _Words, "lexicons": _LineLexicons,
            "beam": _BeamLM if lm is not None else _BeamPattern if pattern is not None else _Beam}[decode]
    return made(beam, nbest, lexicon, word_penalty, lm, lm_weight, lm_bonus, table, pattern)


def _locations(host, cap_len: int, plan, alphabet, strings):
    """host: the align records of a call on the host, strings: the classes that were aligned, per line -> one LineLocation per line"""
    return [_location(al, classes if al.flag != 1 else [], alphabet, rw, sq, int(W)) for al, classes, rw, sq, W in zip(
        parse_align_records(host, cap_len), strings, plan.rws, plan.squeezed, plan.desc[:, 2])]


class PendingReading:
    """What `LineReader.read` started.  `result()` is the only host wait: -> one Reading (decode="beam": one BeamReading, with lm=: one
    BeamLMReading (text, logp: the acoustic mass, lm: the LM term, score = logp + lm, alternatives [(text, logp, lm)]),
    decode="lexicon": one LexiconReading) per line, in input order.  With keep_logits: `logits` [(line indices of the chunk, its
    (T, n, C) logits on the device)]; with keep_scores (lexicon): `scores` [(line indices, the chunk's (n, K) float64 scores)].
    decode="words": one WordsReading per line (`texts()`: the words joined by spaces); with keep_lp: `lp` [(line indices, the chunk's
    (n, T, C) float64 log-soft-max on the device)].
    decode="lexicons": one LexiconReading per line, its words those of the line's OWN list and the posterior taken among them; an
    empty list or a flagged line reads "" with logp = nan; with keep_scores: `scores` [(line indices, the chunk's (n, max count) float64
    scores, the lines' counts)].
    decode="beam" with pattern=: one PatternReading per line (text, logp, mass: the log-probability that the line is ANY member of the
    format, posterior = exp(logp - mass), alternatives [(text, logp, posterior)], best first).  A line without an accepting entry
    reads "" with logp = nan while its mass stays meaningful; a flagged line has mass = nan as well.
    locate=True: `locations()`, one LineLocation per line; the alignment lies behind the decode part of every record row, and `lp`
    (with keep_lp) holds the float64 log-soft-max it ran on."""

    def __init__(self, host, event, cap, plan, mode, state, logits=None, align=None):
        self._host, self._event, self._cap, self._plan, self._mode, self._state = host, event, cap, plan, mode, state
        self.logits, self.scores, self.lp = logits, state.scores, state.lp
        self._align = align                                          # (rec_at, cap_len) of the align part of a row: locate=True
        self._out, self._located = None, None

    def result(self):
        if self._out is None:
            if self._host is None:
                self._out = []
            else:
                self._event.synchronize()
                self._out = self._mode.readings(self._host, self._cap, self._plan, self._state)
        return self._out

    def texts(self):
        return [r.text for r in self.result()]

    def locations(self):
        """locate=True: one LineLocation per line, in input order: the reading's own best string (`text`), the log-probability of its
        most probable alignment (`logp`) and one CharSpan(char, cls, first, last, x0, x1, logp) per character: its steps, its columns
        in the line the caller gets back by the convention of `word_span_pixels`, and the sum of its log-probabilities over its steps.
        flag 1 (a flagged line, or a beam without an entry): "" with logp = nan; flag 2 (a string beyond align_limits()): the text
        without characters.  A string no alignment spells has logp = -inf and no characters."""
        if self._align is None:
            raise ValueError("PendingReading.locations: the reader was made without locate=True")
        if self._host is None:
            return []
        if self._located is not None:
            return self._located
        self._event.synchronize()
        (rec_at, cap_len), (len_at, cls_at, gate_at) = self._align, self._mode.align_source(self._cap)
        strings = [row[cls_at:cls_at + row[len_at]] if (gate_at < 0 or row[gate_at] >= 1) and 0 <= row[len_at] <= self._cap else []
                   for row in self._host.tolist()]
        self._located = _locations(self._host[:, rec_at:rec_at + align_record_words(cap_len)], cap_len, self._plan, self._mode.alphabet,
                                   strings)
        return self._located


class PendingAlignment:
    """What `LineReader.align` started.  `locations()` is the only host wait: one LineLocation per line, in input order (see
    `PendingReading.locations`; `text` is the caller's own, lower-cased).  With keep_logits / keep_lp: `logits` / `lp` as
    `PendingReading` has them."""

    def __init__(self, host, event, cap_len, plan, strings, alphabet, logits=None, lp=None):
        self._host, self._event, self._cap_len, self._plan, self._strings, self._alphabet = host, event, cap_len, plan, strings, alphabet
        self.logits, self.lp, self._out = logits, lp, None

    def locations(self):
        if self._out is None:
            if self._host is None:
                self._out = []
            else:
                self._event.synchronize()
                self._out = _locations(self._host, self._cap_len, self._plan, self._alphabet, self._strings)
        return self._out


def _emitted_classes(crnn):
    """the classes a CRNN's last layer emits, None where the module does not say"""
    try:
        return int(crnn.rnn[-1].embedding.out_features)
    except (AttributeError, IndexError, TypeError):
        return None


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
    as `alternatives`.  Everything else of a call is the same; decode="greedy" is the default.
    decode="beam" with lm = a `CharLM` (lm_weight, default 0.5, lm_bonus, default 0.0: the usual shallow-fusion convention, not tuned on
    anything): the increments table `lm.increments(lm_weight, lm_bonus)` is built and uploaded once, here, and every chunk gets ONE
    tatt_ctc_beam_lm_read launch in place of the beam launch (specification `ctc_beam_lm_read_host`); `result()` gives
    `BeamLMReading`s.  A flagged line reads "" with logp = lm = score = nan.  Without lm= nothing of a call changes.
    decode="beam" with pattern = a `Pattern` or a regular expression (see `Pattern` for the syntax): every line is read against that
    FORMAT.  Every chunk gets ONE tatt_ctc_beam_pattern_read launch (the beam search with the format's DFA acting at every step,
    specification `ctc_beam_pattern_read_host`) and ONE tatt_ctc_pattern_mass launch (the exact log-probability that the line is any
    member of the format, specification `ctc_pattern_mass_host`) in place of the greedy launch; the mass lies behind the beam row of
    the call's one record buffer and travels back in its one copy.  `result()` gives `PatternReading`s.  The table is uploaded once,
    here, for the classes the CRNN emits: no `read` uploads anything for it.  ValueError here for pattern= with another decoding or with
    lm=, an alphabet with more classes than the CRNN emits, a CRNN that does not state what it emits, and a pattern beyond
    pattern_limits().  Without pattern= nothing of a call changes.
    decode="lexicon" (with lexicon = a `Lexicon` or a list of words, 1 <= nbest <= 16): every chunk gets the tatt_ctc_lexicon_score
    launches (one per non-empty segment class of the lexicon) into an (n, K) float64 buffer of its own and ONE tatt_ctc_lexicon_select
    launch in place of the greedy one (specification `ctc_lexicon_read_host`); `result()` gives `LexiconReading`s: the most probable
    word of the list, its exact CTC log-probability, its posterior among the list's words, and the `nbest` best words as
    `alternatives`.  keep_scores=True keeps every chunk's score buffer (`PendingReading.scores`).
    decode="words" (with lexicon = a `Lexicon` or a list of words, word_penalty a finite float): a line is read as a SEQUENCE of list
    words.  Every chunk gets ONE tatt_ctc_words_read launch in place of the greedy one (token passing, specification
    `ctc_words_read_host`); `result()` gives `WordsReading`s: `text` the words joined by spaces, `logp` the log-probability of the
    best alignment (plus word_penalty per word), `words` one `WordSpan(text, index, first, last, x0, x1)` per word: its steps and, by
    the convention of `word_span_pixels`, its columns in the line the caller gets back.  The lexicon must fit words_limits()["lanes"]
    packed lanes (`words_lanes`): ValueError here otherwise.  keep_lp=True keeps every chunk's float64 log-soft-max
    (`PendingReading.lp`).
    decode="lexicons" (1 <= nbest <= 16; no lexicon=): every line is read against a list of words of its OWN, given with the call:
    `read(..., lexicons=)`, a `LineLexicons` or one list per line by INPUT index (specification `ctc_line_lexicons_read_host`).  On
    top of what greedy enqueues: ONE more host-to-device copy from pinned memory (the union's codes and table and every chunk's tile
    table, pairs and counts in one int32 blob, the tables built from the plan's buckets), per chunk one (n, max count) float64 buffer,
    ONE tatt_ctc_lexicon_score_pairs launch (none for a chunk whose lists are all empty) and ONE tatt_ctc_lexicon_select_rows launch
    in place of the greedy one.  `result()` gives `LexiconReading`s: text and alternatives are words of the line's own list, the
    posterior is taken among them; an empty list or a flagged line reads "" with logp = nan.  keep_scores=True keeps (line indices,
    scores, counts) per chunk.  ValueError before anything is enqueued for a missing keyword, len(lexicons) != len(rows) and an
    alphabet with more classes than the CRNN emits.
    locate=True (decode="greedy" or "beam", plain or with lm= or pattern=; ValueError here with "lexicon", "lexicons" and "words", whose
    records hold word indices, not classes): says WHERE the characters are.  Per chunk ONE more launch right behind the decode
    launch(es), tatt_ctc_align (CTC forced alignment, specification `ctc_align_host`): it reads the reading's best string from the
    decode record ON THE DEVICE (greedy: the classes at word 0, the length at 3 cap; beam: entry 0 behind the "entries written" word,
    with the LM layout's offsets where lm= is given) and appends the alignment to the same record row at the next even word
    (`align_record_words(min(cap, 127))` words), so the call still makes its one copy back and waits for nothing.
    `PendingReading.locations()` gives one `LineLocation` per line; `result()` / `texts()` are what they are without the keyword;
    keep_lp=True keeps every chunk's float64 log-soft-max.  Without the keyword a call enqueues exactly what it enqueued before.
    `align(dev_bytes, rows, scale, texts)` aligns strings the caller knows, with no decode launch."""

    def __init__(self, crnn, batch_size: int = 48, device=None, keep_logits: bool = False, w: int = 64, decode: str = "greedy",
                 beam: int = 8, nbest: int = 4, lexicon=None, keep_scores: bool = False, word_penalty: float = 0.0,
                 keep_lp: bool = False, lm=None, lm_weight=None, lm_bonus=None, pattern=None, locate: bool = False):
        from . import functional as Fh
        from .infer import _check_module, _crnn_folds
        emits = _emitted_classes(crnn)
        mode = _reader_decoding(decode, beam, nbest, lexicon, word_penalty, lm, lm_weight, lm_bonus, pattern, locate, emits)
        self._mode, self.decode, self.locate, self.keep_scores, self.keep_lp = mode, decode, bool(locate), bool(keep_scores), bool(keep_lp)
        self.beam, self.nbest, self.lexicon, self.word_penalty, self.pattern = beam, nbest, mode.lexicon, mode.word_penalty, mode.pattern
        self.lm, self.lm_weight, self.lm_bonus = lm, mode.lm_weight, mode.lm_bonus
        _check_module(crnn, "reader CRNN")
        if not (isinstance(batch_size, int) and batch_size > 0):
            raise ValueError("batch_size must be a positive int")
        self.crnn, self.B, self.keep_logits, self.w = crnn, batch_size, bool(keep_logits), int(w)
        self.device = next(crnn.parameters()).device
        want = self.device if device is None else torch.device(device)
        if want.type != "cuda" or (want.index is not None and want.index != self.device.index):
            raise ValueError("LineReader: the CRNN lives on %s, not on %s" % (self.device, want))
        self._limits = read_limits()
        mode.upload(self.device, emits)                              # (the packed words, the pattern's or the LM's table: once, here)
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

    def check_lexicons(self, lexicons, n: int, who: str = "LineReader.read"):
        """the `lexicons=` of a call over n lines -> a `LineLexicons` (None for every decoding but "lexicons"); ValueError for the keyword
        on another decoding, a missing one, a wrong number of lists, an alphabet with more classes than the CRNN emits.  Touches no device."""
        if self.decode != "lexicons":
            if lexicons is not None:
                raise ValueError("%s: lexicons= goes with decode='lexicons'; got decode = %r" % (who, self.decode))
            return None
        if lexicons is None:
            raise ValueError("%s: decode='lexicons' needs lexicons=, one list of words per line" % who)
        lexicons = lexicons if isinstance(lexicons, LineLexicons) else LineLexicons(lexicons)
        if len(lexicons) != n:
            raise ValueError("%s: %d lists of words for %d lines" % (who, len(lexicons), n))
        emits = _emitted_classes(self.crnn)
        if emits is not None and lexicons.n_classes > emits:
            raise ValueError("%s: the lexicons' alphabet has %d classes, the CRNN emits %d" % (who, lexicons.n_classes, emits))
        return lexicons

    def read(self, dev_bytes, rows, scale, keep_logits=None, lexicons=None) -> PendingReading:
        """dev_bytes: the uint8 device buffer holding the lines, rows: (byte offset, H, W, pitch) per line (what the `line_canvases` of a
        `PendingExport` of `DeviceExporter.lines` / `.scene` / `.scene_quads` gives), scale: the SR factor -> PendingReading.
        lexicons (decode="lexicons" only, and required there): a `LineLexicons` or one list of words per line, by INPUT index."""
        rows, mode = list(rows), self._mode
        keep = self.keep_logits if keep_logits is None else bool(keep_logits)
        lexicons = self.check_lexicons(lexicons, len(rows))
        if not rows:
            return PendingReading(None, None, 0, None, mode, _ReadState(), [] if keep else None, (0, 0) if self.locate else None)
        plan = self._lines_plan("LineReader.read", dev_bytes, rows, scale)
        cap = max(rw for rw, _ in plan.buckets) // 4 + 1
        words, align = mode.record_words(cap), None
        if self.locate:
            # the alignment part lies behind the decode part of the same row, at the next even word; the row stride is even
            rec_at, cap_len, source = words + (words & 1), min(cap, ALIGN_LENGTH), mode.align_source(cap)
            words, align = rec_at + align_record_words(cap_len), (rec_at, cap_len)

        def each(state, logits, index, record, lines):
            mode.launch(logits, index, record, cap, lines, state)
            if align is not None:                                    # ONE more launch: the best string is aligned where the decode left it
                ctc_align(logits, index, record, *source, record, rec_at, cap_len, _lp_buffer(state.lp, lines, logits))
        host, ev, kept, state = self._enqueue(dev_bytes, plan, None, words, keep,
                                              lambda tail: mode.begin(self, plan, self._chunk, lexicons), each)
        return PendingReading(host, ev, cap, plan, mode, state, kept, align)

    def align(self, dev_bytes, rows, scale, texts, keep_logits=None) -> "PendingAlignment":
        """Aligns KNOWN strings, one per line (a ground-truth label, a corrected reading): dev_bytes, rows, scale as `read` takes them,
        texts: one string per line (lower-cased here) -> PendingAlignment.  Enqueues what `read` enqueues without any decode launch:
        the descriptor copy (the packed strings travel in it), the luma launch, per chunk the forward and ONE tatt_ctc_align launch,
        the copy back.  ValueError, naming the line, for a character outside the alphabet or a text beyond align_limits()["length"],
        before anything is enqueued."""
        rows, texts = list(rows), [str(t).lower() for t in texts]
        keep = self.keep_logits if keep_logits is None else bool(keep_logits)
        if len(texts) != len(rows):
            raise ValueError("LineReader.align: %d texts for %d lines" % (len(texts), len(rows)))
        alphabet = _alphabet()
        a2d = {ch: i for i, ch in enumerate(alphabet) if i >= 1}
        strings = []
        for i, t in enumerate(texts):
            if len(t) > ALIGN_LENGTH:
                raise ValueError("LineReader.align: line %d: %d characters; at most %d are aligned" % (i, len(t), ALIGN_LENGTH))
            for ch in t:
                if ch not in a2d:
                    raise ValueError("LineReader.align: line %d: the text %r has the character %r, which the alphabet %r lacks"
                                     % (i, t, ch, alphabet[1:]))
            strings.append([a2d[ch] for ch in t])
        kept_lp = [] if self.keep_lp else None
        if not rows:
            return PendingAlignment(None, None, 0, None, [], alphabet, [] if keep else None, kept_lp)
        plan = self._lines_plan("LineReader.align", dev_bytes, rows, scale)
        cap_len = max(len(s) for s in strings)

        def each(src, logits, index, record, lines):
            ctc_align(logits, index, src, 0, 2, -1, record, 0, cap_len, _lp_buffer(kept_lp, lines, logits))
        host, ev, kept, _ = self._enqueue(dev_bytes, plan, pack_strings(strings, cap_len), align_record_words(cap_len), keep,
                                          lambda tail: tail.view(len(rows), 2 + cap_len), each)
        return PendingAlignment(host, ev, cap_len, plan, strings, alphabet, kept, kept_lp)

    # -- the one chunk loop ----------------------------------------------------------------------------------------------------------
    _chunk = property(lambda self: min(self.B, READ_CHUNK))          # most lines of one forward

    def _lines_plan(self, who, dev_bytes, rows, scale):
        if not (isinstance(dev_bytes, torch.Tensor) and dev_bytes.dtype == torch.uint8 and dev_bytes.device == self.device and
                dev_bytes.is_contiguous()):
            raise ValueError("%s takes a contiguous uint8 tensor on %s" % (who, self.device))
        return read_plan(rows, scale, self.w)

    def _enqueue(self, dev_bytes, plan, extra, words, keep, begin, each):
        """What `read` and `align` enqueue on the current stream: the pinned head (the descriptor rows, every line's record row in bucket
        order, then `extra`: int32 words of the caller's, or None) and its one copy, the luma launch, `begin(extra on the device)` ->
        the call's state, per bucket chunk the forward and `each(state, logits, the record rows of the chunk, the (n, words) record,
        the line indices of the chunk)`, then the record's one copy to pinned memory and an event.  Nothing waits for the device.
        -> (the host record, the event, [(line indices, logits)] per chunk or None, the state)"""
        n = int(plan.desc.shape[0])
        order = [i for _, idx in plan.buckets for i in idx]          # bucket order -> input index: the launches' row indices
        chunk, kept, at = self._chunk, [] if keep else None, n * READ_DESC + n
        with torch.cuda.device(self.device):
            self._check_weights()
            head = torch.empty(at + (0 if extra is None else extra.size), dtype=torch.int32, pin_memory=True)
            hn = head.numpy()
            hn[:n * READ_DESC] = plan.desc.reshape(-1)
            hn[n * READ_DESC:at] = order
            if extra is not None:
                hn[at:] = extra.reshape(-1)
            head_dev = torch.empty(head.numel(), dtype=torch.int32, device=self.device)
            head_dev.copy_(head, non_blocking=True)
            luma = torch.empty(plan.floats, dtype=torch.float32, device=self.device)
            line_luma(dev_bytes, head_dev, plan.desc, luma)
            state = begin(head_dev[at:])
            record = torch.empty(n, words, dtype=torch.int32, device=self.device)
            index, pos, foff = head_dev[n * READ_DESC:at], 0, 0
            for rw, idx in plan.buckets:
                x = luma[foff:foff + len(idx) * READ_HEIGHT * rw].view(len(idx), 1, READ_HEIGHT, rw)
                foff += len(idx) * READ_HEIGHT * rw
                for i in range(0, len(idx), chunk):
                    m = min(chunk, len(idx) - i)
                    logits = self.forward(x[i:i + m])
                    each(state, logits, index[pos:pos + m], record, idx[i:i + m])
                    if keep:
                        kept.append((idx[i:i + m], logits))
                    pos += m
            host = torch.empty(n, words, dtype=torch.int32, pin_memory=True)
            host.copy_(record, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        return host, ev, kept, state
