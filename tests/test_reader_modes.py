"""The decodings of `read.LineReader` as objects (`read._reader_decoding`, the pure check behind `LineReader.__init__`): the record width
of every decoding against the public `*_record_words` functions, the place of the best string (`align_source`, what locate=True hands
to tatt_ctc_align) against the row parsers, and every refusal of the reader's keywords.  Needs no GPU: the limits come from host-only
entries of the library."""
import math
import struct

import numpy as np
import pytest
import torch

ABC64 = "-0123456789abcdefghijklmnopqrstuvwxyz" + "".join(chr(0x3b1 + i) for i in range(27))     # 64 classes: more than a 37-class CRNN emits
CAPS = (1, 2, 7, 256)                                                # odd and even, the smallest and READ_MAX // 4 + 1
WORDS = ["ab", "abc", "b"]


def make(decode="greedy", beam=8, nbest=4, lexicon=None, word_penalty=0.0, lm=None, lm_weight=None, lm_bonus=None, pattern=None,
         locate=False, emits=37):
    from tatt_amd import read
    return read._reader_decoding(decode, beam, nbest, lexicon, word_penalty, lm, lm_weight, lm_bonus, pattern, locate, emits)


def uniform_lm():
    from tatt_amd import read
    return read.CharLM(np.log(np.full((37,), 1.0 / 37)))


def configurations(nbest=4):
    """name -> (the keywords, the public width function of (cap))"""
    from tatt_amd import read
    return {
        "greedy": ({}, lambda cap: 3 * cap + 2),
        "beam": ({"decode": "beam", "nbest": nbest}, lambda cap: read.beam_record_words(cap, nbest)),
        "beam+lm": ({"decode": "beam", "nbest": nbest, "lm": uniform_lm()}, lambda cap: read.beam_lm_record_words(cap, nbest)),
        "beam+pattern": ({"decode": "beam", "nbest": nbest, "pattern": "[a-z]+"}, lambda cap: read.pattern_record_words(cap, nbest)),
        "lexicon": ({"decode": "lexicon", "nbest": nbest, "lexicon": WORDS}, lambda cap: read.lexicon_record_words(nbest)),
        "words": ({"decode": "words", "nbest": nbest, "lexicon": WORDS, "word_penalty": -0.5}, read.words_record_words),
        "lexicons": ({"decode": "lexicons", "nbest": nbest}, lambda cap: read.lexicon_record_words(nbest)),
    }


@pytest.mark.parametrize("nbest", (1, 4))
def test_record_width_is_the_public_function(nbest):
    for name, (kw, width) in configurations(nbest).items():
        mode = make(**kw)
        for cap in CAPS:
            assert mode.record_words(cap) == width(cap), (name, cap, nbest)
    assert [make().record_words(cap) for cap in CAPS] == [3 * cap + 2 for cap in CAPS]


def test_the_decoding_holds_what_the_reader_shows():
    """the values `LineReader` publishes as attributes are the decoding's: converted where the reader converted them"""
    from tatt_amd import read
    modes = {name: make(**kw) for name, (kw, _) in configurations().items()}
    assert isinstance(modes["lexicon"].lexicon, read.Lexicon) and modes["lexicon"].lexicon.words == WORDS
    assert modes["words"].word_penalty == -0.5 and modes["greedy"].word_penalty == 0.0 and modes["greedy"].lexicon is None
    assert (modes["beam+lm"].lm_weight, modes["beam+lm"].lm_bonus) == (0.5, 0.0) and modes["beam"].lm_weight is None
    assert modes["beam+lm"].lm_table.shape == (37,) and modes["beam+lm"].lm_table.dtype == np.float64
    assert isinstance(modes["beam+pattern"].pattern, read.Pattern) and modes["beam+pattern"].alphabet == modes["beam+pattern"].pattern.alphabet
    assert modes["greedy"].alphabet == read._alphabet() == modes["beam+lm"].alphabet
    assert len({type(m) for m in modes.values()}) == 7


def f64_words(v):
    return list(struct.unpack("<ii", struct.pack("<d", v)))


def beam_row(cap, nbest, entries, doubles):
    """a beam record row by the layout `parse_beam_records` / `parse_beam_lm_records` document, written out here with its own
    arithmetic: [0] entries written [1] flag, then per entry the float64s, the length, a pad word, `cap` classes padded with -1,
    rounded up to an even count; the words nothing writes hold a value no field may have"""
    es = 2 * doubles + 2 + cap + cap % 2
    row = [len(entries), 0] + [-777] * (nbest * es)
    for i, (classes, values) in enumerate(entries):
        at = 2 + i * es
        for k, v in enumerate(values):
            row[at + 2 * k:at + 2 * k + 2] = f64_words(v)
        row[at + 2 * doubles] = len(classes)
        row[at + 2 * doubles + 2:at + 2 * doubles + 2 + cap] = list(classes) + [-1] * (cap - len(classes))
    return row


@pytest.mark.parametrize("cap", (7, 8))
def test_align_source_reads_what_the_parsers_read(cap):
    """row[cls_at:cls_at + row[len_at]] is the first entry the parser of the decoding returns, and row[gate_at] the entries-written word"""
    from tatt_amd import read
    best, second = [3, 36, 1, 12, 5], [9, 2]
    # greedy: `cap` classes, `cap` steps, `cap` confidences (fp32), the length, the line's confidence
    conf = lambda v: struct.unpack("<i", struct.pack("<f", v))[0]
    greedy = best + [-5] * (cap - 5) + [100 + i for i in range(cap)] + [conf(0.5 + i / 64) for i in range(cap)] + [len(best), conf(0.25)]
    mode = make()
    assert len(greedy) == mode.record_words(cap)
    len_at, cls_at, gate_at = mode.align_source(cap)
    parsed = read.parse_records(torch.tensor([greedy], dtype=torch.int32), cap)[0]
    assert greedy[cls_at:cls_at + greedy[len_at]] == parsed.classes == best and gate_at == -1 and parsed.steps == [100, 101, 102, 103, 104]
    nbest, cfg = 2, configurations(2)
    for name, doubles, parse, entries in (("beam", 1, read.parse_beam_records, [(best, (-1.5,)), (second, (-2.5,))]),
                                          ("beam+pattern", 1, read.parse_beam_records, [(best, (-1.5,)), (second, (-2.5,))]),
                                          ("beam+lm", 2, read.parse_beam_lm_records, [(best, (-1.5, -0.75)), (second, (-2.5, -0.5))])):
        mode = make(**cfg[name][0])
        row = beam_row(cap, nbest, entries, doubles)
        row += [0] * (mode.record_words(cap) - len(row))             # (the pattern's mass lies behind the beam row)
        assert len(row) == mode.record_words(cap) == cfg[name][1](cap)
        len_at, cls_at, gate_at = mode.align_source(cap)
        parsed = parse(torch.tensor([row], dtype=torch.int32), cap, nbest)[0]
        assert parsed.entries[0] == (best,) + entries[0][1] and parsed.entries[1] == (second,) + entries[1][1], name
        assert row[cls_at:cls_at + row[len_at]] == parsed.entries[0][0] == best, name
        assert gate_at == 0 and row[gate_at] == len(parsed.entries) == 2, name
    for name in ("lexicon", "words", "lexicons"):                    # records of word indices: nothing to locate
        assert make(**cfg[name][0]).align_source(cap) is None, name


def refusals():
    """(the keywords, `match=` as the tests of the decodings have it): one set per message `LineReader.__init__` raises from its arguments"""
    from tatt_amd import read
    lm = uniform_lm()
    lanes = read.words_limits()["lanes"]
    over = read.Lexicon(["%d" % i for i in range(10 ** 6, 10 ** 6 + lanes // 16)] + ["x"])
    return [
        ({"decode": "viterbi"}, "decode is 'greedy', 'beam', 'lexicon', 'words' or 'lexicons'"),
        ({"decode": "words", "lexicon": ["a"], "locate": True}, "locate"),
        ({"decode": "words", "lexicon": ["a"], "word_penalty": math.nan}, "word_penalty must be a finite float"),
        ({"decode": "beam", "word_penalty": -1.0}, "word_penalty= goes with decode='words'"),
        ({"decode": "lexicons", "nbest": 17}, "nbest <= 16"),
        ({"decode": "lexicons", "lexicon": ["a"]}, r"lexicon= goes with .* takes the lists of a call as read\(..., lexicons=\)"),
        ({"decode": "lexicon", "lexicon": ["a"], "nbest": 0}, "nbest <= 16"),
        ({"decode": "lexicon"}, "needs lexicon="),
        ({"decode": "words"}, "needs lexicon="),
        ({"decode": "words", "lexicon": ["a", "A"]}, "twice"),
        ({"decode": "lexicon", "lexicon": read.Lexicon(["a"], alphabet=ABC64)}, "the lexicon's alphabet has 64 classes, the CRNN emits 37"),
        ({"decode": "words", "lexicon": over}, "%d lanes.*at most %d" % (lanes + 64, lanes)),
        ({"decode": "beam", "beam": 4, "nbest": 5}, "nbest <= beam"),
        ({"decode": "greedy", "beam": 17}, "nbest <= beam"),
        ({"decode": "beam", "lexicon": ["a"]}, "lexicon= goes with decode='lexicon' or decode='words'; got decode = 'beam'"),
        ({"decode": "beam", "lm_bonus": 0.0}, "lm_weight= and lm_bonus= go with lm="),
        ({"decode": "lexicon", "lexicon": ["a"], "lm": lm}, "lm= goes with decode='beam'"),
        ({"decode": "beam", "lm": "trigrams"}, "lm is a CharLM; got 'str'"),
        ({"decode": "beam", "lm": lm, "emits": 38}, "the language model has 37 classes, the CRNN emits 38"),
        ({"decode": "beam", "lm": lm, "lm_weight": math.inf}, "lm_weight and lm_bonus are finite floats"),
        ({"decode": "greedy", "pattern": "a"}, "pattern= goes with decode='beam'"),
        ({"decode": "beam", "lm": lm, "pattern": "a"}, "do not go together"),
        ({"decode": "beam", "pattern": "^a"}, "at position 0"),
        ({"decode": "beam", "pattern": ".{64}"}, "states"),
        ({"decode": "beam", "pattern": 7}, "pattern"),
        ({"decode": "beam", "pattern": "a", "emits": None}, "states the classes it emits"),
        ({"decode": "beam", "pattern": read.Pattern("a", alphabet=ABC64)}, "the pattern's alphabet has 64 classes, the CRNN emits 37"),
    ]


def test_every_refusal_of_the_keywords():
    for kw, what in refusals():
        with pytest.raises(ValueError, match=what):
            make(**kw)


def test_the_first_broken_rule_wins():
    """Argument sets that break two rules at once.  The expectations were taken from the parent commit: its `LineReader.__init__` was
    run on a CPU module (torch.nn.Linear(1, 1)) with these keywords, and the message it raised is the one demanded here."""
    for kw, what in (({"decode": "lexicons", "lexicon": ["a"], "locate": True}, "locate=True goes with decode='greedy' or decode='beam'"),
                     ({"decode": "beam", "lm": uniform_lm(), "pattern": "a"}, "pattern= and lm= do not go together"),
                     ({"decode": "greedy", "lm_weight": 0.3}, "lm_weight= and lm_bonus= go with lm=, a CharLM"),
                     ({"decode": "greedy", "lm_weight": 0.3, "beam": 99}, "nbest <= beam <= 16 expected; got beam = 99")):
        with pytest.raises(ValueError, match=what) as e:
            make(**kw)
        assert str(e.value).startswith("LineReader: "), kw


def test_the_reader_refuses_through_the_same_check():
    """`LineReader.__init__` reaches these refusals before it looks at the module: the same text on a module that is no CRNN"""
    from tatt_amd import read
    module = torch.nn.Linear(1, 1)
    for kw, what in refusals():
        if kw.get("emits", 0) is not None and "emits" not in what:   # (a Linear states no classes: the refusals that need them stay above)
            kw = {k: v for k, v in kw.items() if k != "emits"}
            with pytest.raises(ValueError, match=what):
                read.LineReader(module, **kw)
