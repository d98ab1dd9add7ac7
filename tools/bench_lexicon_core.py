"""The five entries built on csrc/ctc_lex.h -- tatt_ctc_lexicon_score, tatt_ctc_lexicon_select (ctclex.hip), tatt_ctc_lexicon_score_pairs,
tatt_ctc_lexicon_select_rows (ctclexp.hip) and tatt_ctc_words_read with lp_out (ctcwords.hip) -- on TWO builds of the library in one
process: the tree's libtatt_hip.so and the one given by --against (the same C ABI, e.g. the parent commit's build), alternating the
two.  Both are taken as built (`python -m tatt_amd.build` first).  Reports only (one JSON line), asserts nothing but that the two
libraries write the same bytes: every score buffer, record buffer and lp_out, NaN payloads and what a launch leaves unwritten included.

    timeout -k 10 600 python tools/bench_lexicon_core.py --against OTHER/libtatt_hip.so [--repeats 9] [--warmup 2] [--window-ms 20] [--out FILE]

Shapes, the seeded defaults of the tools that measure the paths around these entries (logits randn * 3, C = 37):
  score        tools/bench_lexicon.py: (T, n, K) = (26, 48, 50), (26, 48, 1000), (256, 16, 1000), words of 3 .. 12 characters, each lexicon
               packed with min_segment 16 (segment classes 16 and 32) and with min_segment 64 (class 64): six calls, nine kernel launches
  select       tatt_ctc_lexicon_select, nbest 4, on the scores of those three lexicons
  score_pairs  tools/bench_line_lexicons.py: (T, n) = (26, 48) and (256, 16) with 50 words per line, (26, 48) with one line of 1,000
               words and the rest 50; no word shared between lines
  select_rows  tatt_ctc_lexicon_select_rows, nbest 4, on the scores of those three
  words_read   tools/bench_words.py: (T, n, K) = (26, 48, 50), (26, 48, 1000), (256, 16, 1000), words of 3 .. 7 characters, word_penalty
               0, the record rows and lp_out in ONE buffer
The calls go through ctypes with the argument lists tatt_amd/read.py builds, the same lists for both libraries.  Windows, rotation,
`<library>_us_<entry>` and `within_<entry>` are tools/bench_resamplers.py's (its `run`): see there."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from bench_resamplers import arguments, run  # noqa: E402


class Call:
    """one call of an entry: `args` without the stream; `out` starts from `init` (every byte 0xa5) when results are compared"""

    def __init__(self, name, args, out, keep=()):
        self.name, self.args, self.out, self.keep = name, args, out, keep
        out.view(torch.uint8).fill_(0xa5)
        self.init = out.clone()

    def __call__(self, lib):
        from tatt_amd import ops
        rc = getattr(lib, self.name)(*self.args, ops.stream())
        assert rc == 0, (self.name, rc)


def make_cases(dev):
    """-> {entry: [Call]}"""
    import numpy as np
    import bench_lexicon
    import bench_line_lexicons
    import bench_words
    from tatt_amd import read
    from tatt_amd.ops import P
    up = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
    logits = lambda T, n: (torch.randn(T, n, 37, generator=torch.Generator().manual_seed(T)) * 3).to(dev)
    f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=dev)
    records = lambda n: torch.empty(n, read.lexicon_record_words(4), dtype=torch.int32, device=dev)
    cases = {k: [] for k in ("score", "select", "score_pairs", "select_rows", "words_read")}

    def score(x, lex, scores):
        T, n, C = x.shape
        codes, table = lex.device(dev)
        return Call("tatt_ctc_lexicon_score", (P(x), *x.stride(), T, n, C, P(codes), lex.n_codes, P(table), len(lex), *lex.counts,
                                               P(scores), scores.stride(0)), scores, (x, codes, table))

    for T, n, K in ((26, 48, 50), (26, 48, 1000), (256, 16, 1000)):
        x, index = logits(T, n), torch.arange(n, dtype=torch.int32).to(dev)
        words = bench_lexicon.make_words(K, K)
        lex16 = read.Lexicon(words)
        cases["score"] += [score(x, lex16, f64(n, K)), score(x, read.Lexicon(words, min_segment=64), f64(n, K))]
        given = read.ctc_lexicon_score(x, lex16, f64(n, K))          # (what the selects read: written once, by the tree's library)
        rec = records(n)
        cases["select"].append(Call("tatt_ctc_lexicon_select", (P(given), given.stride(0), n, K, 4, P(index), P(rec), n, rec.stride(0)),
                                    rec, (given, index)))

        lex = read.Lexicon(bench_words.make_words(K, K))
        codes, table = lex.device(dev)
        width = read.words_record_words(T)
        buf = torch.empty(n * width * 4 + n * T * 37 * 8, dtype=torch.uint8, device=dev)
        rec, lp = buf[:n * width * 4].view(torch.int32).view(n, width), buf[n * width * 4:].view(torch.float64).view(n, T, 37)
        cases["words_read"].append(Call("tatt_ctc_words_read", (P(x), *x.stride(), T, n, 37, P(codes), lex.n_codes, P(table), K, *lex.counts,
                                                                0.0, P(index), P(rec), n, T, rec.stride(0), P(lp), lp.stride(0)), buf,
                                        (x, codes, table, index)))

    for T, n, sizes in ((26, 48, [50] * 48), (256, 16, [50] * 16), (26, 48, [1000] + [50] * 47)):
        x, index, seen = logits(T, n), torch.arange(n, dtype=torch.int32).to(dev), set()
        lex = read.LineLexicons([bench_line_lexicons.make_words(K, 1000 * T + b, seen) for b, K in enumerate(sizes)])
        tiles, pairs, counts = lex.pack(range(n))
        most = int(counts.max())
        codes, table, tiles, pairs, counts = up(lex.codes), up(lex.table), up(tiles), up(pairs), up(counts)
        args = (P(x), *x.stride(), T, n, 37, P(codes), lex.n_codes, P(table), table.shape[0], P(tiles), tiles.shape[0], P(pairs),
                pairs.shape[0], P(counts), most)
        scores = f64(n, most)
        cases["score_pairs"].append(Call("tatt_ctc_lexicon_score_pairs", args + (P(scores), scores.stride(0)), scores,
                                         (x, codes, table, tiles, pairs, counts)))
        given = read.ctc_lexicon_score_pairs(x, codes, lex.n_codes, table, tiles, pairs, counts, f64(n, most), most)
        rec = records(n)
        cases["select_rows"].append(Call("tatt_ctc_lexicon_select_rows", (P(given), given.stride(0), n, P(counts), 4, P(index), P(rec), n,
                                                                         rec.stride(0)), rec, (given, counts, index)))
    return cases


if __name__ == "__main__":
    run("lexicon_core", arguments(), make_cases)
