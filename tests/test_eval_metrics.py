"""Full eval metrics (bicubic LR baseline, normalised edit distances, per-image records): the parts that need no GPU -- the string
edit distance that specifies the score kernel, the 64-wide label encoder, the kernel's numpy restatement against both, the C ABI."""
import ctypes
import random
import string

import pytest
import torch

from tests.greedy_score_ref import CAP, greedy_decode, greedy_score_ref, ned_from_hist, wave_distance

NEW_SYMBOLS = ("tatt_bicubic_resize", "tatt_ctc_greedy_score")
VOC_TYPES = ("digit", "lower", "upper", "all")


def test_new_symbols_declared_and_exported():
    from tatt_amd._lib import LIB_PATH, parse_header
    protos = parse_header()
    dll = ctypes.CDLL(LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos, name
        assert hasattr(dll, name), name
    assert [n for _, n in protos["tatt_ctc_greedy_score"]][-7:] == ["dist", "st_dec", "st_img", "hist", "scored", "skipped", "st"]
    assert [n for _, n in protos["tatt_bicubic_resize"]][-7:] == ["B", "C", "H", "W", "OH", "OW", "st"]


def test_device_entries_refuse_cpu_tensors():
    from tatt_amd.crnn import bicubic_resize
    from tatt_amd.infer import ctc_greedy_score
    with pytest.raises(RuntimeError, match="AMD GPU"):
        bicubic_resize(torch.zeros(1, 3, 4, 4), (8, 8))
    with pytest.raises(RuntimeError, match="AMD GPU"):
        ctc_greedy_score(torch.zeros(26, 2, 37), torch.ones(37, dtype=torch.int32), torch.zeros(2, 64, dtype=torch.int32),
                         torch.zeros(2, dtype=torch.int32))


# ---- io.edit_distance ----------------------------------------------------------------------------------------------------------------
def _brute(a, b):
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        for j in range(len(b) + 1):
            if i == 0 or j == 0:
                D[i][j] = i + j
            else:
                D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D[len(a)][len(b)]


def test_edit_distance():
    from tatt_amd.io import edit_distance
    assert edit_distance("kitten", "sitting") == 3
    assert edit_distance("", "") == 0 and edit_distance("", "abc") == 3 and edit_distance("abcd", "") == 4
    assert edit_distance("abc", "abc") == 0 and edit_distance("abc", "ABC") == 3
    rnd = random.Random(3)
    for _ in range(3000):
        a = "".join(rnd.choice("abc") for _ in range(rnd.randint(0, 9)))
        b = "".join(rnd.choice("abc") for _ in range(rnd.randint(0, 9)))
        d = edit_distance(a, b)
        assert d == _brute(a, b), (a, b)
        assert d == edit_distance(b, a)


# ---- the 64-wide label encoder -------------------------------------------------------------------------------------------------------
def _random_labels(n, seed):                                               # (the pool of tests/test_infer.py)
    rnd = random.Random(seed)
    pool = string.digits + string.ascii_letters + string.punctuation + " "
    out = ["", "-", "ABC", "abc", "a.b", "x" * 26, "y" * 27, "Hello", "0123"]
    while len(out) < n:
        out.append("".join(rnd.choice(pool) for _ in range(rnd.randint(0, 12))))
    return out


@pytest.mark.parametrize("voc", VOC_TYPES)
def test_encode_labels_full_matches_str_filt(voc):
    from tatt_amd.infer import D2A, LABEL_FOREIGN, encode_labels_full
    from tatt_amd.io import ALPHABET, str_filt
    assert LABEL_FOREIGN >= 64
    # 64 and 65 KEPT characters under every vocabulary (digits), with dropped ones in between, and mixed-case / punctuation ones
    labels = _random_labels(300, 11) + ["7" * 64, "7" * 65, " 1" * 64, " 1" * 65, "aB!" * 21 + "c", "aB!" * 21 + "cd", "Z" * 65, "?" * 64]
    codes, lens = encode_labels_full(labels, voc)
    assert len(codes) == len(lens) == len(labels)
    seen_foreign = seen_cap = False
    for lab, c, n in zip(labels, codes, lens):
        want = str_filt(lab, voc)
        assert len(c) == 64
        if len(want) > 64:
            assert n == -1 and all(i == -1 for i in c)
            seen_cap = True
            continue
        assert n == len(want)
        assert all(i == -1 for i in c[n:])
        for ch, i in zip(want, c[:n]):
            if ch in ALPHABET:
                assert 1 <= i <= 36 and D2A[i] == ch
            else:
                assert i == LABEL_FOREIGN
                seen_foreign = True
    assert seen_cap
    assert seen_foreign == (voc in ("upper", "all"))
    assert encode_labels_full([""], voc) == ([[-1] * 64], [0])
    # a narrower cap
    assert encode_labels_full(["abcd", "abc"], "lower", cap=3) == ([[-1] * 3, [11, 12, 13]], [-1, 3])


# ---- the kernel's restatement against the specification ----------------------------------------------------------------------------
def _ctc_logits(T=26, B=96, C=37, seed=0):                                 # (the generator of tests/test_infer_gpu.py)
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


def score_labels(preds, seed=0):
    """Labels around the decodings: equal, other case, with punctuation, shortened, prefixed, empty, shuffled, long, beyond the cap."""
    rnd = random.Random(seed)
    out = []
    for b, p in enumerate(preds):
        sh = list(p)
        rnd.shuffle(sh)
        out.append([p, p.upper(), p + "!", p[:-1], "x" + p, "", "".join(sh), p[::-1] + "Q?", (p + "ab") * 2, "1" * 64, "1" * 65,
                    "".join(rnd.choice(string.ascii_lowercase + string.digits) for _ in range(rnd.randint(1, 30)))][b % 12])
    return out


@pytest.mark.parametrize("voc", VOC_TYPES)
def test_greedy_score_ref_against_edit_distance(voc):
    from tatt_amd.infer import D2A, encode_labels_full, keep_mask
    from tatt_amd.io import ctc_greedy_decode, edit_distance, str_filt
    x = _ctc_logits(seed=len(voc))
    x[5, 41, 7] = float("nan")                                            # a NaN wins its step
    preds = ctc_greedy_decode(x)
    labels = score_labels(preds, seed=len(voc))
    codes, lens = encode_labels_full(labels, voc)
    keep = keep_mask(voc)
    r = greedy_score_ref(x.numpy(), keep, codes, lens)
    vals = []
    for b, (p, t) in enumerate(zip(preds, labels)):
        p, t = str_filt(p, voc), str_filt(t, voc)
        assert "".join(D2A[c] for c in r["dec"][b, :r["dec_len"][b]]) == p, b
        if len(t) > CAP:
            assert r["dist"][b] == -1 and r["correct"][b] == 0
            continue
        assert r["dist"][b] == edit_distance(p, t), (b, p, t)
        assert r["correct"][b] == int(p == t)
        vals.append(edit_distance(p, t) / (max(len(p), len(t)) + 1e-10))
    n_long = sum(t == "1" * 65 for t in labels)                           # the cap excludes these and nothing else
    assert r["skipped"] == n_long == 8 and r["scored"] == 96 - n_long == len(vals) and r["counter"] > 0 and r["hist"][0] == 0
    assert abs(ned_from_hist(r["hist"], r["scored"]) - sum(vals) / len(vals)) <= 1e-12
    assert sum(vals) > 0


def test_wave_distance_random_pairs():
    """The row-parallel recurrence against the textbook DP, foreign codes and every length up to the cap included."""
    from tatt_amd.io import edit_distance
    rnd = random.Random(5)
    sym = "abcd"
    for k in range(1500):
        n, m = rnd.randint(0, 26), rnd.choice([0, 1, 2, 5, 26, 27, 63, 64]) if k % 3 == 0 else rnd.randint(0, 12)
        p = [rnd.randint(1, 4) for _ in range(n)]
        lab = [rnd.choice([1, 2, 3, 4, 64]) for _ in range(m)]
        a = "".join(sym[c - 1] for c in p)
        b = "".join(sym[c - 1] if c < 64 else "#" for c in lab)
        assert wave_distance(p, lab + [-1] * (CAP - m), m) == edit_distance(a, b), (p, lab)
    assert greedy_decode(torch.zeros(3, 1, 4).numpy(), [0, 1, 1, 1]) == [[]]
