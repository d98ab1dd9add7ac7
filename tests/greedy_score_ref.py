"""numpy / string restatement of tatt_ctc_greedy_score (csrc/infer.hip), step for step: the arg-max per step, the merge of repeats,
the blank and the keep mask, then the row-parallel Levenshtein recurrence the kernel runs with one lane per label position,
    tmp[j]  = min(D[i-1][j] + 1, D[i-1][j-1] + (p_i != l_j))
    D[i][j] = min(i + j, j + min_{1 <= k <= j}(tmp[k] - k)),
and the integer outputs.  tests/test_eval_metrics.py holds it to `tatt_amd.io.edit_distance` (the specification); the GPU tests
hold the kernel to it, integer for integer."""
import numpy as np

CAP = 64


def greedy_decode(logits, keep):
    """logits (T, B, C) array, keep (C,) 0/1 -> B lists of classes.  np.argmax, like torch.argmax, takes the first NaN, else the
    first maximum."""
    idx = np.argmax(np.asarray(logits, dtype=np.float32), axis=2)          # (T, B)
    out = []
    for b in range(idx.shape[1]):
        seq, last = [], 0
        for c in idx[:, b].tolist():
            if c != last:
                if c != 0 and keep[c]:
                    seq.append(c)
                last = c
        out.append(seq)
    return out


def wave_distance(p, codes, m):
    """The kernel's DP: 64 columns j = 1..64 over the padded label codes; the answer is column m of the last row."""
    lab = np.asarray(codes, dtype=np.int64)
    assert lab.shape == (CAP,) and 0 <= m <= CAP
    j = np.arange(1, CAP + 1)
    row = j.copy()                                                          # D[0][j]
    for i, pi in enumerate(p, 1):
        diag = np.concatenate([[i - 1], row[:-1]])                          # D[i-1][j-1], D[i-1][0] = i - 1
        tmp = np.minimum(row + 1, diag + (lab != pi))
        row = np.minimum(i + j, j + np.minimum.accumulate(tmp - j))
    return int(len(p) if m == 0 else row[m - 1])


def greedy_score_ref(logits, keep, codes, lens):
    """-> dict of the kernel's outputs: correct (B), counter, dec (B, T) padded with -1, dec_len (B), dist (B), hist (65), scored,
    skipped.  codes (B, 64) / lens (B) as `tatt_amd.infer.encode_labels_full` gives them."""
    T, B, _ = np.asarray(logits).shape
    dec = np.full((B, T), -1, dtype=np.int64)
    dec_len, dist, correct = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    hist = np.zeros(CAP + 1, dtype=np.int64)
    scored = skipped = 0
    for b, p in enumerate(greedy_decode(logits, keep)):
        n, m = len(p), int(lens[b])
        dec[b, :n] = p
        dec_len[b] = n
        if m < 0 or m > CAP:
            dist[b] = -1
            skipped += 1
            continue
        d = wave_distance(p, codes[b], m)
        dist[b] = d
        correct[b] = int(d == 0)
        scored += 1
        if d > 0:
            hist[max(n, m)] += d
    return dict(correct=correct, counter=int(correct.sum()), dec=dec, dec_len=dec_len, dist=dist, hist=hist, scored=scored,
                skipped=skipped)


def ned_from_hist(hist, scored):
    """How the host reads the mean normalised edit distance off the integers."""
    return sum(int(hist[M]) / (M + 1e-10) for M in range(1, CAP + 1)) / (scored + 1e-10)
