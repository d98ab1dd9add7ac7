"""Host specification of the ASTER attention decoder (reference model/recognizer/attention_recognition_head.py) in float64 numpy, written
from its definitions: forced (teacher-given y_prev), greedy (`sample`) and beam (`beam_search`, backtracking included).

Per step and row:  sProj = sEmbed(s);  e_t = wEmbed(tanh(sProj + xEmbed(x_t)));  alpha = softmax_t(e);  ctx = sum_t alpha_t x_t;
                   s' = GRU([tgt_embedding(y_prev), ctx], s);  logits = fc(s').
Tie rule (torch's topk leaves it open): candidates are ordered by score descending, then flat index ascending.

Every decoding also returns, per row, its smallest DECISION MARGIN -- how far the float64 scores were from deciding otherwise:
  greedy: the smallest top-1 - top-2 logit gap over the steps up to and including the row's first EOS;
  beam:   the smallest gap between a selected and an unselected candidate score at any step, and between the final first and second
          sequence score.  Gaps between two candidates at -inf (ended beams, which the tie rule orders) are not gaps of the arithmetic
          and are left out.
A test compares ids only on rows whose margin exceeds its bound."""
import numpy as np
import torch

BEAM = 5
DEC = "decoder.decoder."


def decoder_params(sd, prefix=DEC):
    """state_dict (of the recogniser: prefix 'decoder.decoder.', of the head alone: 'decoder.') -> float64 arrays"""
    g = lambda k: sd[prefix + k].detach().cpu().double().numpy()
    return {"Ws": g("attention_unit.sEmbed.weight"), "bs": g("attention_unit.sEmbed.bias"), "Wx": g("attention_unit.xEmbed.weight"),
            "bx": g("attention_unit.xEmbed.bias"), "wv": g("attention_unit.wEmbed.weight")[0], "wb": g("attention_unit.wEmbed.bias")[0],
            "emb": g("tgt_embedding.weight"), "Wih": g("gru.weight_ih_l0"), "Whh": g("gru.weight_hh_l0"), "bih": g("gru.bias_ih_l0"),
            "bhh": g("gru.bias_hh_l0"), "Wfc": g("fc.weight"), "bfc": g("fc.bias")}


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def step(P, x, xproj, s, y):
    """x, xproj (R, T, D); s (R, S); y (R,) ints -> logits (R, C), s' (R, S)"""
    sproj = s @ P["Ws"].T + P["bs"]
    e = np.tanh(sproj[:, None, :] + xproj) @ P["wv"] + P["wb"]
    e = np.exp(e - e.max(1, keepdims=True))
    alpha = e / e.sum(1, keepdims=True)
    ctx = np.einsum("rt,rtd->rd", alpha, x)
    gi = np.concatenate([P["emb"][y], ctx], 1) @ P["Wih"].T + P["bih"]
    gh = s @ P["Whh"].T + P["bhh"]
    H = s.shape[1]
    r = _sig(gi[:, :H] + gh[:, :H])
    z = _sig(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = np.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
    s2 = (1 - z) * n + z * s
    return s2 @ P["Wfc"].T + P["bfc"], s2


def _start(P, x):
    x = np.asarray(x, dtype=np.float64)
    return x, x @ P["Wx"].T + P["bx"], np.zeros((x.shape[0], P["Whh"].shape[1])), np.full(x.shape[0], P["Wfc"].shape[0], dtype=np.int64)


def forced(P, x, targets):
    """-> logits (B, L, C); y_prev of step i is targets[:, i - 1] (<BOS> at step 0)"""
    x, xproj, s, y = _start(P, x)
    out = []
    for i in range(targets.shape[1]):
        lg, s = step(P, x, xproj, s, y)
        out.append(lg)
        y = np.asarray(targets[:, i], dtype=np.int64)
    return np.stack(out, 1)


def greedy(P, x, L, eos):
    """-> ids (B, L), scores (B, L) (the arg-max's softmax value), margin (B,)"""
    x, xproj, s, y = _start(P, x)
    B = x.shape[0]
    ids, scores = np.zeros((B, L), dtype=np.int64), np.zeros((B, L))
    margin, live = np.full(B, np.inf), np.ones(B, dtype=bool)
    for i in range(L):
        lg, s = step(P, x, xproj, s, y)
        y = lg.argmax(1)
        top = np.sort(lg, 1)
        margin = np.where(live, np.minimum(margin, top[:, -1] - top[:, -2]), margin)
        p = np.exp(lg - lg.max(1, keepdims=True))
        ids[:, i], scores[:, i] = y, 1.0 / p.sum(1)
        live &= y != eos
    return ids, scores, margin


def _order(v):
    """indices of a 1-D score array by score descending, then index ascending"""
    return np.lexsort((np.arange(v.size), -v))


def backtrack(sym, pred, score, eos):
    """stored decisions (L, B, K) (pred: slot of the previous step within the image) -> best ids (B, L), final margin (B,)"""
    L, B, K = sym.shape
    out, margin = np.zeros((B, L), dtype=np.int64), np.full(B, np.inf)
    for b in range(B):
        order = _order(score[L - 1, b])
        s, tp, found = score[L - 1, b, order].copy(), list(order), 0
        p = np.zeros((L, K), dtype=np.int64)
        for t in range(L - 1, -1, -1):
            cs = [sym[t, b, j] for j in tp]
            tp = [pred[t, b, j] for j in tp]
            for j in range(K - 1, -1, -1):
                if sym[t, b, j] == eos:
                    rk = K - (found % K) - 1
                    found += 1
                    tp[rk], cs[rk], s[rk] = pred[t, b, j], sym[t, b, j], score[t, b, j]
            p[t] = cs
        o = _order(s)
        out[b] = p[:, o[0]]
        if np.isfinite(s[o[0]]) and np.isfinite(s[o[1]]):
            margin[b] = s[o[0]] - s[o[1]]
    return out, margin


def beam(P, x, L, eos, K=BEAM, want_history=False):
    """-> ids (B, L) of the best sequence per image, margin (B,) [, (sym, pred, score) each (L, B, K)]"""
    x, xproj, _, _ = _start(P, x)
    B, C = x.shape[0], P["Wfc"].shape[0]
    xr, xpr = np.repeat(x, K, 0), np.repeat(xproj, K, 0)
    s = np.zeros((B * K, P["Whh"].shape[1]))
    y = np.full(B * K, C, dtype=np.int64)
    seq = np.full((B, K), -np.inf)
    seq[:, 0] = 0.0
    margin = np.full(B, np.inf)
    sym, pred, score = (np.zeros((L, B, K), dtype=np.int64), np.zeros((L, B, K), dtype=np.int64), np.zeros((L, B, K)))
    for i in range(L):
        lg, s = step(P, xr, xpr, s, y)
        m = lg.max(1, keepdims=True)
        ls = (lg - m) - np.log(np.exp(lg - m).sum(1, keepdims=True))
        with np.errstate(invalid="ignore"):
            cand = (seq.reshape(B * K, 1) + ls).reshape(B, K * C)
        sel = np.zeros((B, K), dtype=np.int64)
        for b in range(B):
            o = _order(cand[b])
            sel[b] = o[:K]
            lo, hi = cand[b, o[K - 1]], cand[b, o[K]]
            if np.isfinite(lo):
                margin[b] = min(margin[b], lo - hi)
        val = np.take_along_axis(cand, sel, 1)
        sym[i], pred[i], score[i] = sel % C, sel // C, val
        y = sym[i].reshape(B * K)
        s = s[(pred[i] + np.arange(B)[:, None] * K).reshape(B * K)]
        seq = np.where(sym[i] == eos, -np.inf, val)
    ids, fm = backtrack(sym, pred, score, eos)
    margin = np.minimum(margin, fm)
    return (ids, margin, (sym, pred, score)) if want_history else (ids, margin)


def upto_eos(ids, eos):
    """per row: the ids up to and including the first EOS (all of them if there is none) -- what get_string_aster reads"""
    out = []
    for row in np.asarray(ids):
        hit = np.nonzero(row == eos)[0]
        out.append([int(v) for v in (row[:hit[0] + 1] if hit.size else row)])
    return out


def perturb(module, seed):
    """Re-draw the BatchNorm running statistics and affine terms and the STN head's last layer from a seeded generator, in sorted key
    order, and scale the head's first linear layer.  Without it the initial running statistics make folding the identity and stn_fc2.weight = 0 gives every image the same
    control points.  Works on the reference's module and on tatt_amd.ASTER alike (same keys)."""
    g = torch.Generator().manual_seed(seed)
    sd = module.state_dict()
    with torch.no_grad():
        for k in sorted(sd):
            if not k.endswith("running_mean"):
                continue
            p = k[:-len("running_mean")]
            n = sd[k].numel()
            sd[p + "running_mean"].copy_(0.1 * torch.randn(n, generator=g))
            sd[p + "running_var"].copy_(0.5 + torch.rand(n, generator=g))
            sd[p + "weight"].copy_(0.7 + 0.3 * torch.rand(n, generator=g))      # (lower: 45 layers lose the image)
            sd[p + "bias"].copy_(0.1 * torch.randn(n, generator=g))
        if "stn_head.stn_fc2.weight" in sd:
            # the head's fully connected end is initialised to ignore the image (fc1 at std 0.001, fc2 at zero): fc1 x 300 and fc2 at std
            # 0.03 move the control points by up to 0.1 and by 5e-3 from image to image
            sd["stn_head.stn_fc1.0.weight"].mul_(300.0)
            w = sd["stn_head.stn_fc2.weight"]
            w.copy_(0.03 * torch.randn(w.shape, generator=g))
    return module


def scale_fc(module, factor=30.0):
    """the recipe that gives the decoder real decision margins: at initialisation its logits lie within +-0.6 and greedy gaps go down to
    1e-4, below fp32 error; fc.weight x 30 gives gaps >= 0.03 at |logit| <= 15 and rows of every length"""
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if k.endswith("decoder.fc.weight"):
                v.mul_(factor)
    return module


def make_head(seed, C, sDim=512, attDim=512, L=100, factor=30.0):
    """tatt_amd's decoder head from a seed, with the scaling recipe: the weights every decoder test rebuilds"""
    from tatt_amd.aster import AttentionRecognitionHead
    torch.manual_seed(seed)
    head = AttentionRecognitionHead(num_classes=C, in_planes=512, sDim=sDim, attDim=attDim, max_len_labels=L)
    return scale_fc(head, factor)


# ---- the cases the decoder tests and tools/gen_golden_aster.py share -----------------------------------------------------------------
# forced mode: (B, L, C, T).  B = 17 crosses 16 rows and leaves a partial block, T = 7 leaves padding in the softmax, both class counts
# in use and both ends of L appear with every B
FORCED_CASES = [(1, 12, 39, 25), (1, 100, 97, 7), (3, 100, 39, 25), (3, 12, 97, 7), (17, 12, 97, 25), (17, 100, 39, 7)]
HEAD_SEED = 1
EOS = {39: 36, 97: 94}


def forced_inputs(i):
    B, L, C, T = FORCED_CASES[i]
    g = torch.Generator().manual_seed(100 + i)
    x = torch.randn(B, T, 512, generator=g)
    targets = torch.randint(0, C, (B, L), generator=g)
    return x, targets


def features(B, T=25, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, 512, generator=g)


def end_all_beams(head, eos, K=2000.0, theta=0.54, unit=0):
    """Parameter surgery that makes every hypothesis end at the same step.  A live beam offers one EOS candidate, so all five beams end
    only where five live beams all prefer EOS, i.e. where its probability jumps from negligible to overwhelming -- what a trained
    recogniser does at the end of a word and random weights never do.  Hidden unit `unit` is turned into a counter (z = 0.8, n = 1:
    h_t = 1 - 0.8^t whatever the input) and the EOS logit reads only it, K (h - theta): about -100 up to the third step, +100 from the
    fourth on."""
    du = head.decoder
    H = du.gru.weight_hh_l0.shape[1]
    with torch.no_grad():
        for g in range(3):
            du.gru.weight_ih_l0[g * H + unit].zero_()
            du.gru.weight_hh_l0[g * H + unit].zero_()
            du.gru.bias_ih_l0[g * H + unit] = 0.0
            du.gru.bias_hh_l0[g * H + unit] = 0.0
        du.gru.bias_ih_l0[H + unit] = float(np.log(0.8 / 0.2))
        du.gru.bias_ih_l0[2 * H + unit] = 10.0
        du.fc.weight[eos].zero_()
        du.fc.weight[eos, unit] = K
        du.fc.bias[eos] = -K * theta
    return head


def shift_eos(module, eos, shift):
    """fc.bias[eos] += shift: rows end sooner, and a beam that runs fewer steps keeps larger margins"""
    with torch.no_grad():
        for k, v in module.state_dict().items():
            if k.endswith("decoder.fc.bias"):
                v[eos] += shift
    return module


# the whole-recogniser fixture (tests/golden/aster_e2e.npz): model seed, `perturb` seed, image seed, EOS shift.  Image seed and shift are the
# first of a search (shift 0, 1, 1.5, 2 x seeds 0..39) at which all three rows keep beam and greedy margins above the bound
E2E_SEED, PERTURB_SEED, IMG_SEED, E2E_EOS_SHIFT = 7, 11, 7, 1.0
DECODE_FEATURE_SEED = 18          # features(8, seed): the first seed at which at most two of the eight rows' beam margins are below the bound


def e2e_model(cls, **kw):
    """the fixture's recogniser from its seeds: `cls` is tatt_amd.ASTER (tests) or the reference's RecognizerBuilder (the generator)"""
    torch.manual_seed(E2E_SEED)
    m = cls(**kw)
    scale_fc(perturb(m, PERTURB_SEED))
    return shift_eos(m, kw["eos"], E2E_EOS_SHIFT)


def margin_bound(ref_err, maxabs):
    """the forced-mode error bar 4 x (the reference's own fp32 error) + 1e-7 x max |logit|, and 100 x it: the margin a row needs"""
    bar = 4.0 * float(ref_err) + 1e-7 * float(maxabs)
    return bar, 100.0 * bar
