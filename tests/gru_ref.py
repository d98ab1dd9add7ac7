"""TEST INFRASTRUCTURE: dtype-generic specifications of the GRU recurrences of csrc/gru.hip -- the small bidirectional GRU of the
sequential-residual blocks (gru32_*) and the query-embedding GRU (qgru_*).  Plain torch, every step written out as a loop over time; run
in float64 they are the reference, run in float32 on the CPU they are the unit of the error bars.  Nothing here imports tatt_amd.
tests/test_gru_ref.py pins them on the CPU against torch.nn.GRU and the oracle in float64 and against float64 autograd; the GPU file
tests/test_gru_routes_gpu.py compares the HIP kernels with them.

Small BiGRU.  The kernels take the input projection gi [tok][192] = [fwd r, z, n | rev r, z, n] on a token grid that a geometry tuple
(nseq, T, s_in, stride_hi, stride_lo, stride_t) cuts into sequences: step t of sequence s is token
(s // s_in) * stride_hi + (s % s_in) * stride_lo + t * stride_t (`seq_tokens`).  Sequences are independent, so every function works on
a LIST of sequences and returns its results per (listed sequence, time step); `seq_tokens` gives the token each of them belongs to.
Layouts (the ones csrc/gru.hip documents): out [.][64] = [fwd h | rev h]; gates [.][256] = per direction r | z | n | W_hn h + b_hn (32
each); dgi [.][192] the gradient of gi; dgh [.][192] the recurrent-side gate gradients (= dgi with the n gate scaled by r); hprev [.][64]
the h_{t-1} each step consumed (0 at a direction's first step).

Error measure and bars (`rel`, `bar`): max|got - ref| / max|ref| per tensor; bar = margin x unit + 1e-7 with unit = the same measure for
the float32 CPU run against the float64 run on the same inputs.
"""
import torch


def rel(got, ref):
    """max|got - ref| / max|ref|"""
    ref = ref.detach().double().cpu()
    return float((got.detach().double().cpu() - ref).abs().max() / max(float(ref.abs().max()), 1e-300))


def bar(unit, margin=4.0):
    return margin * unit + 1e-7


# ---- the small bidirectional GRU (hidden 32) ------------------------------------------------------------------------------------------
def seq_geom(B, H, W, vertical):
    """the geometry tuple of the (B, H, W) token grid: image columns (vertical) or image rows as sequences"""
    if vertical:
        return B * W, H, W, H * W, 1, W
    return B * H, W, 1, W, 0, 1


def seq_tokens(geom, seqs=None):
    """-> (len(seqs), T) int64: the token of every step of the listed sequences (default: all of them)"""
    nseq, T, s_in, stride_hi, stride_lo, stride_t = geom
    s = torch.arange(nseq) if seqs is None else torch.as_tensor(list(seqs), dtype=torch.int64)
    assert int(s.min()) >= 0 and int(s.max()) < nseq
    base = torch.div(s, s_in, rounding_mode="floor") * stride_hi + (s % s_in) * stride_lo
    return base[:, None] + torch.arange(T)[None, :] * stride_t


def bigru32_steps(gis, whh, bhh):
    """gis (S, T, 192): gi of S sequences; whh = (W_hh forward, W_hh reverse) (96, 32); bhh = (b_hh forward, reverse) (96)
    -> out (S, T, 64), gates (S, T, 256), hprev (S, T, 64)"""
    S, T, _ = gis.shape
    out, gates, hprev = [[None] * T, [None] * T], [[None] * T, [None] * T], [[None] * T, [None] * T]
    for d in range(2):
        W, b = whh[d], bhh[d]
        h = gis.new_zeros(S, 32)
        for t in (range(T - 1, -1, -1) if d else range(T)):
            g = gis[:, t, 96 * d:96 * (d + 1)]
            gh = h @ W.t() + b
            r = torch.sigmoid(g[:, 0:32] + gh[:, 0:32])
            z = torch.sigmoid(g[:, 32:64] + gh[:, 32:64])
            n = torch.tanh(g[:, 64:96] + r * gh[:, 64:96])
            hprev[d][t] = h
            h = (1.0 - z) * n + z * h
            out[d][t] = h
            gates[d][t] = torch.cat([r, z, n, gh[:, 64:96]], 1)
    join = lambda a: torch.cat([torch.stack(a[0], 1), torch.stack(a[1], 1)], 2)
    return join(out), join(gates), join(hprev)


def bigru32(gi, whh, bhh, geom, seqs=None, dout=None):
    """gi [tok][192] (only the rows of the listed sequences are read), dout [tok][64] or None
    -> {"tok": (S, T), "out", "gates", "hprev"} and, with dout, {"dgi", "dgh"}: all (S, T, .) in gi's dtype; dgi from autograd"""
    tok = seq_tokens(geom, seqs)
    res = bigru32_rows(gi[tok], whh, bhh, None if dout is None else dout[tok])
    res["tok"] = tok
    return res


def bigru32_rows(gis, whh, bhh, douts=None):
    """`bigru32` on rows gathered already: gis (S, T, 192), douts (S, T, 64) or None"""
    gis = gis.detach().clone().requires_grad_(douts is not None)
    out, gates, hprev = bigru32_steps(gis, whh, bhh)
    res = {"out": out.detach(), "gates": gates.detach(), "hprev": hprev.detach()}
    if douts is not None:
        (dgi,) = torch.autograd.grad(out, gis, douts)
        res["dgi"] = dgi
        res["dgh"] = dgh_of(dgi, res["gates"])
    return res


def dgh_of(dgi, gates):
    """the recurrent-side gate gradients: gi and W_hh h + b_hh enter r and z as a sum (same gradient), and n as gi_n + r (W_hn h + b_hn)"""
    dgh = dgi.clone()
    for d in range(2):
        dgh[..., 96 * d + 64:96 * d + 96] = dgi[..., 96 * d + 64:96 * d + 96] * gates[..., 128 * d:128 * d + 32]
    return dgh


def bigru32_weight_grads(dgi, dgh, hprev, x):
    """(., 192), (., 192), (., 64) and the block's input x (., K) over the same rows -> what tatt_gru_wgrad_frag leaves:
    dWp (192, K) = dgi^T x, dbp (192) = sum dgi, compact dW_hh (192, 32) = [forward; reverse], db_hh (192) = sum dgh"""
    dgi, dgh, hprev, x = (t.reshape(-1, t.shape[-1]) for t in (dgi, dgh, hprev, x))
    full = dgh.t() @ hprev
    return dgi.t() @ x, dgi.sum(0), torch.cat([full[:96, :32], full[96:, 32:]], 0), dgh.sum(0)


# ---- the query-embedding GRU ----------------------------------------------------------------------------------------------------------
QGRU_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l0_reverse", "weight_hh_l0_reverse",
              "bias_ih_l0_reverse", "bias_hh_l0_reverse")


def query_gru(emb, params, B):
    """emb (H*W, C); params: the eight nn.GRU(H*C, H*C/2, bidirectional) parameters in QGRU_NAMES order; -> (B, H, W, C).
    The GRU's batch is the W image columns and its TIME axis is the sample axis, with the same input x[w] = emb[h*W + w, c] over (h, c)
    at every step: q[n, h, w, c] = [forward h_n | reverse h_n][w, h*C + c]."""
    wih0, whh0, bih0, bhh0, wih1, whh1, bih1, bhh1 = params
    HW, C = emb.shape
    IN, HID = wih0.shape[1], whh0.shape[1]
    H = IN // C
    W = HW // H
    assert H * C == IN and H * W == HW and 2 * HID == IN
    x = emb.reshape(H, W, C).permute(1, 0, 2).reshape(W, IN)
    ys = []
    for d, (wih, whh, bih, bhh) in enumerate(((wih0, whh0, bih0, bhh0), (wih1, whh1, bih1, bhh1))):
        gi = x @ wih.t() + bih
        h = x.new_zeros(W, HID)
        hs = [None] * B
        for t in (range(B - 1, -1, -1) if d else range(B)):
            gh = h @ whh.t() + bhh
            r = torch.sigmoid(gi[:, :HID] + gh[:, :HID])
            z = torch.sigmoid(gi[:, HID:2 * HID] + gh[:, HID:2 * HID])
            n = torch.tanh(gi[:, 2 * HID:] + r * gh[:, 2 * HID:])
            h = (1.0 - z) * n + z * h
            hs[t] = h
        ys.append(torch.stack(hs, 0))                                  # (B, W, HID)
    y = torch.cat(ys, 2)                                               # (B, W, H*C)
    return y.reshape(B, W, H, C).permute(0, 2, 1, 3)


def query_gru_with_grads(emb, params, B, dq, dtype):
    """-> [q, d emb, d params x 8] in `dtype`, gradients of sum(q dq) from autograd"""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in [emb] + list(params)]
    q = query_gru(leaves[0], leaves[1:], B)
    grads = torch.autograd.grad(q, leaves, dq.to(dtype))
    return [q.detach()] + list(grads)
