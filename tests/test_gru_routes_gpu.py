"""The GRU recurrences of csrc/gru.hip against float64 at every route and edge: both generations of the small bidirectional GRU
(gru32_*: forward, forward dispatch, three backward routes, the fragment stream through tatt_gru_wgrad_frag), saturated and extreme
gates, either side of the 32-bit addressing bound at 2^22 tokens (route level and through Fh.gru_block), the per-step kernels of the
query GRU (qgru_*) at every row-block template, and its persistent chains at every width they take.

Reference: tests/gru_ref.py in float64 (pinned on the CPU by tests/test_gru_ref.py); no reference here comes from a kernel.  The one
comparison between kernel runs that remains is the bitwise equality of the forward with and without the gate record.
Measure: max|got - ref| / max|ref| per tensor.  Bar: margin x unit + 1e-7, unit = the same measure for the float32 CPU run of the
reference against its float64 run on the same inputs (computed inside the test), margin = 4 everywhere: no route needed more, the
hardware exp and rcp of sigmoid_fast / tanh_fast included.  The weight gradients that come through split-bf16 products carry the bound
those products were tested with before (2e-5), the split-bf16 chains of the query GRU theirs (1e-4: 2^-16 per product, carried
through B steps).

Measured on the MI355X.  Per route and tensor, the case that came nearest its bar (unit and bar are that case's; n = cases); the
gradients of the two directions of the query GRU share a row:
  route                  tensor unit       bar        error        n
  fwd1                   out    1.958e-07  8.830e-07  5.533e-07   32      first generation, every grid of GRIDS and FRAG_CASES
                         gates  5.990e-08  3.396e-07  1.595e-07   32
  fwd2                   out    1.372e-07  6.489e-07  2.762e-07   32      second generation, forced at every length
                         gates  5.990e-08  3.396e-07  1.595e-07   32
  dispatch               out    2.166e-07  9.666e-07  3.047e-07    2      T = 31 and 32 as shipped
                         gates  1.855e-07  8.421e-07  2.496e-07    2
  bwd1                   dgi    3.524e-08  2.410e-07  1.520e-07   32
                         dgh    1.010e-07  5.041e-07  3.385e-07   32
                         hprev  1.958e-07  8.830e-07  5.533e-07   32
  bwd2                   dgi    3.524e-08  2.410e-07  1.520e-07   32
                         dgh    1.010e-07  5.041e-07  3.385e-07   32
                         hprev  1.919e-07  8.677e-07  3.477e-07   32
  frag                   dgi    1.695e-07  7.778e-07  2.812e-07    4
                         dWp        -      2.000e-05  5.525e-06   24      (4 geometries x 3 group counts x K = 64, 128)
                         dbp        -      2.000e-05  2.593e-06   24
                         dWhh       -      2.000e-05  4.950e-06   24
                         dbhh       -      2.000e-05  2.362e-06   24
  fwd1 / bwd1 saturated  out    7.603e-07  3.141e-06  6.930e-07    1      gates 2.264e-07 of 8.692e-07, dgi 2.562e-07 of 7.867e-07,
                                                                          dgh 3.957e-07 of 1.140e-06, hprev 6.184e-07 of 3.141e-06
  fwd1 / bwd1 extreme    out    2.854e-07  1.241e-06  3.741e-07    1      gates 2.160e-07 of 7.630e-07, dgi 2.733e-07 of 8.162e-07,
                                                                          dgh 2.345e-07 of 6.459e-07, hprev 3.186e-07 of 1.119e-06
  fwd2 / bwd2 saturated  out    4.367e-07  1.847e-06  4.919e-07    1      gates 1.394e-07 of 9.490e-07, dgi 2.121e-07 of 6.166e-07 (frag:
                                                                          the same), dgh 1.788e-07 of 6.217e-07; frag dWp 4.669e-06,
                                                                          dbp 2.736e-06, dWhh 4.902e-06, dbhh 2.578e-06 of 2e-5
  fwd2 / bwd2 extreme    out    3.310e-07  1.424e-06  3.382e-07    1      gates 1.586e-07 of 8.818e-07, dgi 2.351e-07 of 9.373e-07 (frag:
                                                                          the same), dgh 2.883e-07 of 9.275e-07; frag dWp 5.378e-06,
                                                                          dbp 1.938e-06, dWhh 4.331e-06, dbhh 2.321e-06 of 2e-5
  2^22 B=4095 H          out    2.834e-07  1.234e-06  3.099e-07    1      gates 1.638e-07 of 9.460e-07, dgi 1.946e-07 of 7.196e-07 (both
                                                                          routes), dgh 1.841e-07 of 7.610e-07; frag dWp 5.261e-06,
                                                                          dbp 1.997e-06, dWhh 4.340e-06, dbhh 1.331e-06 of 2e-5
  2^22 B=4096 H          out    3.218e-07  1.387e-06  4.044e-07    1      gates 2.473e-07 of 1.022e-06, dgi 4.760e-07 of 1.352e-06,
                                                                          dgh 5.344e-07 of 1.628e-06
  2^22 B=4095 V          out    2.971e-07  1.288e-06  2.908e-07    1      gates 1.417e-07 of 1.229e-06, dgi 2.186e-07 of 8.738e-07 (both
                                                                          routes), dgh 3.595e-07 of 9.188e-07; frag dWp 5.827e-06,
                                                                          dbp 1.387e-06, dWhh 4.101e-06, dbhh 2.004e-06 of 2e-5
  gru_block at B = 4096: the ten parameter gradients 1.3e-06 .. 5.5e-06 of their largest value (bound: rtol 2e-3, atol 2e-4 x max)
  qstep RB=1             q      8.069e-07  3.327e-06  1.781e-06    8
                         d_emb  3.260e-07  1.404e-06  4.110e-07    8
                         d_wih  2.711e-07  1.185e-06  5.414e-07   16
                         d_whh  4.079e-07  1.732e-06  1.130e-06   16
                         d_bih  1.882e-07  8.527e-07  4.052e-07   16
                         d_bhh  1.979e-07  8.918e-07  4.465e-07   16
  qstep RB=2             q      1.098e-06  4.491e-06  1.298e-06    8
                         d_emb  3.704e-07  1.582e-06  4.358e-07    8
                         d_wih  4.171e-07  1.768e-06  5.314e-07   16
                         d_whh  3.811e-07  1.625e-06  5.681e-07   12      split form (4 cases): 5.545e-06 of 2e-5
                         d_bih  2.003e-07  9.013e-07  3.573e-07   16
                         d_bhh  2.610e-07  1.144e-06  4.626e-07   12      split form: 2.665e-06 of 2e-5
  qstep RB=4             q      1.218e-06  4.973e-06  1.757e-06    8
                         d_emb  3.961e-07  1.684e-06  6.304e-07    8
                         d_wih  3.674e-07  1.570e-06  4.032e-07   16
                         d_whh  4.530e-07  1.912e-06  6.744e-07   12      split form: 4.489e-06 of 2e-5
                         d_bih  2.205e-07  9.818e-07  4.158e-07   16
                         d_bhh  2.248e-07  9.993e-07  4.407e-07   12      split form: 2.886e-06 of 2e-5
  qchain fp32            q      8.600e-07  3.540e-06  8.487e-07    7
                         d_emb  4.054e-07  1.722e-06  3.614e-07    7
                         d_wih  3.605e-07  1.542e-06  5.337e-07   14
                         d_whh  4.267e-07  1.807e-06  6.853e-07   14
                         d_bih  2.001e-07  9.005e-07  2.778e-07   14
                         d_bhh  1.699e-07  7.794e-07  2.626e-07   14
  qchain split           q      9.757e-07  1.000e-04  3.609e-06    7
                         d_emb  3.522e-07  1.000e-04  8.912e-07    7
                         d_wih  2.931e-07  1.000e-04  8.633e-07   14
                         d_whh  5.045e-07  1.000e-04  9.922e-06   14
                         d_bih  1.939e-07  1.000e-04  8.929e-07   14
                         d_bhh  2.902e-07  1.000e-04  3.512e-06   14
"""
import contextlib
import functools

import pytest
import torch

from oracle import tatt_oracle as O
from tatt_amd import ops, functional as Fh
from tests.util import check_close

import gru_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F64 = torch.float64

SPLIT_BF16_WGRAD = 2e-5             # test_gru_wgrad_frag_vs_fp64 / test_query_gru_recurrent_weight_gradient_split_bf16_vs_fp64
SPLIT_BF16_CHAIN = 1e-4             # test_query_gru_persistent_chain_matches_stepwise


@contextlib.contextmanager
def _hooks(mod, **kw):
    old = {k: getattr(mod, k) for k in kw}
    for k, v in kw.items():
        setattr(mod, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(mod, k, v)


@contextlib.contextmanager
def _recorded_calls(calls):
    real = ops.call
    ops.call = lambda name, *a: (calls.append(name), real(name, *a))[1]
    try:
        yield
    finally:
        ops.call = real


class _Judge:
    """prints unit / bar / error of every tensor it is shown and fails at the end if one was over its bar"""

    def __init__(self, route):
        self.route, self.bad = route, []

    def __call__(self, name, got, ref, unit=None, limit=None):
        err = G.rel(got, ref)
        assert torch.isfinite(got).all(), (self.route, name)
        if limit is None:
            limit = G.bar(unit)
        print("%-44s %-8s unit %s bar %.3e error %.3e%s" % (self.route, name, "%.3e" % unit if unit is not None else "    -    ", limit, err,
                                                            "" if err <= limit else "   <-- OVER"))
        if not err <= limit:
            self.bad.append((name, err, limit))

    def done(self):
        assert not self.bad, (self.route, self.bad)


def _d(t):
    return None if t is None else t.to(DEV)


# ---- the small bidirectional GRU: inputs, float64 reference and units, once per case -------------------------------------------------------
# (B, H, W) grids, each run along its rows (T = W, B*H sequences) and along its columns (T = H, B*W sequences): T in {1, 3, 4, 5, 7, 8, 9,
# 16, 17, 31, 32, 33} on either side of the prefetch depths 4 and 8 and of the forward dispatch at 32; 1, 2, 3 and 5 sequences (the
# first generation packs 4 per work-group, the second 2: padding groups and waves redo the last sequence) and more
GRIDS = [(1, 1, 1), (1, 3, 5), (1, 5, 4), (1, 4, 7), (1, 1, 8), (1, 8, 9), (3, 1, 16), (1, 16, 17), (1, 2, 31), (5, 1, 32), (1, 31, 32),
         (2, 1, 33), (1, 33, 1)]
FRAG_CASES = [(1, 8, 32, False), (3, 8, 16, True), (2, 16, 64, False), (2, 16, 64, True)]
KINDS = ("plain", "saturated", "extreme")


@functools.lru_cache(maxsize=None)
def _case(B, H, W, vertical, kind="plain"):
    gen = torch.Generator().manual_seed(7919 * B + 131 * H + 17 * W + int(vertical) + 1000003 * KINDS.index(kind))
    M = B * H * W
    gi = torch.randn(M, 192, generator=gen)
    whh = [torch.randn(96, 32, generator=gen) * 0.3 for _ in range(2)]
    bhh = [torch.randn(96, generator=gen) * 0.3 for _ in range(2)]
    dout = torch.randn(M, 64, generator=gen)
    x = torch.randn(M, 128, generator=gen)
    if kind == "saturated":                          # pre-activations reach about +-12 and beyond
        gi = gi * 4.0
    elif kind == "extreme":                          # where __expf overflows to inf or underflows to 0
        hit = torch.rand(M, 192, generator=gen) < 0.03
        val = torch.tensor([100.0, -100.0, 1e4, -1e4])[torch.randint(0, 4, (M, 192), generator=gen)]
        gi = torch.where(hit, val, gi)
    geom = G.seq_geom(B, H, W, vertical)
    assert geom == ops.seq_geom(B, H, W, vertical)
    r64 = G.bigru32(gi.double(), [w.double() for w in whh], [b.double() for b in bhh], geom, dout=dout.double())
    r32 = G.bigru32(gi, whh, bhh, geom, dout=dout)
    tok = r64["tok"].reshape(-1)
    names = ("out", "gates", "dgi", "dgh", "hprev")
    ref = {k: r64[k].reshape(tok.numel(), -1) for k in names}
    unit = {k: G.rel(r32[k], r64[k]) for k in names}
    if kind == "saturated":                          # the case is what it says: gates within 1e-5 of 0 and 1, n within 1e-6 of +-1
        g = ref["gates"].reshape(-1, 2, 4, 32)
        assert float(g[:, :, :2].min()) < 1e-5 and float(g[:, :, :2].max()) > 1 - 1e-5
        assert float(g[:, :, 2].min()) < -1 + 1e-6 and float(g[:, :, 2].max()) > 1 - 1e-6
    wg = {}
    for cat in (False, True):
        xx = x if cat else x[:, :64]
        wg[cat] = G.bigru32_weight_grads(ref["dgi"], ref["dgh"], ref["hprev"], xx.double()[tok])
    return dict(gi=gi, whh=whh, bhh=bhh, dout=dout, x=x, geom=geom, tok=tok, ref=ref, unit=unit, wg=wg)


def _forward(c, gen, save=True):
    with _hooks(ops, GRU32_V2=(gen == 2), GRU32_FWD_V2_MIN_T=0):
        return ops.gru32_fwd(_d(c["gi"]), _d(c["whh"][0]), _d(c["bhh"][0]), _d(c["whh"][1]), _d(c["bhh"][1]), c["geom"], save=save)


def _check_forward(c, gen, route):
    calls = []
    with _recorded_calls(calls):
        out, gates = _forward(c, gen)
        out_ns, none = _forward(c, gen, save=False)
    assert calls == ["tatt_gru32_fwd2" if gen == 2 else "tatt_gru32_fwd"] * 2, calls
    assert none is None and torch.equal(out, out_ns)              # the gate record changes no output bit
    j = _Judge(route)
    tok = c["tok"].to(DEV)
    j("out", out[tok], c["ref"]["out"], c["unit"]["out"])
    j("gates", gates[tok], c["ref"]["gates"], c["unit"]["gates"])
    j.done()
    return out, gates


def _check_backward(c, route_name, label, groups=(1, 3, 128)):
    """route_name: bwd1 (first generation), bwd2 (second, dgh / hprev written), frag (second, operand fragments + tatt_gru_wgrad_frag);
    each from its own generation's saved forward"""
    gen = 1 if route_name == "bwd1" else 2
    out, gates = _forward(c, gen)
    tok = c["tok"].to(DEV)
    whh = [_d(w) for w in c["whh"]]
    j = _Judge("%s %s" % (route_name, label))
    calls = []
    with _hooks(ops, GRU32_V2=(gen == 2)), _recorded_calls(calls):
        if route_name != "frag":
            dgi, dgh, hprev = ops.gru32_bwd(gates, out, _d(c["dout"]), whh[0], whh[1], c["geom"])
            assert calls == ["tatt_gru32_bwd2" if gen == 2 else "tatt_gru32_bwd"]
            for name, got in (("dgi", dgi), ("dgh", dgh), ("hprev", hprev)):
                j(name, got[tok], c["ref"][name], c["unit"][name])
        else:
            assert ops.gru_frag_ok(c["geom"])
            dgi, frag = ops.gru32_bwd_frag(gates, out, _d(c["dout"]), whh[0], whh[1], c["geom"])
            j("dgi", dgi[tok], c["ref"]["dgi"], c["unit"]["dgi"])
            for G_ in groups:
                for cat in (False, True):
                    K = 128 if cat else 64
                    dWp, dWhh = torch.empty(192, K, device=DEV), torch.empty(192, 32, device=DEV)
                    dbp, dbhh = torch.empty(192, device=DEV), torch.empty(192, device=DEV)
                    x = _d(c["x"][:, :64].contiguous())
                    xb = _d(c["x"][:, 64:].contiguous()) if cat else None
                    with _hooks(ops, GRU_WGRAD_FRAG_GROUPS=G_):
                        ops.gru_wgrad_frag(frag, x, xb, c["geom"], dWp, dWhh, dbp, dbhh)
                    for name, got, want in zip(("dWp", "dbp", "dWhh", "dbhh"), (dWp, dbp, dWhh, dbhh), c["wg"][cat]):
                        j("%s K=%d G=%d" % (name, K, G_), got, want, limit=SPLIT_BF16_WGRAD)
    j.done()


def _label(B, H, W, vertical, kind="plain"):
    return "(%d,%d,%d) %s%s" % (B, H, W, "V" if vertical else "H", "" if kind == "plain" else " " + kind)


# ---- a. forward, both generations ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gen", [1, 2])
@pytest.mark.parametrize("vertical", [False, True])
@pytest.mark.parametrize("B,H,W", GRIDS + [(2, 16, 64), (3, 8, 16), (1, 8, 32)])
def test_gru32_forward_vs_fp64(B, H, W, vertical, gen):
    """tatt_gru32_fwd / tatt_gru32_fwd2, each forced at every length: out and the gate record against float64; the output with and
    without the gate record bit for bit"""
    _check_forward(_case(B, H, W, vertical), gen, "fwd%d %s" % (gen, _label(B, H, W, vertical)))


# ---- b. forward dispatch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,entry", [(31, "tatt_gru32_fwd"), (32, "tatt_gru32_fwd2")])
def test_gru32_forward_dispatch_at_32_steps(T, entry):
    """ops.gru32_fwd as shipped: the first generation below GRU32_FWD_V2_MIN_T = 32 steps, the second from there on"""
    assert ops.GRU32_V2 and ops.GRU32_FWD_V2_MIN_T == 32
    c = _case(1, 2, T, False)
    calls = []
    with _recorded_calls(calls):
        out, gates = ops.gru32_fwd(_d(c["gi"]), _d(c["whh"][0]), _d(c["bhh"][0]), _d(c["whh"][1]), _d(c["bhh"][1]), c["geom"], save=True)
    assert calls == [entry], calls
    j = _Judge("dispatch T=%d" % T)
    j("out", out[c["tok"].to(DEV)], c["ref"]["out"], c["unit"]["out"])
    j("gates", gates[c["tok"].to(DEV)], c["ref"]["gates"], c["unit"]["gates"])
    j.done()


# ---- c. backward, three routes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["bwd1", "bwd2"])
@pytest.mark.parametrize("vertical", [False, True])
@pytest.mark.parametrize("B,H,W", GRIDS + [(2, 16, 64), (3, 8, 16), (1, 8, 32)])
def test_gru32_backward_vs_fp64(B, H, W, vertical, route):
    """tatt_gru32_bwd and tatt_gru32_bwd2 (no fragments), as shipped at lengths that are no multiple of 8 too: dgi, dgh and hprev"""
    _check_backward(_case(B, H, W, vertical), route, _label(B, H, W, vertical))


@pytest.mark.parametrize("B,H,W,vertical", FRAG_CASES)
def test_gru32_backward_fragments_vs_fp64(B, H, W, vertical):
    """tatt_gru32_bwd2 leaving operand fragments: dgi directly, the fragment stream through tatt_gru_wgrad_frag at 1, 3 and 128
    work-groups against float64 products of the REFERENCE's dgi / dgh / hprev and float64 x (with and without a concatenated half)"""
    _check_backward(_case(B, H, W, vertical), "frag", _label(B, H, W, vertical))


# ---- d. saturated and extreme gates -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["saturated", "extreme"])
@pytest.mark.parametrize("gen,B,H,W,vertical", [(1, 3, 8, 16, True), (2, 1, 8, 32, False)])
def test_gru32_saturated_and_extreme_gates(gen, B, H, W, vertical, kind):
    """gi x 4 (pre-activations to +-12 and beyond: r, z within 1e-5 of 0 or 1, n within 1e-6 of +-1), and a sprinkling of +-100 and
    +-1e4 (where __expf overflows to inf or underflows to 0): forward and every backward route of the generation, everything finite
    (`_Judge` asserts it), bars relative to the largest value of the tensor as everywhere"""
    c = _case(B, H, W, vertical, kind)
    lab = _label(B, H, W, vertical, kind)
    _check_forward(c, gen, "fwd%d %s" % (gen, lab))
    _check_backward(c, "bwd%d" % gen, lab)
    if gen == 2:
        _check_backward(c, "frag", lab, groups=(3,))


# ---- e. either side of 2^22 tokens --------------------------------------------------------------------------------------------------
def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def _sampled(nseq):
    """the first and the last sequences, ones around the middle, one elsewhere"""
    return [0, 1, nseq // 2 - 1, nseq // 2, nseq // 2 + 1, (5 * nseq) // 8 + 3, nseq - 2, nseq - 1]


@pytest.mark.parametrize("B,vertical", [(4095, False), (4096, False), (4095, True)])
def test_gru32_either_side_of_2p22_tokens(B, vertical):
    """16 x 64 grids.  B = 4095: the second generation with its largest byte offsets just under 2^32; B = 4096: tatt_gru32_fwd2 /
    tatt_gru32_bwd2 run the first generation inside the library.  Inputs are drawn on the device; 8 sequences are copied back and held
    against float64.  dout is non-zero on those sequences only, so dgi is exactly zero everywhere else (one reduction on the device)
    and the fragment route's weight gradients are sums over the sampled sequences alone."""
    H, W = 16, 64
    geom = ops.seq_geom(B, H, W, vertical)
    M = B * H * W
    fits = ops.gru2_fits(*geom)
    assert fits == (B == 4095) and ops.gru_frag_ok(geom) == fits
    gen = torch.Generator(device=DEV).manual_seed(4000 + B + int(vertical))
    cg = torch.Generator().manual_seed(77)
    whh = [torch.randn(96, 32, generator=cg) * 0.3 for _ in range(2)]
    bhh = [torch.randn(96, generator=cg) * 0.3 for _ in range(2)]
    seqs = _sampled(geom[0])
    tok2 = G.seq_tokens(geom, seqs)                                   # (8, T)
    tok = tok2.reshape(-1).to(DEV)
    douts = torch.randn(len(seqs), geom[1], 64, generator=cg)
    xs = torch.randn(len(seqs), geom[1], 128, generator=cg)
    j = _Judge("2^22 B=%d %s" % (B, "V" if vertical else "H"))
    try:
        gi = torch.randn(M, 192, device=DEV, generator=gen)
        gis = gi[tok].cpu().reshape(len(seqs), geom[1], 192)
        r64 = G.bigru32_rows(gis.double(), [w.double() for w in whh], [b.double() for b in bhh], douts.double())
        r32 = G.bigru32_rows(gis, whh, bhh, douts)
        ref = {k: v.reshape(tok.numel(), -1) for k, v in r64.items()}
        unit = {k: G.rel(r32[k], r64[k]) for k in r64}
        w = [_d(t) for t in (whh[0], bhh[0], whh[1], bhh[1])]
        with _hooks(ops, GRU32_FWD_V2_MIN_T=0):                       # (the 16-step columns too)
            out, gates = ops.gru32_fwd(gi, *w, geom, save=True)
        del gi
        j("out", out[tok], ref["out"], unit["out"])
        j("gates", gates[tok], ref["gates"], unit["gates"])
        dout = torch.zeros(M, 64, device=DEV)
        dout[tok] = _d(douts.reshape(-1, 64))
        dgi, dgh, hprev = ops.gru32_bwd(gates, out, dout, w[0], w[2], geom)
        for name, got in (("dgi", dgi), ("dgh", dgh), ("hprev", hprev)):
            j(name, got[tok], ref[name], unit[name])
        assert int(torch.count_nonzero(dgi)) == int(torch.count_nonzero(dgi[tok]))          # exactly zero off the sampled sequences
        del dgi, dgh, hprev
        _free()
        if fits:
            dgi, frag = ops.gru32_bwd_frag(gates, out, dout, w[0], w[2], geom)
            j("dgi", dgi[tok], ref["dgi"], unit["dgi"])
            assert int(torch.count_nonzero(dgi)) == int(torch.count_nonzero(dgi[tok]))
            del dgi, gates, out, dout
            x = torch.randn(M, 64, device=DEV, generator=gen)
            xb = torch.randn(M, 64, device=DEV, generator=gen)
            x[tok], xb[tok] = _d(xs[..., :64].reshape(-1, 64)), _d(xs[..., 64:].reshape(-1, 64))
            dWp, dWhh = torch.empty(192, 128, device=DEV), torch.empty(192, 32, device=DEV)
            dbp, dbhh = torch.empty(192, device=DEV), torch.empty(192, device=DEV)
            ops.gru_wgrad_frag(frag, x, xb, geom, dWp, dWhh, dbp, dbhh)
            want = G.bigru32_weight_grads(r64["dgi"], r64["dgh"], r64["hprev"], xs.double())
            for name, got, wnt in zip(("dWp", "dbp", "dWhh", "dbhh"), (dWp, dbp, dWhh, dbhh), want):
                j(name, got, wnt, limit=SPLIT_BF16_WGRAD)
    finally:
        gi = out = gates = dout = dgi = dgh = hprev = frag = x = xb = None
        _free()
    j.done()


@pytest.mark.parametrize("cat", [True, False])
def test_gru_block_trains_at_2p22_tokens(cat):
    """Fh.gru_block on GruBlock(128, 64) with xb and on GruBlock(64, 64) at B = 4096, 16 x 64, along the rows: 2^22 tokens, where the
    second-generation recurrences and with them the fragment route do not exist.  The step runs (before `ops.gru_frag_ok` knew the
    32-bit bound, the backward asked tatt_gru32_bwd2 for fragments there and got return code 3); output rows, dx / dxb rows and all ten
    parameter gradients against O.gru_block in float64 on the sampled sequences, at the bounds of test_gru_block_fused."""
    from tatt_amd.tsrn import GruBlock
    B, H, W = 4096, 16, 64
    M = B * H * W
    geom = ops.seq_geom(B, H, W, False)
    assert not ops.gru_frag_ok(geom)
    torch.manual_seed(11)
    blk = GruBlock(128 if cat else 64, 64)
    sd = {"b." + n: p.detach().double() for n, p in blk.named_parameters()}
    seqs = _sampled(geom[0])
    tok = G.seq_tokens(geom, seqs).reshape(-1).to(DEV)
    cg = torch.Generator().manual_seed(78)
    douts = torch.randn(len(seqs), W, 64, generator=cg)
    gen = torch.Generator(device=DEV).manual_seed(4100 + int(cat))
    blk = blk.to(DEV)
    calls = []
    try:
        x = torch.randn(B, H, W, 64, device=DEV, generator=gen).requires_grad_()
        xb = torch.randn(B, H, W, 64, device=DEV, generator=gen).requires_grad_() if cat else None
        dout = torch.zeros(M, 64, device=DEV)
        dout[tok] = _d(douts.reshape(-1, 64))
        with _recorded_calls(calls):
            y = Fh.gru_block(x, blk, False, xb=xb)
            y.backward(dout.reshape(B, H, W, 64))
        torch.cuda.synchronize()
        assert "tatt_gru32_bwd2" in calls and "tatt_gru_wgrad_frag" not in calls, calls
        rows = lambda t: t.detach().reshape(M, -1)[tok].cpu()
        xin = rows(x) if not cat else torch.cat([rows(x), rows(xb)], 1)
        got_y, got_dx, got_dxb = rows(y), rows(x.grad), (rows(xb.grad) if cat else None)
        assert int(torch.count_nonzero(x.grad)) == int(torch.count_nonzero(x.grad.reshape(M, -1)[tok]))
        got_pg = {n: p.grad.detach().cpu() for n, p in blk.named_parameters()}
    finally:
        x = xb = y = dout = None
        for p in blk.parameters():
            p.grad = None
        _free()
    # float64: every sampled sequence as an image of one row
    xi = xin.double().reshape(len(seqs), W, -1).permute(0, 2, 1)[:, :, None, :].clone().requires_grad_()
    ps = {k: v.clone().requires_grad_() for k, v in sd.items()}
    yr = O.gru_block(xi, ps, "b")                                   # (S, 64, 1, W)
    yr.backward(douts.double().permute(0, 2, 1)[:, :, None, :])
    want_y = yr.detach()[:, :, 0, :].permute(0, 2, 1).reshape(-1, 64)
    want_dx = xi.grad[:, :, 0, :].permute(0, 2, 1).reshape(len(seqs) * W, -1)
    check_close("gru_block.out", got_y, want_y, rtol=2e-4, atol=2e-5)
    gatol = 5e-5 * max(1.0, float(want_dx.abs().max()))
    check_close("gru_block.dx", got_dx, want_dx[:, :64], rtol=1e-3, atol=gatol)
    if cat:
        check_close("gru_block.dxb", got_dxb, want_dx[:, 64:], rtol=1e-3, atol=gatol)
    assert len(got_pg) == 10
    for n, g in got_pg.items():
        w = ps["b." + n].grad
        print("gru_block cat=%d grad %-28s error %.3e" % (cat, n, G.rel(g, w)))
        check_close("gru_block.grad." + n, g, w, rtol=2e-3, atol=2e-4 * float(w.abs().max()))


# ---- f. the query GRU's per-step kernels at every row-block template ------------------------------------------------------------------
def _qgru_params(H, C, scale, seed):
    gen = torch.Generator().manual_seed(seed)
    IN, HID = H * C, H * C // 2
    shapes = [(3 * HID, IN), (3 * HID, HID), (3 * HID,), (3 * HID,)] * 2
    return [(torch.rand(s, generator=gen) * 2 - 1) * scale for s in shapes]


@functools.lru_cache(maxsize=None)
def _qcase(B, H, W, C, scale):
    gen = torch.Generator().manual_seed(9000 + 100 * B + W)
    params = _qgru_params(H, C, scale, 5)
    emb = torch.randn(H * W, C, generator=gen)
    dq = torch.randn(B, H, W, C, generator=gen)
    r64 = G.query_gru_with_grads(emb, params, B, dq, F64)
    r32 = G.query_gru_with_grads(emb, params, B, dq, torch.float32)
    return emb, params, dq, r64, [G.rel(a, b) for a, b in zip(r32, r64)]


QNAMES = ("q", "d_emb") + tuple("d_" + n.replace("weight_", "w").replace("bias_", "b").replace("_l0", "").replace("_reverse", "_r")
                                for n in G.QGRU_NAMES)


def _qgru_run(B, H, W, C, scale, route, limit_of):
    emb, params, dq, r64, unit = _qcase(B, H, W, C, scale)
    leaves = [_d(t).requires_grad_() for t in [emb] + params]
    calls = []
    with _recorded_calls(calls):
        q = Fh.QueryGruFn.apply(*leaves, B, H, W)
        grads = torch.autograd.grad(q, leaves, _d(dq))
    torch.cuda.synchronize()
    Fh.qgru_chain_check()
    j = _Judge(route)
    for k, (name, got, ref) in enumerate(zip(QNAMES, [q.detach()] + list(grads), r64)):
        j(name, got, ref, unit[k], limit=limit_of(name))
    return j, calls


@pytest.mark.parametrize("wgrad_sb", [False, True])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("W,rb", [(8, 1), (24, 1), (256, 2), (250, 2), (512, 4), (500, 4)])
def test_query_gru_steps_at_every_row_block_template(W, rb, B, wgrad_sb):
    """tatt_qgru_fwd_step / tatt_qgru_bwd_gates / tatt_qgru_bwd_fused at H = 8, C = 64 (HID = 256, the smallest the kernels take):
    one row block per work-group (W = 8, and 24 with a ragged last block), two (16 row blocks: W = 256, 250) and four (32: W = 512, 500);
    B = 1 has no recurrent backward step.  Output and all nine gradients against float64; where the recurrent weight gradient takes
    the split-bf16 form (B W a multiple of 32), dW_hh and db_hh carry that form's bound."""
    H, C, HID = 8, 64, 256
    nrb, r = -(-W // 16), 1                                           # qgru_step_rb of csrc/gru.hip, restated: the case is what it says
    while r < 4 and nrb % (2 * r) == 0 and (nrb // (2 * r)) * (HID // 16) * 2 >= 256:
        r *= 2
    assert r == rb
    split = wgrad_sb and (B * W) % 32 == 0
    lim = lambda name: SPLIT_BF16_WGRAD if split and name in ("d_whh", "d_bhh", "d_whh_r", "d_bhh_r") else None
    with _hooks(Fh, QGRU_CHAIN_FWD=False, QGRU_CHAIN_BWD=False, QGRU_WGRAD_SB=wgrad_sb):
        j, calls = _qgru_run(B, H, W, C, 0.08, "qstep RB=%d W=%d B=%d%s" % (rb, W, B, " split" if split else ""), lim)
    assert calls.count("tatt_qgru_fwd_step") == B and calls.count("tatt_qgru_bwd_fused") == B - 1, calls
    assert ("tatt_qgru_wgrad_sb" in calls) == split and not [c for c in calls if c.endswith("_chain")], calls
    j.done()


# ---- g. the query GRU's persistent chains at every width they take --------------------------------------------------------------------
@pytest.mark.parametrize("sb", [False, True])
@pytest.mark.parametrize("W,B", [(16, 2), (16, 5), (32, 2), (32, 5), (48, 2), (48, 5), (64, 2)])
def test_query_gru_chains_at_every_width(W, B, sb):
    """tatt_qgru_fwd_chain / tatt_qgru_bwd_chain at H = 16, C = 64 (HID = 512, IN = 1024) with 1, 2, 3 and 4 row blocks (the group
    count and the placement of the work-groups differ), a backward chain of one step (B = 2) and of four, fp32 and split-bf16 products:
    output and all nine gradients against float64, once (the hand-off has its load tests elsewhere); no wait expired."""
    H, C = 16, 64
    with _hooks(Fh, QGRU_CHAIN_FWD=True, QGRU_CHAIN_BWD=True, QGRU_CHAIN_SB=sb, QGRU_WGRAD_SB=sb):
        if not (Fh._qgru_chain_takes(W, 512, False, device=DEV) and Fh._qgru_chain_takes(W, 512, True, device=DEV)):
            pytest.skip("the chains decline W = %d on this device: capacity %s" % (W, (Fh.sync_capacity(DEV),)))
        sticky = Fh.sticky_word(DEV)
        lim = (lambda name: SPLIT_BF16_CHAIN) if sb else (lambda name: None)
        j, calls = _qgru_run(B, H, W, C, 0.05, "qchain %s W=%d B=%d" % ("split" if sb else "fp32", W, B), lim)
    assert calls.count("tatt_qgru_fwd_chain") == 1 and calls.count("tatt_qgru_bwd_chain") == 1, calls
    assert not [c for c in calls if c in ("tatt_qgru_fwd_step", "tatt_qgru_bwd_fused")], calls
    assert int(sticky[0].item()) == 0
    j.done()
