"""CPU: the float64 GRU references of tests/gru_ref.py are pinned here before tests/test_gru_routes_gpu.py trusts them -- against
torch.nn.GRU and the oracle in float64, against float64 autograd for the dgh / hprev formulas, a restricted sequence list against the
full run; and `ops.gru_frag_ok` on both sides of the 32-bit addressing bound of the second-generation recurrences."""
import pytest
import torch

import gru_ref as G
from oracle import tatt_oracle as O

F64 = torch.float64


def _gru(seed, scale=0.3):
    g = torch.nn.GRU(64, 32, bidirectional=True, batch_first=True).double()
    gen = torch.Generator().manual_seed(seed)
    for p in g.parameters():
        p.data = (torch.rand(p.shape, generator=gen, dtype=F64) * 2 - 1) * scale
    return g


def _grid_as_sequences(x, vertical):
    """(B, H, W, C) -> (nseq, T, C) in the sequence order of `seq_geom`, and the way back"""
    B, H, W, C = x.shape
    if vertical:
        return x.permute(0, 2, 1, 3).reshape(B * W, H, C), lambda y: y.reshape(B, W, H, -1).permute(0, 2, 1, 3)
    return x.reshape(B * H, W, C), lambda y: y.reshape(B, H, W, -1)


@pytest.mark.parametrize("vertical", [False, True])
@pytest.mark.parametrize("B,H,W", [(2, 3, 5), (1, 4, 1), (3, 1, 9)])
def test_bigru32_against_nn_gru_float64(vertical, B, H, W):
    """outputs, the gate record, and the gradients: nn.GRU has no gi, so dgi is held against everything nn.GRU's autograd makes of it
    (dx = dgi W_ih, dW_ih = dgi^T x, db_ih = sum dgi), and dgh / hprev against its recurrent gradients (dW_hh = dgh^T hprev, db_hh = sum dgh)"""
    g = _gru(7)
    gen = torch.Generator().manual_seed(B * 100 + H * 10 + W)
    x = torch.randn(B, H, W, 64, generator=gen, dtype=F64, requires_grad=True)
    dout = torch.randn(B, H, W, 64, generator=gen, dtype=F64)
    xs, back = _grid_as_sequences(x, vertical)
    want = back(g(xs)[0])
    want.backward(dout)

    wih = torch.cat([g.weight_ih_l0, g.weight_ih_l0_reverse], 0).detach()
    bih = torch.cat([g.bias_ih_l0, g.bias_ih_l0_reverse], 0).detach()
    x2 = x.detach().reshape(-1, 64)
    gi = x2 @ wih.t() + bih
    whh = (g.weight_hh_l0.detach(), g.weight_hh_l0_reverse.detach())
    bhh = (g.bias_hh_l0.detach(), g.bias_hh_l0_reverse.detach())
    geom = G.seq_geom(B, H, W, vertical)
    r = G.bigru32(gi, whh, bhh, geom, dout=dout.reshape(-1, 64))
    tok = r["tok"].reshape(-1)
    assert sorted(tok.tolist()) == list(range(B * H * W))             # every token on exactly one sequence step
    flat = lambda k: torch.zeros(B * H * W, r[k].shape[-1], dtype=F64).index_copy_(0, tok, r[k].reshape(-1, r[k].shape[-1]))
    out, gates, dgi, dgh, hprev = (flat(k) for k in ("out", "gates", "dgi", "dgh", "hprev"))
    tol = dict(rtol=0, atol=1e-12)
    torch.testing.assert_close(out, want.detach().reshape(-1, 64), **tol)
    torch.testing.assert_close(dgi @ wih, x.grad.reshape(-1, 64), **tol)
    torch.testing.assert_close(dgi.t() @ x2, torch.cat([g.weight_ih_l0.grad, g.weight_ih_l0_reverse.grad], 0), **tol)
    torch.testing.assert_close(dgi.sum(0), torch.cat([g.bias_ih_l0.grad, g.bias_ih_l0_reverse.grad], 0), **tol)
    _, _, dwhh, dbhh = G.bigru32_weight_grads(dgi, dgh, hprev, x2)
    torch.testing.assert_close(dwhh, torch.cat([g.weight_hh_l0.grad, g.weight_hh_l0_reverse.grad], 0), **tol)
    torch.testing.assert_close(dbhh, torch.cat([g.bias_hh_l0.grad, g.bias_hh_l0_reverse.grad], 0), **tol)
    # the gate record: r, z, n reproduce h; the fourth block is W_hn h_{t-1} + b_hn
    for d in range(2):
        rg, z, n, an = (gates[:, 128 * d + 32 * k:128 * d + 32 * k + 32] for k in range(4))
        hp = hprev[:, 32 * d:32 * d + 32]
        torch.testing.assert_close((1 - z) * n + z * hp, out[:, 32 * d:32 * d + 32], **tol)
        torch.testing.assert_close(hp @ whh[d][64:].t() + bhh[d][64:], an, **tol)
        torch.testing.assert_close(torch.tanh(gi[:, 96 * d + 64:96 * d + 96] + rg * an), n, **tol)
        torch.testing.assert_close(torch.sigmoid(gi[:, 96 * d:96 * d + 32] + hp @ whh[d][:32].t() + bhh[d][:32]), rg, **tol)


@pytest.mark.parametrize("vertical", [False, True])
def test_bigru32_against_the_oracle_float64(vertical):
    B, H, W = 2, 4, 6
    g = _gru(8)
    sd = {"g." + k: v.detach() for k, v in g.named_parameters()}
    x = torch.randn(B, H, W, 64, generator=torch.Generator().manual_seed(3), dtype=F64)
    xs, back = _grid_as_sequences(x, vertical)
    want = back(O.bigru(xs, sd, "g")).reshape(-1, 64)
    gi = x.reshape(-1, 64) @ torch.cat([sd["g.weight_ih_l0"], sd["g.weight_ih_l0_reverse"]], 0).t() \
        + torch.cat([sd["g.bias_ih_l0"], sd["g.bias_ih_l0_reverse"]], 0)
    r = G.bigru32(gi, (sd["g.weight_hh_l0"], sd["g.weight_hh_l0_reverse"]), (sd["g.bias_hh_l0"], sd["g.bias_hh_l0_reverse"]),
                  G.seq_geom(B, H, W, vertical))
    torch.testing.assert_close(r["out"].reshape(-1, 64), want[r["tok"].reshape(-1)], rtol=0, atol=1e-12)


def test_dgh_and_hprev_formulas_against_autograd():
    """dW_hh = dgh^T hprev (diagonal blocks) and db_hh = sum dgh, against autograd through the recurrence itself; saturating inputs"""
    gen = torch.Generator().manual_seed(21)
    S, T = 3, 9
    gis = torch.randn(S, T, 192, generator=gen, dtype=F64) * 4
    douts = torch.randn(S, T, 64, generator=gen, dtype=F64)
    whh = [(torch.randn(96, 32, generator=gen, dtype=F64) * 0.5).requires_grad_() for _ in range(2)]
    bhh = [(torch.randn(96, generator=gen, dtype=F64) * 0.5).requires_grad_() for _ in range(2)]
    out, _, _ = G.bigru32_steps(gis, whh, bhh)
    want = torch.autograd.grad(out, whh + bhh, douts)
    r = G.bigru32_rows(gis, [w.detach() for w in whh], [b.detach() for b in bhh], douts)
    _, _, dwhh, dbhh = G.bigru32_weight_grads(r["dgi"], r["dgh"], r["hprev"], gis.new_zeros(S, T, 64))
    torch.testing.assert_close(dwhh, torch.cat(want[:2], 0), rtol=0, atol=1e-12)
    torch.testing.assert_close(dbhh, torch.cat(want[2:], 0), rtol=0, atol=1e-12)
    assert float(r["hprev"][:, 0, :32].abs().max()) == 0.0 and float(r["hprev"][:, T - 1, 32:].abs().max()) == 0.0


@pytest.mark.parametrize("vertical", [False, True])
def test_a_restricted_sequence_list_gives_the_rows_of_the_full_run(vertical):
    B, H, W = 3, 4, 5
    gen = torch.Generator().manual_seed(22)
    gi = torch.randn(B * H * W, 192, generator=gen, dtype=F64)
    dout = torch.randn(B * H * W, 64, generator=gen, dtype=F64)
    whh = [torch.randn(96, 32, generator=gen, dtype=F64) * 0.3 for _ in range(2)]
    bhh = [torch.randn(96, generator=gen, dtype=F64) * 0.3 for _ in range(2)]
    geom = G.seq_geom(B, H, W, vertical)
    full = G.bigru32(gi, whh, bhh, geom, dout=dout)
    seqs = [0, geom[0] // 2, geom[0] - 1, 4]
    part = G.bigru32(gi, whh, bhh, geom, seqs=seqs, dout=dout)
    for k in ("tok", "out", "gates", "hprev", "dgi", "dgh"):
        assert torch.equal(part[k], full[k][seqs]), k


def test_seq_tokens_is_the_kernels_addressing():
    for B, H, W in ((2, 3, 5), (1, 1, 1)):
        grid = torch.arange(B * H * W).reshape(B, H, W)
        assert torch.equal(G.seq_tokens(G.seq_geom(B, H, W, False)), grid.reshape(B * H, W))
        assert torch.equal(G.seq_tokens(G.seq_geom(B, H, W, True)), grid.permute(0, 2, 1).reshape(B * W, H))


def _qgru(H, C, seed):
    g = torch.nn.GRU(C * H, C * H // 2, bidirectional=True, batch_first=True).double()
    gen = torch.Generator().manual_seed(seed)
    for p in g.parameters():
        p.data = (torch.rand(p.shape, generator=gen, dtype=F64) * 2 - 1) * 0.2
    return g


@pytest.mark.parametrize("B,H,W,C", [(1, 2, 3, 4), (3, 2, 5, 4), (4, 4, 2, 2)])
def test_query_gru_against_nn_gru_and_the_oracle_float64(B, H, W, C):
    """the sample axis is the GRU's time axis: output and the gradients of all nine leaves"""
    g = _qgru(H, C, 31)
    gen = torch.Generator().manual_seed(32)
    emb = torch.randn(H * W, C, generator=gen, dtype=F64, requires_grad=True)
    dq = torch.randn(B, H, W, C, generator=gen, dtype=F64)
    x = emb.reshape(H, W, C).permute(1, 0, 2).reshape(W, 1, H * C).expand(W, B, H * C)
    want = g(x)[0].reshape(W, B, H, C).permute(1, 2, 0, 3)
    want_grads = torch.autograd.grad(want, [emb] + [getattr(g, n) for n in G.QGRU_NAMES], dq)
    params = [getattr(g, n).detach() for n in G.QGRU_NAMES]
    got = G.query_gru_with_grads(emb, params, B, dq, F64)
    for a, b in zip(got, [want] + list(want_grads)):
        torch.testing.assert_close(a, b.detach(), rtol=0, atol=1e-12)
    sd = {"ig.transformer.gru_encoding." + n: p for n, p in zip(G.QGRU_NAMES, params)}
    sd["ig.init_factor.weight"] = emb.detach()
    o = O.query_embedding(sd, "ig", B, H, W).reshape(B, H, W, C)
    assert o.dtype == F64
    torch.testing.assert_close(got[0], o, rtol=0, atol=1e-12)


def test_the_float32_run_is_a_yardstick():
    """the same functions in float32: a small distance from the float64 run, not zero"""
    gen = torch.Generator().manual_seed(41)
    gis = torch.randn(2, 8, 192, generator=gen)
    douts = torch.randn(2, 8, 64, generator=gen)
    whh = [torch.randn(96, 32, generator=gen) * 0.3 for _ in range(2)]
    bhh = [torch.randn(96, generator=gen) * 0.3 for _ in range(2)]
    r32 = G.bigru32_rows(gis, whh, bhh, douts)
    r64 = G.bigru32_rows(gis.double(), [w.double() for w in whh], [b.double() for b in bhh], douts.double())
    for k in r64:
        assert r32[k].dtype == torch.float32 and r64[k].dtype == F64
        assert 0.0 < G.rel(r32[k], r64[k]) < 1e-5, k
    assert G.bar(1e-6) == pytest.approx(4.1e-6) and G.bar(1e-6, 16) == pytest.approx(1.61e-5)


@pytest.mark.parametrize("vertical", [False, True])
def test_gru_frag_ok_stops_at_the_32_bit_bound(vertical):
    """(4095, 16, 64) is the largest batch whose byte offsets fit 32 bits (2^22 tokens x 1 KB gate rows): the fragment route of
    tatt_gru32_bwd2 exists there and not at 4096, where the library runs the first generation (no fragments)"""
    from tatt_amd import ops
    assert ops.gru_frag_ok(ops.seq_geom(4095, 16, 64, vertical))
    assert not ops.gru_frag_ok(ops.seq_geom(4096, 16, 64, vertical))
    assert ops.gru2_fits(*ops.seq_geom(4095, 16, 64, vertical)) and not ops.gru2_fits(*ops.seq_geom(4096, 16, 64, vertical))
    assert ops.gru_frag_ok(ops.seq_geom(2, 16, 64, vertical)) and not ops.gru_frag_ok(ops.seq_geom(3, 5, 7, vertical))
    assert ops.seq_geom(3, 5, 7, vertical) == G.seq_geom(3, 5, 7, vertical)
