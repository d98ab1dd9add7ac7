"""End-to-end parity of the HIP path (through the nn.Module surface) against the committed golden vectors
(generated from the real reference by tools/gen_golden.py) and against the CPU oracle on the same inputs.

Stated tolerance (BASELINE.json north_star): SR within 1e-3 max-abs of the reference fp32 forward.  Measured
errors are ~1e-6 in eval mode; train mode with the STN on is conditioned like 1e-4 (see tests/golden/REPORT.txt).
"""
import numpy as np
import pytest
import torch

from oracle import tatt_oracle as O
from oracle.fixtures import randomize_state_dict, make_inputs, summarize
from tests.util import max_err, rel_err, compare_param_grads, compare_first_step_moments, STRUCTURAL_ZERO_GRAD

pytestmark = pytest.mark.gpu
STD = dict(scale_factor=2, width=128, height=32, STN=True, mask=True, srb_nums=5, hidden_units=32)
SR_TOL = 1e-3
# Train-mode SR without the STN against the oracle / reference vectors.  Round 2 (exact-fp32 MFMA convolutions) measured <= 1.5e-5 and
# asserted 2e-5; the split-bf16 3x3 convolutions (16 mantissa bits per operand, tatt_conv3_c64_fwd_sb) measure 2.1e-5 / 2.2e-5 on the
# same cases -- batch statistics re-normalise every convolution output, so its 1e-6-relative error is carried through ten
# BatchNorms.  The eval forwards stay at 2e-5; the stated bar of the path is 1e-3 (north_star).
SR_TRAIN_TOL = 5e-5


def build(cls, dev, randomize=True, seed=1234, **kw):
    import tatt_amd
    torch.manual_seed(seed)
    m = getattr(tatt_amd, cls)(**kw)
    if randomize:
        m.load_state_dict(randomize_state_dict(m.state_dict()))
    return m.to(dev)


def psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return 99.0 if mse == 0 else 20 * np.log10(1.0 / np.sqrt(mse))


def test_kat_default_init_eval(dev):
    """Known-answer vector of SURVEY.md 8c: seed-1234 default init, eval, B=2."""
    z = np.load("tests/golden/kat.npz")
    m = build("TSRN_TL_TRANS", dev, randomize=False, **STD).eval()
    with torch.no_grad():
        y, w = m(torch.from_numpy(z["x"]).to(dev), torch.from_numpy(z["tp"]).to(dev))
    assert abs(float(y.double().sum()) - 168.209915) < 5e-3
    assert max_err(y, torch.from_numpy(z["sr"])) < SR_TOL
    assert max_err(y, torch.from_numpy(z["sr"])) < 2e-5, max_err(y, torch.from_numpy(z["sr"]))
    assert max_err(w, torch.from_numpy(z["pr_weights"])) < 1e-5
    assert tuple(y.shape) == (2, 4, 32, 128) and tuple(w.shape) == (2, 1024, 26)


@pytest.mark.parametrize("name,cls,tatt", [("tatt_eval_b2", "TSRN_TL_TRANS", True), ("tsrn_eval_b2", "TSRN", False)])
def test_eval_forward_golden(dev, name, cls, tatt):
    z = np.load("tests/golden/%s.npz" % name)
    m = build(cls, dev, **STD).eval()
    x = torch.from_numpy(z["x"]).to(dev)
    with torch.no_grad():
        if tatt:
            y, w = m(x, torch.from_numpy(z["tp"]).to(dev))
            assert max_err(w, torch.from_numpy(z["pr_weights"])) < 1e-5
        else:
            y = m(x)
    e = max_err(y, torch.from_numpy(z["sr"]))
    assert e < 2e-5, e
    assert psnr(y.cpu(), torch.from_numpy(z["sr"])) > 90
    assert max_err(m.block["1"][:, :8], torch.from_numpy(z["block1"])) < 1e-4
    assert max_err(m.block["7"][:, :8], torch.from_numpy(z["block7"])) < 1e-4


def test_large_tile_golden(dev):
    z = np.load("tests/golden/large_tile.npz")
    m = build("TSRN_TL_TRANS", dev, scale_factor=2, width=256, height=64, STN=False, mask=True, srb_nums=5,
              hidden_units=32).eval()
    with torch.no_grad():
        y, w = m(torch.from_numpy(z["x"]).to(dev), torch.from_numpy(z["tp"]).to(dev))
    assert tuple(y.shape) == (1, 4, 64, 256)
    assert max_err(y, torch.from_numpy(z["sr"])) < 2e-5
    assert max_err(w, torch.from_numpy(z["pr_weights"])) < 1e-5


def _train_case(dev, cls, tatt, B, golden):
    from tatt_amd.train import image_loss
    z = np.load("tests/golden/%s.npz" % golden)
    m = build(cls, dev, **STD).train()
    if tatt:
        m.infoGen.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, hr = torch.from_numpy(z["x"]), torch.from_numpy(z["hr"])
    tp = torch.from_numpy(z["tp"]) if tatt else None
    out = m(x.to(dev), tp.to(dev)) if tatt else m(x.to(dev))
    sr = out[0] if tatt else out
    loss = image_loss(sr, hr.to(dev)).mean() * 100
    loss.backward()
    # ---- against the oracle on the same inputs (full tensors) ----
    o_loss, o_grads, o_sd1, _, o_out, o_total = O.train_step(sd0, x, tp, hr, tatt=tatt, stn=True)
    assert max_err(sr, o_out["sr"]) < 3e-4, max_err(sr, o_out["sr"])
    assert abs(float(loss.detach()) - float(o_loss)) < 1e-4 * abs(float(o_loss))
    # STN parameters sit behind BatchNorms over B*1*2 samples and ReLU kinks: looser (reference-vs-oracle is 5e-3 there)
    worst = compare_param_grads(m.named_parameters(), o_grads, rtol=1e-2, rtol_stn=3e-2)
    print("worst relative gradient error vs oracle: %s %.3e" % worst)
    noise = set(z["noise_keys"].tolist())
    # ---- against the reference-generated golden vector ----
    assert max_err(sr, torch.from_numpy(z["sr"])) < SR_TOL        # stated tolerance; STN conditioning, see DESIGN.md 2
    assert abs(float(loss.detach()) - float(z["loss"])) < 1e-4 * abs(float(z["loss"]))
    gsum = dict(zip(list(z["grad_keys"]), z["grad_summary"]))
    params = dict(m.named_parameters())
    for k, ref in gsum.items():
        if k in noise:
            continue
        got = summarize(params[k].grad.cpu())
        lim = 3e-2 if k.startswith("stn_head") else (5e-2 if params[k].numel() == 1 else 1e-2)   # see tests/util.py
        assert abs(got[0] - ref[0]) < lim * ref[0] + 1e-7, (k, got[0], ref[0])       # l2 norm of the gradient
    for key in z.files:
        if key.startswith("g:"):
            g = params[key[2:]].grad.cpu()
            ref = torch.from_numpy(z[key])
            lim = 3e-2 if key.startswith("g:stn_head") else (5e-2 if g.numel() == 1 else 1e-2)
            assert rel_err(g, ref) < lim, (key, rel_err(g, ref))
    # running statistics were updated like the reference's BatchNorm
    sd1 = m.state_dict()
    for k in sd1:
        if k.endswith("running_mean") or k.endswith("running_var"):
            assert max_err(sd1[k], o_sd1[k]) < 1e-4, k
        if k.endswith("num_batches_tracked"):
            assert int(sd1[k]) == int(o_sd1[k]), k
    return m


def test_tatt_train_step_grads(dev):
    m = _train_case(dev, "TSRN_TL_TRANS", True, 4, "tatt_train_b4")
    none = [k for k, p in m.named_parameters() if p.grad is None]
    assert len(none) == 14, none       # unused parameters of the reference


def test_tsrn_train_step_grads(dev):
    _train_case(dev, "TSRN", False, 3, "tsrn_train_b3")


def test_train_step_without_stn_is_tight(dev):
    """Without the (ill-conditioned) STN/TPS front end the train-mode forward/backward agrees with the oracle to fp32
    round-off: SR to 2e-5, every gradient to 2e-3 relative."""
    from tatt_amd.train import image_loss
    kw = dict(STD, STN=False)
    m = build("TSRN_TL_TRANS", dev, **kw).train()
    m.infoGen.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, tp, hr = make_inputs(3, seed=5)
    sr, mid = m(x.to(dev), tp.to(dev))
    loss = image_loss(sr, hr.to(dev)).mean() * 100
    loss.backward()
    o_loss, o_grads, _, _, o_out, _ = O.train_step(sd0, x, tp, hr, tatt=True, stn=False)
    assert max_err(sr, o_out["sr"]) < SR_TRAIN_TOL, max_err(sr, o_out["sr"])
    assert max_err(mid["trans_feat"], o_out["tp_map"]) < 2e-5
    assert max_err(mid["pr_weights"], o_out["pr_weights"]) < 1e-6
    worst = compare_param_grads(m.named_parameters(), o_grads, rtol=2e-3)
    assert worst[1] < 2e-3, worst


def test_optimizer_step_matches_oracle(dev):
    """clip 0.25 + Adam(1e-3,(0.5,0.999)) through the train harness: post-step weights vs the oracle."""
    from tatt_amd.train import Trainer
    z = np.load("tests/golden/tatt_train_b4.npz")
    m = build("TSRN_TL_TRANS", dev, **STD).train()
    m.infoGen.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, hr, tp = (torch.from_numpy(z[k]) for k in ("x", "hr", "tp"))
    tr = Trainer(m, use_graph=False)
    loss = tr.step(x.to(dev), tp.to(dev), hr.to(dev))
    _, o_grads, o_sd1, _, _, o_total = O.train_step(sd0, x, tp, hr, tatt=True, stn=True)
    assert abs(float(tr.last_grad_norm) - float(o_total)) < 2e-3 * float(o_total)
    noise = set(z["noise_keys"].tolist())
    sd1 = m.state_dict()
    for k in sd1:
        if k in noise or k.endswith("num_batches_tracked"):
            continue
        d = float((sd1[k].cpu().float() - o_sd1[k].float()).abs().mean())
        assert d < 2e-4, (k, d)
    # the clip coefficient and the betas do not reach the weights of a first step; they do reach the moments
    coef = min(1.0, 0.25 / (float(o_total) + 1e-6))
    assert coef < 0.5
    clipped = {k: (None if g is None else g * coef) for k, g in o_grads.items()}
    worst = compare_first_step_moments(tr, list(m.named_parameters()), clipped, rtol=1e-2, rtol_stn=3e-2, skip=noise)
    print("worst first-step moment vs oracle: %s %.3e" % worst)


def test_dropout_train_mode_runs_and_varies(dev):
    """Every training forward draws fresh masks on its own (no Trainer needed); the seed word makes the stream reproducible; a
    backward that runs after a later forward still regenerates the masks of ITS forward (per-forward seed snapshot)."""
    from tatt_amd import functional as Fh
    from tatt_amd.train import image_loss
    m = build("TSRN_TL_TRANS", dev, **dict(STD, STN=False)).train()
    x, tp, hr = make_inputs(2)
    x, tp, hr = x.to(dev), tp.to(dev), hr.to(dev)
    Fh.set_seed(dev, 1)
    a, _ = m(x, tp)
    c, _ = m(x, tp)                              # next call: different masks
    Fh.set_seed(dev, 1)
    b, _ = m(x, tp)                              # same seed word -> same masks as `a`
    assert torch.isfinite(a).all()
    assert max_err(a, b) < 1e-6
    assert max_err(a, c) > 1e-6
    # two forwards in flight, backwards in the opposite order == each forward followed by its own backward
    def grads(interleaved):
        Fh.set_seed(dev, 5)
        for p in m.parameters():
            p.grad = None
        y1, _ = m(x, tp)
        if not interleaved:
            (image_loss(y1, hr).mean() * 100).backward()
        y2, _ = m(x, tp)
        (image_loss(y2, hr).mean() * 100).backward()
        if interleaved:
            (image_loss(y1, hr).mean() * 100).backward()
        return m.infoGen.fc_in.weight.grad.clone(), m.block3.conv1.weight.grad.clone()
    g_seq, g_int = grads(False), grads(True)
    for u, v in zip(g_seq, g_int):
        assert rel_err(u, v) < 1e-5, rel_err(u, v)


def test_requires_gpu_and_no_text():
    import tatt_amd
    m = tatt_amd.TSRN_TL_TRANS(**STD).eval()
    with pytest.raises(RuntimeError):
        m(torch.rand(1, 4, 16, 64))


def test_ptflops_style_probe(dev):
    """interfaces/base.py:372 calls the model on a (1,4,16,64) input with NO text prior."""
    m = build("TSRN_TL_TRANS", dev, **STD).eval()
    with torch.no_grad():
        y, w = m(torch.rand(1, 4, 16, 64, device=dev))
    assert tuple(y.shape) == (1, 4, 32, 128) and torch.isfinite(y).all()


# ---- TBSRN variant (BASELINE.json configs[4]) -------------------------------------------------------
TBSRN_KW = dict(scale_factor=2, width=512, height=32, STN=True, mask=True, input_channel=4)


@pytest.mark.parametrize("arithmetic", ["split_bf16", "fp32"])
def test_tbsrn_golden_eval_and_train(dev, arithmetic):
    """LR 16x256 (H*W = 4096: the only geometry the unmodified reference executes), B=2: eval SR, train SR, loss and
    every parameter gradient against the reference-generated vectors and the oracle -- under both arithmetics: exact fp32 products
    (bound 2e-5 on the images) and the default split-bf16 products (2^-16 per product through 5 attention blocks of 7 projections
    each: bound 5e-5, measured 2.4e-5)."""
    import tatt_amd
    from tatt_amd.train import image_loss
    z = np.load("tests/golden/tbsrn_b2.npz")
    tatt_amd.set_arithmetic(arithmetic)
    try:
        tol = 2e-5 if arithmetic == "fp32" else 5e-5
        m = build("TBSRN", dev, **TBSRN_KW).eval()
        sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
        x, hr = torch.from_numpy(z["x"]), torch.from_numpy(z["hr"])
        with torch.no_grad():
            y = m(x.to(dev))
        e = max_err(y, torch.from_numpy(z["sr_eval"]))
        assert e < tol, e
        m.train()
        m.stn = False                     # see tools/gen_golden.py: the reference cannot train with its STN at this geometry
        m.dropout_on = False
        sr = m(x.to(dev))
        loss = image_loss(sr, hr.to(dev)).mean() * 100
        loss.backward()
        assert max_err(sr, torch.from_numpy(z["sr_train"])) < tol
        assert abs(float(loss.detach()) - float(z["loss"])) < 1e-4 * float(z["loss"])
        _, o_grads, o_sd1, _, o_out, _ = O.train_step(sd0, x, None, hr, stn=False, tbsrn=True)
        worst = compare_param_grads(m.named_parameters(), o_grads, rtol=5e-3)
        print("tbsrn (%s) worst relative gradient error vs oracle: %s %.3e" % ((arithmetic,) + tuple(worst)))
        assert len([k for k, p in m.named_parameters() if p.grad is None]) == len(z["none_keys"])
        params = dict(m.named_parameters())
        scale = max(float(r[0]) for r in z["grad_summary"])
        for k, ref in zip(z["grad_keys"].tolist(), z["grad_summary"]):
            got = summarize(params[k].grad.cpu())
            assert abs(got[0] - ref[0]) < 1e-2 * ref[0] + 1e-6 * scale * params[k].numel() ** 0.5, (k, got[0], ref[0])
    finally:
        tatt_amd.set_arithmetic("split_bf16")


def test_tbsrn_train_with_stn_at_16x64(dev):
    """16x64 LR with the STN on (the throughput geometry; the reference's hard-wired 4096-position table cannot run it, the
    oracle uses positionalencoding2d(64,16,64) -- the commented-out original at model/tbsrn.py:84)."""
    from tatt_amd.train import image_loss
    m = build("TBSRN", dev, scale_factor=2, width=128, height=32, STN=True, mask=True, input_channel=4).train()
    m.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, _, hr = make_inputs(3, seed=9)
    sr = m(x.to(dev))
    loss = image_loss(sr, hr.to(dev)).mean() * 100
    loss.backward()
    o_loss, o_grads, _, _, o_out, _ = O.train_step(sd0, x, None, hr, stn=True, tbsrn=True)
    # STN conditioning and then five global self-attentions that couple every pixel: measured 4.4e-4
    assert max_err(sr, o_out["sr"]) < SR_TOL
    assert abs(float(loss.detach()) - float(o_loss)) < 1e-4 * abs(float(o_loss))
    # STN-head gradients pass through the sampler's coordinate noise and five global attentions: measured 4.9e-2 relative
    compare_param_grads(m.named_parameters(), o_grads, rtol=1e-2, rtol_stn=1e-1)


def test_tbsrn_trainer_step_with_dropout(dev):
    from tatt_amd.train import Trainer
    m = build("TBSRN", dev, randomize=False, scale_factor=2, width=128, height=32, STN=True, mask=True, input_channel=4).train()
    tr = Trainer(m, use_graph=False)
    x, _, hr = make_inputs(4, seed=3)
    l0 = float(tr.step(x.to(dev), None, hr.to(dev)))
    for _ in range(5):
        l1 = float(tr.step(x.to(dev), None, hr.to(dev)))
    assert l1 == l1 and l1 < l0


def test_width_not_a_multiple_of_64(dev):
    """LR 16x48 (width=96): none of the 64-pixel-segment kernels applies -- the convolutions fall back to the implicit-GEMM kernel,
    the GRUs scan 48-step rows.  Eval and train forward/backward against the oracle, batch of 1 and of 3."""
    from tatt_amd.train import image_loss
    kw = dict(scale_factor=2, width=96, height=32, STN=False, mask=True, srb_nums=5, hidden_units=32)
    m = build("TSRN_TL_TRANS", dev, **kw)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    for B in (1, 3):
        x, tp, hr = make_inputs(B, 16, 48, seed=20 + B)
        m.eval()
        with torch.no_grad():
            y, w = m(x.to(dev), tp.to(dev))
            o = O.generator_forward(sd0, x, tp, training=False, tatt=True, stn=False)
        assert tuple(y.shape) == (B, 4, 32, 96)
        assert max_err(y, o["sr"]) < 2e-5
        assert max_err(w, o["pr_weights"]) < 1e-5
    m.train()
    m.infoGen.dropout_on = False
    for p in m.parameters():
        p.grad = None
    sr, _ = m(x.to(dev), tp.to(dev))
    (image_loss(sr, hr.to(dev)).mean() * 100).backward()
    _, o_grads, _, _, o_out, _ = O.train_step(sd0, x, tp, hr, tatt=True, stn=False)
    assert max_err(sr, o_out["sr"]) < 5e-5
    worst = compare_param_grads(m.named_parameters(), o_grads, rtol=5e-3)
    assert worst[1] < 5e-3, worst


# ---- the published number's own configuration: hipGraph replay, the second stream, B = 48 ---------------------------------------
def _flat_state(m, tr):
    sd = m.state_dict()

    def canon(buf):                  # parameters in the MODULE's order, whatever bucket layout the trainer chose
        return torch.cat([buf[o:o + k] for o, k in (tr.flat.offsets[id(p)] for p in m.parameters())])
    return {"p": canon(tr.flat_p), "m": canon(tr.flat_m), "v": canon(tr.flat_v),
            "bn": torch.cat([v.reshape(-1).float() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))]),
            "nbt": torch.stack([v.reshape(()) for k, v in sd.items() if k.endswith("num_batches_tracked")])}


def _run_steps(dev, nsteps, B, dropout, stn=True, model_seed=1234, **trainer_kw):
    from tatt_amd import functional as Fh
    from tatt_amd.train import Trainer
    m = build("TSRN_TL_TRANS", dev, seed=model_seed, **dict(STD, STN=stn)).train()
    m.infoGen.dropout_on = dropout
    Fh.set_seed(dev, 99)
    tr = Trainer(m, **trainer_kw)
    losses = []
    for i in range(nsteps):
        x, tp, hr = make_inputs(B, seed=40 + i + (0 if model_seed == 1234 else model_seed))    # (tools/gen_golden_drift.py: data_seed)
        losses.append(tr.step(x.to(dev), tp.to(dev), hr.to(dev)))
    torch.cuda.synchronize()
    return [float(l) for l in losses], _flat_state(m, tr), int(Fh.seed_tensor(dev)), float(tr.last_grad_norm)


@pytest.mark.parametrize("dropout,B,stn", [(False, 4, True), (True, 4, True), (True, 48, True), (False, 3, False)])
def test_graph_replay_equals_eager(dev, dropout, B, stn):
    """6 steps (2 eager + capture + 3 replays, fresh data every step) through Trainer(use_graph=True) next to the same 6 steps
    launched eagerly, from the same weights and dropout seed: same losses, weights, Adam moments, BatchNorm running
    statistics, num_batches_tracked and seed word.  The kernels and their order are identical, so the comparison is (near-)exact;
    with dropout ON it also proves that replays draw the masks the eager run draws."""
    # (STN off: "first" is the LAST stage, so its deferred closures run merged onto the main stream -- the layout in which a closure
    # split across two lanes raced in round 4; kept as a case of its own)
    le, se, seed_e, gn_e = _run_steps(dev, 6, B, dropout, stn=stn, use_graph=False)
    lg, sg, seed_g, gn_g = _run_steps(dev, 6, B, dropout, stn=stn, use_graph=True, warmup_eager=2)
    assert len(set(lg)) == len(lg), "graph mode returned an aliased loss tensor"
    for a, b in zip(le, lg):
        assert abs(a - b) <= 1e-6 * abs(a), (le, lg)
    assert seed_e == seed_g
    assert torch.equal(se["nbt"], sg["nbt"]) and int(se["nbt"][0]) == 6
    for k in ("p", "m", "v", "bn"):
        d = float((se[k] - sg[k]).abs().max())
        assert d <= 1e-6, (k, d)
    assert abs(gn_e - gn_g) <= 1e-6 * gn_e


@pytest.mark.parametrize("si", [0, 1, 2])
def test_split_bf16_training_drift_against_the_fp64_yardstick(dev, si):
    """Multi-step drift of the default arithmetic, measured against float64: 12 training steps (B = 8, STN on, dropout off, fresh data
    every step, lr 1e-5) on the GPU with the split-bf16 kernel families AND with exact fp32 products (`tatt_amd.set_arithmetic`), both
    against the same 12 steps evaluated by the CPU oracle in float64 (tests/golden/drift_fp64.npz, tools/gen_golden_drift.py), three
    model / data seeds.  Rounds 4-5 compared the two GPU arithmetics with EACH OTHER and had to widen the bound when new kernels moved the
    late steps (a self-comparison inside the scatter of Adam's +-lr steps on zero-gradient parameters); against float64 each arithmetic
    has a distance of its own and the assertion is the one that matters: per step, the split-bf16 run is no further from float64 than
    K = 4 x the worst fp32 step so far is (plus a floor of 2e-6 relative for steps where fp32 happens to land on the yardstick).  Measured:
    the fp32 run itself is 5e-8 .. 2.4e-4 from float64 over the twelve steps and the split-bf16 run 1.5e-7 .. 2.3e-4 -- the late-step
    separation that rounds 4-5 attributed to the split kernels is the conditioning of the trajectory in ANY fp32 arithmetic.  lr = 1e-5 because at the recipe's 1e-3 the first steps of a fresh model amplify ANY perturbation a hundredfold within
    five steps (loss 37 -> 12 -> 15 -> 22 -> 31); there only the first two steps are compared (seed 0)."""
    import tatt_amd
    gold = np.load("tests/golden/drift_fp64.npz")
    seed = int(gold["seeds"][si])
    l64 = gold["losses"][si]
    n = int(gold["nstep"])
    assert int(gold["batch"]) == 8 and abs(float(gold["lr"]) - 1e-5) < 1e-12
    try:
        tatt_amd.set_arithmetic("fp32")
        l32, s32, _, _ = _run_steps(dev, n, 8, False, use_graph=False, lr=1e-5, model_seed=seed)
    finally:
        tatt_amd.set_arithmetic("split_bf16")
    lsb, ssb, _, _ = _run_steps(dev, n, 8, False, use_graph=False, lr=1e-5, model_seed=seed)
    e32 = np.abs(np.array(l32) - l64) / np.abs(l64)
    esb = np.abs(np.array(lsb) - l64) / np.abs(l64)
    print("seed %d, 12 steps at lr 1e-5, |loss - fp64| / |fp64| per step:\n  fp32       %s\n  split bf16 %s" % (
        seed, " ".join("%.1e" % v for v in e32), " ".join("%.1e" % v for v in esb)))
    K = 4.0
    run32 = np.maximum.accumulate(e32)                      # (the worst fp32 step so far: a single lucky fp32 step is not the yardstick)
    assert (esb <= K * run32 + 2e-6).all(), (e32, esb)
    assert esb.max() <= 1e-3 and e32.max() <= 1e-3, (e32, esb)     # (sanity only: measured <= 2.4e-4 for BOTH arithmetics, profiles/r06_drift_fp64.txt)
    # the weights: both arithmetics end at the same distance from each other as in rounds 4-5 (max-abs <= 12 lr: a parameter whose true
    # gradient is zero receives round-off as gradient and Adam turns either sign into a full lr step, in any arithmetic)
    dp = float((s32["p"] - ssb["p"]).abs().max())
    rp = float((s32["p"] - ssb["p"]).norm() / s32["p"].norm())
    assert dp <= 12 * 1e-5 * 1.01 and rp <= 1e-4, (dp, rp)
    wn = float(s32["p"].double().norm())
    assert abs(wn - float(gold["weight_norm"][si])) <= 1e-5 * wn, (wn, float(gold["weight_norm"][si]))
    if si == 0:
        try:
            tatt_amd.set_arithmetic("fp32")
            a, _, _, _ = _run_steps(dev, 2, 8, False, use_graph=False, lr=1e-3)
        finally:
            tatt_amd.set_arithmetic("split_bf16")
        b, _, _, _ = _run_steps(dev, 2, 8, False, use_graph=False, lr=1e-3)
        rel = max(abs(u - v) / abs(u) for u, v in zip(a, b))
        print("split-bf16 vs fp32, first 2 steps at lr 1e-3: loss rel %.3e" % rel)
        assert rel <= 1e-4, (a, b)


@pytest.mark.parametrize("B", [6, 48])
def test_staged_deferred_backward_equals_single_pass(dev, B):
    """Backward in eight stages (up-sampler, five SRBs, TP interpreter, block1 + STN) with the weight-gradient kernels and the
    query GRU's backward deferred to the side lane of each stage, against the plain single-pass backward: identical kernels on
    identical inputs, only the order in which fan-in gradients are added differs (fp32 round-off).  Compared after ONE step
    (Adam turns round-off on near-zero gradients into +-lr, so trajectories drift apart by construction): same loss, gradient
    norm to 1e-6, first moments (= 0.5 x gradient) to 2e-5 in l2 -- a race between the lanes, a stale packed filter or a lost
    gradient would not pass.  The lane layouts themselves (one stream / two streams, eager / hipGraph) run the same kernels in
    the same order: bit-identical over five steps."""
    l1, s1, _, g1 = _run_steps(dev, 1, B, True, use_graph=False, defer_param_grads=False)
    l0, s0, _, g0 = _run_steps(dev, 1, B, True, use_graph=False, defer_param_grads=True, side_stream=True)
    assert l1 == l0 and abs(g1 - g0) <= 1e-6 * g1, (l1, l0, g1, g0)
    # (the flat layouts agree: both follow grad_buckets() order)
    assert float((s1["m"] - s0["m"]).norm() / s1["m"].norm()) < 2e-5
    assert float((s1["bn"] - s0["bn"]).abs().max()) == 0.0 and torch.equal(s1["nbt"], s0["nbt"])
    l2, s2, _, g2 = _run_steps(dev, 5, B, True, use_graph=False, defer_param_grads=True, side_stream=True)
    l3, s3, _, g3 = _run_steps(dev, 5, B, True, use_graph=True, defer_param_grads=True, side_stream=True)
    l4, s4, _, g4 = _run_steps(dev, 5, B, True, use_graph=True, defer_param_grads=True, side_stream=False)
    assert l3 == l2 and l4 == l2
    for k in s2:
        assert torch.equal(s2[k], s3[k]) and torch.equal(s2[k], s4[k]), k


@pytest.mark.parametrize("hook,value", [("OUTCONV_BUCKET", "now"), ("OUTCONV_BUCKET", "trunk"), ("QGRU_BUCKET", "tp")])
def test_alternative_filings_of_deferred_work_compute_the_same_step(dev, monkeypatch, hook, value):
    """The measured-and-not-chosen places for the two late-filed pieces of side work (profiles/r05_ab_buckets.txt) stay correct: the 9x9 output
    convolution's weight gradient issued AT ONCE on the second stream beside the backward from the loss (`SIDE.immediate`: a side lane
    of the producing pass itself) or with its own stage, the query GRU's backward one pass earlier -- same loss, same gradient norm, same
    first moments as the default filing after one step, and graph replay == eager over five."""
    import tatt_amd.tsrn as T
    l0, s0, _, g0 = _run_steps(dev, 1, 6, True, use_graph=False)
    monkeypatch.setattr(T, hook, value)
    l1, s1, _, g1 = _run_steps(dev, 1, 6, True, use_graph=False)
    assert l1 == l0 and abs(g1 - g0) <= 1e-6 * g0, (l1, l0, g1, g0)
    l2, s2, _, _ = _run_steps(dev, 5, 6, True, use_graph=False)
    l3, s3, _, _ = _run_steps(dev, 5, 6, True, use_graph=True)
    assert l3 == l2
    for k in s2:
        assert torch.equal(s2[k], s3[k]), k


def test_single_rank_process_group_runs_the_staged_step(dev):
    """The data-parallel step (bucketed flat buffers, backward in stages, asynchronous RCCL all-reduce per bucket between the
    stage graphs, 1/world in Adam) with a world of ONE rank on this GPU equals the plain single-GPU step."""
    import torch.distributed as dist
    import socket
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)
    try:
        from tatt_amd.dp import rank_dropout_seed
        base = 77
        l0, s0, _, g0 = _run_steps(dev, 5, 4, True, use_graph=True, dropout_seed=rank_dropout_seed(base, 0))
        l1, s1, _, g1 = _run_steps(dev, 5, 4, True, use_graph=True, process_group=dist.group.WORLD, dropout_seed=base)
        l2, s2, _, g2 = _run_steps(dev, 3, 4, True, use_graph=False, process_group=dist.group.WORLD, dropout_seed=base)
        # which buckets go on the wire when: trunk + the five residual blocks after the pass that runs the TP interpreter's main
        # lane, the TP interpreter's while the STN head back-propagates, block1 (+ query GRU) and the STN head last
        from tatt_amd.train import Trainer
        m = build("TSRN_TL_TRANS", dev, **STD).train()
        tr = Trainer(m, use_graph=True, warmup_eager=1, process_group=dist.group.WORLD)
        x, tp, hr = make_inputs(4, seed=40)
        for _ in range(3):
            tr.step(x.to(dev), tp.to(dev), hr.to(dev))
        assert tr.stages == ["trunk", "srb4", "srb3", "srb2", "srb1", "srb0", "tp", "first", "stn"]
        assert tr.reduce_log == [(6, 0, 5), (7, 6, 6), (8, 7, 8)], tr.reduce_log
        sizes = [e - s for s, e in tr.flat.ranges]
        assert sizes[7] > 4.7e6 and len(tr._graphs["pass"]) == 3      # (the query GRU stays with block1: tatt_amd.tsrn.DP_QGRU_WITH_TP)
    finally:
        dist.destroy_process_group()
    # (the flat layouts differ -- bucket order -- so compare through the module's own tensors)
    for a, b in zip(l0, l1):
        assert abs(a - b) <= 1e-6 * abs(a), (l0, l1)
    for a, b in zip(l2, l1):
        assert abs(a - b) <= 1e-5 * abs(a), (l2, l1)
    assert float((s0["bn"] - s1["bn"]).abs().max()) <= 1e-6 and torch.equal(s0["nbt"], s1["nbt"])
    # weights and Adam moments tensor by tensor (canonical module order on both sides): the data-parallel path runs the same kernels
    # on the same inputs; only the fan-in order of the staged gradients may differ from the single graph (fp32 round-off on m,
    # and -- through Adam's normalisation -- at most a fraction of lr on a weight whose gradient is at round-off level)
    for k, tol in (("m", 2e-5), ("v", 2e-5)):
        assert float((s0[k] - s1[k]).norm() / s0[k].norm()) < tol, k
    assert float((s0["p"] - s1["p"]).abs().max()) <= 5 * 1e-3 * 1.001 and float((s0["p"] - s1["p"]).norm() / s0["p"].norm()) < 1e-4
    assert abs(g0 - g1) <= 1e-5 * g0


def test_b48_parity_eval_and_train_step(dev):
    """The benchmarked batch: because of the batch-axis query GRU (model/transformer_v2.py:201-221) the result depends on B and
    on the sample's index, so parity is pinned at B = 48 too: eval forward and one full training step (dropout off, STN off)
    against the oracle."""
    from tatt_amd.train import Trainer
    kw = dict(STD, STN=False)
    m = build("TSRN_TL_TRANS", dev, **kw)
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, tp, hr = make_inputs(48, seed=48)
    m.eval()
    with torch.no_grad():
        y, w = m(x.to(dev), tp.to(dev))
        o = O.generator_forward(sd0, x, tp, training=False, tatt=True, stn=False)
    assert max_err(y, o["sr"]) < 2e-5, max_err(y, o["sr"])
    assert max_err(w, o["pr_weights"]) < 1e-5
    # first and last sample see different query embeddings: make sure the test would notice a batch-axis mix-up
    assert max_err(o["sr"][0], O.generator_forward(sd0, x[:1], tp[:1], training=False, tatt=True, stn=False)["sr"][0]) > 1e-6
    m.train()
    m.infoGen.dropout_on = False
    tr = Trainer(m, use_graph=False)
    loss = tr.step(x.to(dev), tp.to(dev), hr.to(dev))
    o_loss, o_grads, o_sd1, _, o_out, o_total = O.train_step(sd0, x, tp, hr, tatt=True, stn=False)
    assert abs(float(loss) - float(o_loss)) < 1e-5 * abs(float(o_loss)), (float(loss), float(o_loss))
    assert abs(float(tr.last_grad_norm) - float(o_total)) < 1e-3 * float(o_total)
    worst = compare_param_grads(m.named_parameters(), o_grads, rtol=2e-3)
    print("B=48 worst relative gradient error vs oracle: %s %.3e" % worst)
    sd1 = m.state_dict()
    for k in sd1:
        if k.endswith(("running_mean", "running_var")):
            assert max_err(sd1[k], o_sd1[k]) < 1e-5, k
        elif k.endswith("num_batches_tracked"):
            assert int(sd1[k]) == int(o_sd1[k]), k
        elif not STRUCTURAL_ZERO_GRAD.match(k):
            d = float((sd1[k].cpu().float() - o_sd1[k].float()).abs().mean())
            assert d < 2e-4, (k, d)
    coef = min(1.0, 0.25 / (float(o_total) + 1e-6))
    assert coef < 0.5
    clipped = {k: (None if g is None else g * coef) for k, g in o_grads.items()}
    worst = compare_first_step_moments(tr, list(m.named_parameters()), clipped, rtol=2e-3)
    print("B=48 worst first-step moment vs oracle: %s %.3e" % worst)


LARGE = dict(scale_factor=2, width=256, height=64, STN=False, mask=True, srb_nums=5, hidden_units=32)


def test_large_tile_train_golden(dev):
    """BASELINE.json configs[4] geometry (LR 32x128 -> 64x256): train-mode forward + backward against the reference-generated
    vectors (tests/golden/large_train_b2.npz) and, tensor by tensor, against the oracle: query-GRU backward at hidden 1024,
    horizontal GRUs of 128 steps, 3x3 weight gradients with two 64-pixel segments per row, attention backward over 4096 queries."""
    from tatt_amd.train import image_loss
    z = np.load("tests/golden/large_train_b2.npz")
    m = build("TSRN_TL_TRANS", dev, **LARGE).train()
    m.infoGen.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, tp, hr = (torch.from_numpy(z[k]) for k in ("x", "tp", "hr"))
    sr, mid = m(x.to(dev), tp.to(dev))
    loss = image_loss(sr, hr.to(dev)).mean() * 100
    loss.backward()
    assert tuple(sr.shape) == (2, 4, 64, 256)
    assert max_err(sr, torch.from_numpy(z["sr"])) < SR_TRAIN_TOL, max_err(sr, torch.from_numpy(z["sr"]))
    assert abs(float(loss.detach()) - float(z["loss"])) < 1e-5 * float(z["loss"])
    assert max_err(mid["pr_weights"][:, ::16], torch.from_numpy(z["pr_weights"])) < 1e-5
    assert max_err(mid["trans_feat"][:, :4], torch.from_numpy(z["tp_map"])) < 2e-5
    params = dict(m.named_parameters())
    assert sorted(k for k, p in params.items() if p.grad is None) == sorted(z["none_keys"].tolist())
    scale = max(float(r[0]) for r in z["grad_summary"])
    for k, ref in zip(z["grad_keys"].tolist(), z["grad_summary"]):
        if STRUCTURAL_ZERO_GRAD.match(k):
            continue
        got = summarize(params[k].grad.cpu())
        assert abs(got[0] - ref[0]) < 2e-3 * ref[0] + 1e-7 * scale * params[k].numel() ** 0.5, (k, got[0], ref[0])
    for key in z.files:
        if key.startswith("g:"):
            e = rel_err(params[key[2:]].grad, torch.from_numpy(z[key]))
            assert e < 2e-3, (key, e)
    _, o_grads, o_sd1, _, _, _ = O.train_step(sd0, x, tp, hr, tatt=True, stn=False)
    worst = compare_param_grads(m.named_parameters(), o_grads, rtol=2e-3)
    print("large tile worst relative gradient error vs oracle: %s %.3e" % worst)
    sd1 = m.state_dict()
    assert max_err(sd1["block4.bn1.running_mean"], torch.from_numpy(z["bn_mean"])) < 1e-5
    assert max_err(sd1["block4.bn1.running_var"], torch.from_numpy(z["bn_var"])) < 1e-5


def test_large_tile_trainer_graph_step(dev):
    """The large-tile benchmark path itself (B = 16, hipGraph, dropout on) runs, and its first-step loss with dropout off is
    the reference's (tests/golden/bench_losses.json)."""
    import json
    from bench import make_batch, first_step_loss
    import tatt_amd
    torch.manual_seed(1234)
    m = tatt_amd.TSRN_TL_TRANS(**LARGE).to(dev).train()
    x, tp, hr = make_batch(16, 0, dev, 32, 128)
    ref = json.load(open("tests/golden/bench_losses.json"))["tatt_b16_32x128"]
    got = first_step_loss(m, x, tp, hr)
    assert abs(got - ref) < 2e-4 * ref, (got, ref)
    from tatt_amd.train import Trainer
    tr = Trainer(m, use_graph=True, warmup_eager=2)
    ls = [float(tr.step(x, tp, hr)) for _ in range(5)]
    assert all(l == l for l in ls) and ls[-1] < ls[0]


def test_gradients_vs_fp64(dev):
    """Conditioning, measured instead of argued: on the tatt_train_b4 case the distance of every HIP gradient from the fp64
    gradient of the same graph (oracle evaluated in float64, here) is held to a small multiple of the distance of the
    REFERENCE's own fp32 gradient from it (tests/golden/fp64_error_bars.npz, generated with the reference)."""
    from tatt_amd.train import image_loss
    z = np.load("tests/golden/tatt_train_b4.npz")
    bars = np.load("tests/golden/fp64_error_bars.npz")
    ref_err = dict(zip(bars["keys"].tolist(), bars["ref32_err"].tolist()))
    m = build("TSRN_TL_TRANS", dev, **STD).train()
    m.infoGen.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, hr, tp = (torch.from_numpy(z[k]) for k in ("x", "hr", "tp"))
    sr, _ = m(x.to(dev), tp.to(dev))
    (image_loss(sr, hr.to(dev)).mean() * 100).backward()
    l64, g64, _, _, _, _ = O.train_step_fp64(sd0, x, tp, hr, tatt=True, stn=True)
    # (the TPS buffers are built with an fp32 torch.inverse on THIS host's CPU: last-bit differences between machines, amplified
    # by the sampler, move even the fp64 loss by ~1e-6 relative)
    assert abs(float(l64) - float(bars["loss64"])) < 1e-5 * float(l64)
    scale = float(bars["scale"])
    rows = []
    for k, p in m.named_parameters():
        if p.grad is None:
            assert g64[k] is None, k
            continue
        d = g64[k]
        den = float(d.norm()) + 1e-7 * scale * d.numel() ** 0.5
        err = float((p.grad.detach().cpu().double() - d).norm()) / den
        # floor: tensors the reference itself gets to 1e-6 are allowed plain fp32 round-off of a different summation order (single
        # slopes -- one cancelling sum over 3 M products -- a little more)
        if STRUCTURAL_ZERO_GRAD.match(k):                 # mathematically zero: both sides are round-off noise
            continue
        # 3 x the reference's own distance, plus a floor for the tensors the reference happens to get to 1e-6: a k-ordered fp32
        # MFMA accumulation over 4096 pixels and oneDNN's blocked accumulation round differently (measured up to 2e-4 on 3x3 filters)
        lim = 3.0 * ref_err[k] + 5e-4
        rows.append((err / lim, k, err, ref_err[k]))
    rows.sort(reverse=True)
    for r in rows[:12]:
        print("fp64 yardstick  ratio %.2f  %-60s hip %.2e  ref32 %.2e" % r)
    assert rows[0][0] <= 1.0, rows[0]


def test_text_prior_sr_trainer_step_clips_per_model(dev):
    """TextPriorSR (tsrn_tl composition: the SR loss reaches the student) through the Trainer: the SR generator is clipped by ITS OWN gradient norm, the recogniser is not clipped
    (reference: `for model in model_list: clip_grad_norm_(model.parameters(), 0.25)`, interfaces/super_resolution.py:1082-1083,
    model_list holds the SR models only); post-Adam weights of both against the oracle composition."""
    import tatt_amd
    from oracle import crnn_oracle as C
    from tatt_amd.train import TextPriorSR, Trainer
    kw = dict(STD, STN=False)
    torch.manual_seed(1234)
    sr_m = tatt_amd.TSRN_TL_TRANS(**kw)
    sr_m.load_state_dict(randomize_state_dict(sr_m.state_dict()))
    tpg = tatt_amd.CRNN(32, 1, 37, 256)
    tpg.load_state_dict(randomize_state_dict(tpg.state_dict()))
    sd_sr = {k: v.detach().clone() for k, v in sr_m.state_dict().items()}
    sd_tpg = {k: v.detach().clone() for k, v in tpg.state_dict().items()}
    m = TextPriorSR(sr_m, tpg, detach_prior=False).to(dev).train()
    sr_m.infoGen.dropout_on = False
    x, _, hr = make_inputs(3, seed=11)
    tr = Trainer(m, use_graph=False)
    assert len(tr.groups) == 2 and tr.groups[1][2] == 0.0
    tr.step(x.to(dev), None, hr.to(dev))
    # oracle composition: one loss, two parameter sets
    lv_sr = {k: v.clone().requires_grad_(True) for k, v in sd_sr.items() if O.is_param(k)}
    lv_tp = {k: v.clone().requires_grad_(True) for k, v in sd_tpg.items() if v.is_floating_point() and not k.endswith(("running_mean", "running_var"))}
    prior = C.text_prior(C.crnn_forward(dict(sd_tpg, **lv_tp), C.parse_crnn_data(x), training=True))
    out = O.generator_forward(dict(sd_sr, **lv_sr), x, prior, training=True, tatt=True, stn=False)
    (O.image_loss(out["sr"], hr).mean() * 100).backward()
    g_sr = {k: v.grad for k, v in lv_sr.items() if v.grad is not None}
    clipped, total = O.clip_grad_norm(g_sr, 0.25)
    assert abs(float(tr.last_grad_norm) - float(total)) < 2e-3 * float(total), (float(tr.last_grad_norm), float(total))
    got_sr, got_tp = sr_m.state_dict(), tpg.state_dict()
    for k, g in clipped.items():
        if STRUCTURAL_ZERO_GRAD.match(k):
            continue
        p1, _, _ = O.adam_step(sd_sr[k], g, torch.zeros_like(g), torch.zeros_like(g), 1)
        assert float((got_sr[k].cpu() - p1).abs().mean()) < 2e-4, k
    moved = 0
    for k, v in lv_tp.items():
        if v.grad is None or k in ("cnn.conv2.bias", "cnn.conv4.bias", "cnn.conv6.bias"):
            continue
        p1, _, _ = O.adam_step(sd_tpg[k], v.grad, torch.zeros_like(v.grad), torch.zeros_like(v.grad), 1)   # NOT clipped
        d = float((got_tp[k].cpu() - p1).abs().mean())
        assert d < 3e-4, (k, d)
        moved += 1
    assert moved > 20
    # The weights above move by about lr with or without the clip.  The moments tell the groups apart: the generator's follow its
    # CLIPPED gradient, the recogniser's its unclipped one -- and on this input the two differ by far more than the limit.
    coef = float(torch.clamp(0.25 / (total + 1e-6), max=1.0))
    assert coef < 0.5, coef
    worst = compare_first_step_moments(tr, list(sr_m.named_parameters()), clipped, rtol=2e-3)
    print("generator worst first-step moment vs clipped oracle gradient: %s %.3e" % worst)
    # Limits for the recogniser, whose gradients compare_param_grads has none for.  The recurrent layers reach the loss through smooth
    # operations only: 5e-3, what tests/test_crnn.py holds them to through the SR composition.  Every cnn.* gradient passes the mask
    # of a ReLU or a max-pool whose input the product computes with 16-bit operand mantissas (2e-5 relative): an element within
    # that distance of the kink takes the other branch than in the oracle, and ONE such element among the 78 rows of a channel of
    # the last BatchNorm moves that channel's sums by a percent.  Measured with a fixed upstream gradient: 5e-5 on rnn.0, 3e-3 on
    # batchnorm6.bias behind the first mask, 6e-3 to 1.6e-2 on the convolutions; the fp32 oracle itself is 1e-2 from float64 on
    # conv0 .. conv4.  Hence 5e-2 there, the limit tests/test_crnn.py applies to the layers behind the pools.  A clipped recogniser
    # would be off by 1 - coef > 0.5.
    deep = ("rnn.",)
    g_tp = {k: v.grad for k, v in lv_tp.items()}
    worst = compare_first_step_moments(tr, list(tpg.named_parameters()), g_tp, rtol=5e-2,
                                       skip=("cnn.conv2.bias", "cnn.conv4.bias", "cnn.conv6.bias"),
                                       limit_of=lambda k: 5e-3 if k.startswith(deep) else 5e-2)
    print("recogniser worst first-step moment vs UNCLIPPED oracle gradient: %s %.3e" % worst)


def test_b48_stn_on_gradients_vs_fp64(dev):
    """The BENCHMARKED configuration -- B = 48, STN on -- pinned gradient by gradient: one training step through the product Trainer
    (staged two-lane backward, dropout off) against the fp64 gradients of the same graph, every tensor held to 3 x the distance of
    the REFERENCE's own fp32 gradient from fp64 at this batch (tests/golden/fp64_error_bars_b48.npz, generated with the
    reference by tools/gen_golden.py --only-fp64-b48) + the 5e-4 floor of test_gradients_vs_fp64."""
    from tatt_amd.train import Trainer
    bars = np.load("tests/golden/fp64_error_bars_b48.npz")
    ref_err = dict(zip(bars["keys"].tolist(), bars["ref32_err"].tolist()))
    m = build("TSRN_TL_TRANS", dev, **STD).train()
    m.infoGen.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, tp, hr = make_inputs(48, seed=48)
    tr = Trainer(m, use_graph=False)
    loss = tr.step(x.to(dev), tp.to(dev), hr.to(dev))
    l64, g64, _, _, _, _ = O.train_step_fp64(sd0, x, tp, hr, tatt=True, stn=True)
    assert abs(float(l64) - float(bars["loss64"])) < 1e-5 * float(l64)
    assert abs(float(loss) - float(l64)) < 2e-5 * float(l64), (float(loss), float(l64))
    scale = float(bars["scale"])
    rows = []
    for k, p in m.named_parameters():
        if p.grad is None:
            assert g64[k] is None, k
            continue
        if STRUCTURAL_ZERO_GRAD.match(k):
            continue
        d = g64[k]
        den = float(d.norm()) + 1e-7 * scale * d.numel() ** 0.5
        err = float((p.grad.detach().cpu().double() - d).norm()) / den
        lim = 3.0 * ref_err[k] + 5e-4
        rows.append((err / lim, k, err, ref_err[k]))
    rows.sort(reverse=True)
    for r in rows[:12]:
        print("fp64 yardstick B=48  ratio %.2f  %-60s hip %.2e  ref32 %.2e" % r)
    assert rows[0][0] <= 1.0, rows[0]


def test_tbsrn_b48_train_step_vs_oracle(dev):
    """configs[3] at its benchmarked batch: TBSRN, B = 48, LR 16x64, STN on, one training step (dropout off) against the oracle:
    SR, loss and every parameter gradient."""
    from tatt_amd.train import image_loss
    m = build("TBSRN", dev, scale_factor=2, width=128, height=32, STN=True, mask=True, input_channel=4).train()
    m.dropout_on = False
    sd0 = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    x, _, hr = make_inputs(48, seed=148)
    sr = m(x.to(dev))
    loss = image_loss(sr, hr.to(dev)).mean() * 100
    loss.backward()
    o_loss, o_grads, _, _, o_out, _ = O.train_step(sd0, x, None, hr, stn=True, tbsrn=True)
    assert max_err(sr, o_out["sr"]) < SR_TOL
    assert abs(float(loss.detach()) - float(o_loss)) < 1e-4 * abs(float(o_loss))
    compare_param_grads(m.named_parameters(), o_grads, rtol=1e-2, rtol_stn=1e-1)
