"""Throughput of the eval / test loop: the eager `tatt_amd.io.evaluate` against the graph-captured `tatt_amd.infer.evaluate_session`,
and the one-launch LSTM layer against the per-step kernels.  Reports only (one JSON line per case), asserts nothing.

    python tools/bench_infer.py [--steps 20] [--warmup 3] [--repeats 5] [--full-metrics]

Timing as bench.py: warm-up, device-synchronised, median of repeats.  Cases:
  tatt_crnn_b48  TATT with a CRNN prior and a CRNN recogniser (accuracies of SR / LR / HR), B = 48
  tatt_b1        TATT with the CRNN prior at B = 1 (the reference's demo())
  tsrn_b48       TSRN, PSNR / SSIM only, B = 48
  lstm_b48       one BiLSTM layer of the CRNN (T = 26, H = 256): chain vs per-step launches, same process and data
--full-metrics runs ONE case instead: tatt_crnn_b48 through `evaluate_session` with and without `full_metrics=True` (bicubic LR
baseline, edit distances, per-image records), alternating in one process; min / median / max of the repeats and the kernel nodes
of either graph.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def _timed(fn, steps, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) / steps)
    return statistics.median(ts)


def _models(dev, tatt):
    import tatt_amd
    from oracle.fixtures import randomize_state_dict
    torch.manual_seed(1234)
    kw = dict(scale_factor=2, width=128, height=32, STN=True, mask=True, srb_nums=5, hidden_units=32)
    g = (tatt_amd.TSRN_TL_TRANS if tatt else tatt_amd.TSRN)(**kw)
    g.load_state_dict(randomize_state_dict(g.state_dict()))
    c = tatt_amd.CRNN(32, 1, 37, 256)
    c.load_state_dict(randomize_state_dict(c.state_dict(), seed=5))
    return g.to(dev).eval(), c.to(dev).eval()


def _batches(dev, B, n, labels):
    from oracle.fixtures import make_inputs
    out = []
    for i in range(n):
        x, _, hr = make_inputs(B, seed=100 + i)
        b = (x.to(dev), hr.to(dev), None)
        out.append(b + ((["word"] * B),) if labels else b)
    return out


def bench_loop(name, dev, tatt, B, use_prior, use_rec, args):
    from tatt_amd.crnn import parse_crnn_data, text_prior
    from tatt_amd.infer import evaluate_session
    from tatt_amd.io import evaluate
    g, c = _models(dev, tatt)
    batches = _batches(dev, B, args.steps, use_rec)
    prior_fn = (lambda lr: text_prior(c(parse_crnn_data(lr)))) if use_prior else None
    sessions = {}
    eager = _timed(lambda: evaluate(g, batches, prior_fn=prior_fn, recognizer=c if use_rec else None), 1, args.warmup, args.repeats)
    sess = _timed(lambda: evaluate_session(g, batches, prior=c if use_prior else None, recognizer=c if use_rec else None,
                                           sessions=sessions), 1, args.warmup, args.repeats)
    n_img = B * args.steps
    print(json.dumps({"case": name, "B": B, "batches": args.steps, "eager_ms_per_batch": round(1e3 * eager / args.steps, 3),
                      "session_ms_per_batch": round(1e3 * sess / args.steps, 3), "eager_img_s": round(n_img / eager, 1),
                      "session_img_s": round(n_img / sess, 1), "speedup": round(eager / sess, 2)}), flush=True)


def _graph_kernel_nodes(session):
    """Kernel nodes of the session's graph: its forward captured once more into a graph that keeps its hipGraph_t, whose nodes the
    HIP runtime lists (hipGraphGetNodes / hipGraphNodeGetType; type 0 is a kernel launch)."""
    import ctypes
    from tatt_amd import functional as Fh
    with open("/proc/self/maps") as f:                                    # the runtime torch already loaded, not a second copy
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    g = torch.cuda.CUDAGraph(keep_graph=True)
    fork = (Fh.FWD_FORK.enabled, Fh.FWD_FORK_B.enabled)
    Fh.FWD_FORK.enabled = Fh.FWD_FORK_B.enabled = False                   # as InferenceSession.run captures
    try:
        with torch.no_grad(), torch.cuda.graph(g):
            session._forward()
    finally:
        Fh.FWD_FORK.enabled, Fh.FWD_FORK_B.enabled = fork
    graph, n = ctypes.c_void_p(g.raw_cuda_graph()), ctypes.c_size_t(0)
    if hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    nodes = (ctypes.c_void_p * n.value)()
    if hip.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) != 0:
        raise RuntimeError("hipGraphGetNodes failed")
    kernels = 0
    for node in nodes:
        kind = ctypes.c_int(-1)
        if hip.hipGraphNodeGetType(ctypes.c_void_p(node), ctypes.byref(kind)) != 0:
            raise RuntimeError("hipGraphNodeGetType failed")
        kernels += kind.value == 0
    return kernels


def bench_full_metrics(dev, args, B=48):
    from tatt_amd.infer import evaluate_session
    g, c = _models(dev, True)
    batches = _batches(dev, B, args.steps, True)
    sessions = {}
    run = {full: (lambda full=full: evaluate_session(g, batches, prior=c, recognizer=c, sessions=sessions, full_metrics=full))
           for full in (False, True)}
    for _ in range(args.warmup):
        for full in (False, True):
            run[full]()
    torch.cuda.synchronize()
    ts = {False: [], True: []}
    for _ in range(args.repeats):                                         # alternating: both see the same machine state
        for full in (False, True):
            t0 = time.perf_counter()
            run[full]()                                                   # (ends in the host read of the totals)
            torch.cuda.synchronize()
            ts[full].append(1e3 * (time.perf_counter() - t0) / args.steps)
    launches = {}
    for key, s in sessions.items():
        try:
            launches[s.full_metrics] = _graph_kernel_nodes(s)
        except Exception as e:                                            # a report, not a check
            launches[s.full_metrics] = "not measured (%s: %s)" % (type(e).__name__, e)
    stat = lambda v: {"min": round(min(v), 3), "median": round(statistics.median(v), 3), "max": round(max(v), 3)}
    print(json.dumps({"case": "tatt_crnn_b48_full_metrics", "B": B, "batches": args.steps, "repeats": args.repeats,
                      "session_ms_per_batch": stat(ts[False]), "full_metrics_ms_per_batch": stat(ts[True]),
                      "graph_launches": launches.get(False), "full_metrics_graph_launches": launches.get(True)}), flush=True)


def bench_lstm(dev, args, B=48, T=26):
    from tatt_amd.infer import bilstm_eval
    torch.manual_seed(0)
    rnn = torch.nn.LSTM(512, 256, bidirectional=True).to(dev)
    x = torch.randn(T, B, 512, device=dev)
    sync = torch.zeros(1024, dtype=torch.int32, device=dev)
    res = {}
    with torch.no_grad():
        for chain in (True, False):
            res[chain] = _timed(lambda: bilstm_eval(x, rnn, sync, chain=chain), args.steps, args.warmup, args.repeats)
        graphs = {}
        for chain in (True, False):                                       # as replayed inside the session's graph
            bilstm_eval(x, rnn, sync, chain=chain)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                bilstm_eval(x, rnn, sync, chain=chain)
            graphs[chain] = _timed(gr.replay, args.steps, args.warmup, args.repeats)
    print(json.dumps({"case": "lstm_b%d" % B, "T": T, "H": 256, "chain_us": round(1e6 * res[True], 1),
                      "per_step_us": round(1e6 * res[False], 1), "chain_graph_us": round(1e6 * graphs[True], 1),
                      "per_step_graph_us": round(1e6 * graphs[False], 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20, help="batches per timed loop")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", default="", help="comma-separated case names")
    ap.add_argument("--full-metrics", action="store_true", help="time evaluate_session with and without full_metrics=True instead")
    args = ap.parse_args()
    import __graft_entry__
    __graft_entry__.build()
    dev = torch.device("cuda:0")
    if args.full_metrics:
        bench_full_metrics(dev, args)
        import tatt_amd
        tatt_amd.sync_check()
        return
    only = set(filter(None, args.only.split(",")))
    cases = [("tatt_crnn_b48", True, 48, True, True), ("tatt_b1", True, 1, True, False), ("tsrn_b48", False, 48, False, False)]
    for name, tatt, B, pr, rec in cases:
        if not only or name in only:
            bench_loop(name, dev, tatt, B, pr, rec, args)
    if not only or "lstm_b48" in only:
        bench_lstm(dev, args)
    import tatt_amd
    tatt_amd.sync_check()


if __name__ == "__main__":
    main()
