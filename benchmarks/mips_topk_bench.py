"""Exhaustive top-k: ops.mips_topk against torch.topk(q_bf16 @ corpus.T, k).

    python benchmarks/mips_topk_bench.py [--B 1 16 256 4096 --N 65536 1048576
                                          --D 64 128 256 --k 10 100]

Both paths are captured in a graph and timed over replays with device events;
the two alternate, `--repeats` timings each, and the median and the max-min
spread are reported. Points whose [B, N] bf16 score matrix would exceed
`--max-score-gib` are skipped for the torch chain (and marked so). For each
point one JSON line: both times, their ratio, and the corpus bytes / time of
the fused path as a share of the 6.3 TB/s achievable HBM bandwidth.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchrec_amd import ops  # noqa: E402

ACHIEVABLE_BW = 6.3e12


def _graph_of(fn, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    graph.replay()
    torch.cuda.synchronize()
    return graph


def _time_ms(graph, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--N", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--D", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-ms", type=float, default=40.0, help="work per timing")
    ap.add_argument("--max-score-gib", type=float, default=16.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mips_topk_bench needs a GPU"
    ops.hip_ops()

    torch.manual_seed(0)
    for N in args.N:
        for D in args.D:
            corpus = torch.randn(N, D, device="cuda").bfloat16()  # D % 32 == 0: no pad
            for B in args.B:
                q = torch.randn(B, D, device="cuda").bfloat16()
                for k in args.k:
                    paths = {"fused": lambda: ops.mips_topk(q, corpus, k)}
                    if B * N * 2 <= args.max_score_gib * 2 ** 30:
                        paths["torch"] = lambda: torch.topk(q @ corpus.t(), k)
                    graphs = {p: _graph_of(fn, args.warmup) for p, fn in paths.items()}
                    iters = {p: max(3, min(200, int(args.target_ms / _time_ms(g, 3))))
                             for p, g in graphs.items()}
                    times = {p: [] for p in graphs}
                    for _ in range(args.repeats):
                        for p, g in graphs.items():  # alternate the paths
                            times[p].append(_time_ms(g, iters[p]))
                    out = {"B": B, "N": N, "D": D, "k": k}
                    for p, ts in times.items():
                        out[f"{p}_ms"] = round(statistics.median(ts), 4)
                        out[f"{p}_spread_ms"] = round(max(ts) - min(ts), 4)
                    if "torch" in times:
                        out["torch_over_fused"] = round(out["torch_ms"] / out["fused_ms"], 2)
                    else:
                        out["torch_ms"] = "skipped: score matrix too large"
                    out["fused_corpus_bw_share"] = round(
                        N * D * 2 / (out["fused_ms"] * 1e-3) / ACHIEVABLE_BW, 3)
                    print(json.dumps(out), flush=True)
                    del graphs


if __name__ == "__main__":
    main()
