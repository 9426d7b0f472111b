"""Per-layer cost of the MLP backward's non-GEMM tail at the flagship batch.

For the seven ReLU layers of the DLRM dense/over arch (M = 8192, bf16) this
times, in one process, three equivalent chains that turn (dy, y, split-K
chunks) into (g, db, dW); the bmm itself is left out:

  torch : g = dy * (y > 0); db = g.sum(0); dW = parts.sum(0)
  colsum: relu_bwd_col_sum (partial + final fold) + parts.sum(0)
  pair  : relu_bwd_colsum_partial + splitk_fold_bias        (two kernels)

Each chain is captured REPS times into a hipGraph and replayed, so the figure
is GPU time per chain without launch overhead, as in the captured train step.
One JSON line per layer."""

import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from torchrec_amd import ops

ops.hip_ops()
T = torch.ops.trec_amd

M, S, REPS, REPLAYS = 8192, 8, 20, 10
# (N, K) of each Linear+ReLU: dense arch 13-512-256-128, over arch 479-1024-1024-512-256
LAYERS = [(512, 13), (256, 512), (128, 256), (1024, 479), (1024, 1024), (512, 1024), (256, 512)]


def graph_us(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(REPS):
            keep = fn()  # noqa: F841
    graph.replay()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(REPLAYS):
        graph.replay()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / (REPS * REPLAYS)


def main():
    torch.manual_seed(0)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    for N, K in LAYERS:
        y = torch.randn(M, N, **bf).relu()
        dy = torch.randn(M, N, **bf)
        parts = torch.randn(S, N, K, **bf)

        def chain_torch():
            g = dy * (y > 0)
            return g, g.sum(0), parts.sum(0)

        def chain_colsum():
            g, db = T.relu_bwd_col_sum(dy, y)
            return g, db, parts.sum(0)

        def chain_pair():
            g, partial = T.relu_bwd_colsum_partial(dy, y)
            dw, db = T.splitk_fold_bias(parts, partial)
            return g, db, dw

        # bytes the work needs: read dy, y, write g; read S chunks, write one
        need = (3 * M * N + (S + 1) * N * K) * 2
        row = {"M": M, "N": N, "K": K, "needed_MB": round(need / 1e6, 2)}
        for name, fn in (("torch", chain_torch), ("colsum", chain_colsum), ("pair", chain_pair)):
            row[f"{name}_us"] = round(graph_us(fn), 2)
        row["pair_GBps"] = round(need / row["pair_us"] / 1e3, 0)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
