"""LowRankCrossNet: eager torch chain against the fused MFMA kernels.

    python benchmarks/crossnet_bench.py [--batch 8192 --features 3456 --rank 512 --layers 3]

Forward (no_grad) and forward+backward, bf16, device-event timing after
warm-up. The two paths alternate inside one process, five timings each;
reported are the median and the max-min spread per path, plus the fused
forward's achieved FLOP/s from 4*B*N*r per layer. A difference between the
paths counts only if it exceeds the spread. Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from torchrec_amd.models.dlrm import LowRankCrossNet  # noqa: E402


def _time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--features", type=int, default=3456)
    ap.add_argument("--rank", type=int, default=512)
    ap.add_argument("--layers", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "crossnet_bench needs a GPU"

    torch.manual_seed(0)
    B, N, r, L = args.batch, args.features, args.rank, args.layers
    net = LowRankCrossNet(N, L, r).to(device="cuda", dtype=torch.bfloat16)
    x = torch.randn(B, N, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    g = torch.randn(B, N, device="cuda", dtype=torch.bfloat16)
    os.environ.pop("TREC_CROSSNET_EAGER", None)

    def run(eager, backward):
        os.environ["TREC_CROSSNET_FUSED"] = "0" if eager else "1"
        if backward:
            net(x).backward(g)
            x.grad = None
            net.zero_grad(set_to_none=True)
        else:
            with torch.no_grad():
                net(x)

    out = {"shape": {"B": B, "N": N, "r": r, "L": L}, "dtype": "bf16", "iters": args.iters}
    for mode, backward in (("fwd", False), ("fwd_bwd", True)):
        times = {"eager": [], "fused": []}
        for path in times:
            for _ in range(args.warmup):
                run(path == "eager", backward)
        torch.cuda.synchronize()
        for _ in range(args.repeats):
            for path in times:  # alternate the two paths
                times[path].append(_time_ms(lambda: run(path == "eager", backward), args.iters))
        for path, ts in times.items():
            out[f"{mode}_{path}_ms"] = {
                "median": round(statistics.median(ts), 4),
                "spread": round(max(ts) - min(ts), 4),
            }
    flops = 4.0 * B * N * r * L
    out["fused_fwd_tflops"] = round(flops / (out["fwd_fused_ms"]["median"] * 1e-3) / 1e12, 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
