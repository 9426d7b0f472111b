"""IVF-Flat search (coarse ops.mips_topk over the centroids + ops.ivf_topk
over the probed lists) against the exhaustive ops.mips_topk over the same
corpus, same build, same run.

    python benchmarks/ivf_topk_bench.py [--B 1 16 256 4096 --N 1048576 --D 128
                                         --k 10 100 --nlist 1024 --nprobe 1 8 32]

The corpus is a mixture of `--clusters` Gaussians, the queries are corpus rows
plus noise, the metric is L2, and the rows are filed by IVFFlatIndex (k-means,
`--niter`). Both paths are captured in a graph and timed over replays with
device events; they alternate, `--repeats` timings each, and the median and
the max-min spread are reported. One JSON line per point: both times, their
ratio, the recall of the IVF result against the exhaustive one, and the bytes
of list rows the scan kernel reads (a list once per 32 queries that probe it)
/ time as a share of the 6.3 TB/s achievable HBM bandwidth.

`--profile B K NPROBE` instead runs the IVF search of that one point eagerly
`--profile-iters` times, for a kernel trace (rocprofv3 --kernel-trace -- python
...) that splits the time into the coarse, plan, scan and merge kernels. The
coarse stage is the mips_topk_partial_kernel calls that are not part of
building the index: take the median per kernel name.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from benchmarks.mips_topk_bench import ACHIEVABLE_BW, _graph_of, _time_ms  # noqa: E402
from torchrec_amd import ops  # noqa: E402
from torchrec_amd.modules import IVFFlatIndex  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 256, 4096])
    ap.add_argument("--N", type=int, default=1048576)
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--niter", type=int, default=4)
    ap.add_argument("--clusters", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--target-ms", type=float, default=40.0, help="work per timing")
    ap.add_argument("--profile", type=int, nargs=3, metavar=("B", "K", "NPROBE"))
    ap.add_argument("--profile-iters", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "ivf_topk_bench needs a GPU"
    ops.hip_ops()

    torch.manual_seed(0)
    N, D = args.N, args.D
    index = IVFFlatIndex(D, args.nlist, metric="l2", device=torch.device("cuda"))
    centres = torch.randn(args.clusters, D, device="cuda")
    data = centres[torch.randint(0, args.clusters, (N,), device="cuda")]
    data += 0.5 * torch.randn(N, D, device="cuda")
    index.train(data[: min(N, 64 * args.nlist)], niter=args.niter)
    index.add(data)
    index._regroup()
    corpus, offsets, cent = index.corpus[:N], index.list_offsets, index.centroids
    bias, cent_bias = index.bias[:N], index.centroid_bias
    lengths = offsets.diff()
    row_bytes = corpus.shape[1] * 2
    print(json.dumps({"N": N, "D": D, "nlist": args.nlist, "list_rows_min": int(lengths.min()),
                      "list_rows_max": int(lengths.max())}), flush=True)

    def ivf(q, k, nprobe):
        probes = ops.mips_topk(q, cent, nprobe, cent_bias)[1]
        return ops.ivf_topk(q, corpus, offsets, probes, k, bias)

    def queries(B):
        rows = data[torch.randint(0, N, (B,), device="cuda")]
        return (rows + 0.1 * torch.randn(B, D, device="cuda")).bfloat16()

    if args.profile:
        B, k, nprobe = args.profile
        q = queries(B)
        for _ in range(args.profile_iters):
            ivf(q, k, nprobe)
        torch.cuda.synchronize()
        return

    for B in args.B:
        q = queries(B)
        for k in args.k:
            flat_rows = ops.mips_topk(q, corpus, k, bias)[1]
            for nprobe in args.nprobe:
                paths = {"ivf": lambda: ivf(q, k, nprobe),
                         "flat": lambda: ops.mips_topk(q, corpus, k, bias)}
                graphs = {p: _graph_of(fn, args.warmup) for p, fn in paths.items()}
                iters = {p: max(3, min(200, int(args.target_ms / _time_ms(g, 3))))
                         for p, g in graphs.items()}
                times = {p: [] for p in graphs}
                for _ in range(args.repeats):
                    for p, g in graphs.items():  # alternate the paths
                        times[p].append(_time_ms(g, iters[p]))
                out = {"B": B, "k": k, "nprobe": nprobe}
                for p, ts in times.items():
                    out[f"{p}_ms"] = round(statistics.median(ts), 4)
                    out[f"{p}_spread_ms"] = round(max(ts) - min(ts), 4)
                out["flat_over_ivf"] = round(out["flat_ms"] / out["ivf_ms"], 2)
                probes = ops.mips_topk(q, cent, nprobe, cent_bias)[1]
                rows = ops.ivf_topk(q, corpus, offsets, probes, k, bias)[1]
                hit = (rows[:, :, None] == flat_rows[:, None, :]).any(dim=2)
                out["recall"] = round(hit.float().mean().item(), 3)
                tiles = (torch.bincount(probes.reshape(-1), minlength=args.nlist) + 31) // 32
                read = int((tiles * lengths).sum()) * row_bytes
                out["ivf_list_bw_share"] = round(read / (out["ivf_ms"] * 1e-3) / ACHIEVABLE_BW, 3)
                print(json.dumps(out), flush=True)
                del graphs


if __name__ == "__main__":
    main()
