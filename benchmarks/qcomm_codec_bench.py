"""MXFP8 / MXFP4 qcomm codec: the HIP kernels against what they replace.

    python benchmarks/qcomm_codec_bench.py [--batch 8192 --blocks 8]

The message is the pooled all-to-all's at bench.py's default model:
W * B * D_local fp32 values with W = 1 and D_local = tables * EMB_DIM.

Flat mode, per format, encode and decode:
  hip    the qcomm_codec.hip kernel
  eager  the plain-PyTorch reference functions run on GPU tensors (the chain
         of elementwise launches a codec written in torch ops costs)
  bf16   t.to(bfloat16) / .to(float32), the cheapest existing compressed wire
Slab mode, with the columns split into --blocks rank blocks:
  slab   one kernel, gather / paste folded in
  flat+copy  slice + cat then flat encode; flat decode then view + cat(dim=1)

Device-event timing after warm-up; the paths of a comparison alternate inside
one call, --repeats timings each, reported as median and max-min spread. Each
path cycles through four input buffers (more than the 256 MB of last-level
cache) so no path is timed on cache-resident data. Bytes are computed from
the shapes: 4 n in and 33 n / 32 or 17 n / 32 out for encode, the reverse for
decode; the share of peak is those bytes over the time against 8 TB/s HBM3E.
Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import DLRM_EMB_ROWS, EMB_DIM  # noqa: E402
from torchrec_amd import ops  # noqa: E402
from torchrec_amd.distributed import qcomm_codecs as qc  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s
GROUP_BYTES = {"mxfp8": 33, "mxfp4": 17}
NBUF = 4


def _time_ms(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for i in range(iters):
        fn(i % NBUF)
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters


def _compare(paths, iters, warmup, repeats):
    """paths: name -> fn(buffer index). Alternates the paths; ms median/spread."""
    for fn in paths.values():
        for i in range(warmup):
            fn(i % NBUF)
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for k, fn in paths.items():
            times[k].append(_time_ms(fn, iters))
    return {
        k: {"median": round(statistics.median(ts), 4), "spread": round(max(ts) - min(ts), 4)}
        for k, ts in times.items()
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "qcomm_codec_bench needs a GPU"

    torch.manual_seed(0)
    B, F = args.batch, len(DLRM_EMB_ROWS)
    sum_D = F * EMB_DIM
    n = B * sum_D
    per = [F // args.blocks + (1 if r < F % args.blocks else 0) for r in range(args.blocks)]
    dims = [t * EMB_DIM for t in per]
    mats = [torch.randn(B, sum_D, device="cuda") for _ in range(NBUF)]
    flats = [m.view(-1) for m in mats]
    half = [f.to(torch.bfloat16) for f in flats]
    out = {"shape": {"B": B, "D_local": sum_D, "numel": n, "block_dims": dims}, "iters": args.iters}

    for fmt in ("mxfp8", "mxfp4"):
        wire_bytes = n // 32 * GROUP_BYTES[fmt]
        moved = 4 * n + wire_bytes
        wires = [ops.qcomm_mx_encode(f, fmt) for f in flats]
        swires = [ops.qcomm_mx_encode(m, fmt, block_dims=dims) for m in mats]
        res = {"bytes_moved": moved}
        res["encode_ms"] = _compare(
            {
                "hip": lambda i: ops.qcomm_mx_encode(flats[i], fmt),
                "eager": lambda i: qc.mx_encode_reference(flats[i], fmt),
                "bf16": lambda i: flats[i].to(torch.bfloat16),
            },
            args.iters, args.warmup, args.repeats,
        )
        res["decode_ms"] = _compare(
            {
                "hip": lambda i: ops.qcomm_mx_decode(wires[i], n, fmt),
                "eager": lambda i: qc.mx_decode_reference(wires[i], n, fmt),
                "bf16": lambda i: half[i].to(torch.float32),
            },
            args.iters, args.warmup, args.repeats,
        )
        res["slab_encode_ms"] = _compare(
            {
                "slab": lambda i: ops.qcomm_mx_encode(mats[i], fmt, block_dims=dims),
                "flat+copy": lambda i: ops.qcomm_mx_encode(
                    qc._gather_pooled_blocks(mats[i], dims), fmt
                ),
            },
            args.iters, args.warmup, args.repeats,
        )
        res["slab_decode_ms"] = _compare(
            {
                "slab": lambda i: ops.qcomm_mx_decode(swires[i], n, fmt, block_dims=dims, B=B),
                "flat+copy": lambda i: qc._paste_pooled_blocks(
                    ops.qcomm_mx_decode(swires[i], n, fmt), B, dims
                ),
            },
            args.iters, args.warmup, args.repeats,
        )
        for k in ("encode_ms", "decode_ms"):
            bw = moved / (res[k]["hip"]["median"] * 1e-3)
            res[k]["hip_tb_per_s"] = round(bw / 1e12, 2)
            res[k]["hip_share_of_hbm_peak"] = round(bw / HBM_PEAK, 3)
        out[fmt] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
