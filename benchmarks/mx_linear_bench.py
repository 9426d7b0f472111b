"""MXFP8 dense layers (mx_linear.hip) against what serving runs today.

    python benchmarks/mx_linear_bench.py [--batches 16 256 4096]

Layer shapes are bench.py's DLRM: the dense arch NUM_DENSE -> DENSE_ARCH and
the over arch (EMB_DIM + pairs of the 26 + 1 features) -> OVER_ARCH, ReLU on
every layer but the over arch's last, which is a plain nn.Linear. Per batch
size M and per Perceptron layer, and for each arch as a whole chain:
  fp32   relu(linear) under inference_mode, what an unquantized model serves
  bf16   the same with bf16 weights and activations
  mxfp8  ops.mx_linear on packed weights, fp32 in and out (``mxfp8_bf16``:
         bf16 between the layers of a chain; bf16 in and out for one layer;
         ``mxfp8_act``: the MXFP8 codes and scales themselves between the
         layers of a chain, in and out for one layer)
  mxfp4  the same with MXFP4 weights (``weight_format="mxfp4"``), fp32 in and
         out; ``mxfp4_act``: MXFP4 weights with the MXFP8 pair between the
         layers, what quantize_dense(weight_format="mxfp4",
         activation_format="mxfp8") serves
The mx chains are what quantize_dense serves: the last Perceptron of an arch
returns fp32 and the over arch's final nn.Linear stays an fp32 linear, which
also keeps its fp32 weight bytes.

A timing is a device-event window around --iters back-to-back calls of the
path (a whole chain of calls, never one launch), after warm-up; the paths of
a comparison alternate, --repeats windows each, reported as median and
max - min spread in microseconds per call. ``--graph`` replays the window
from a captured graph instead, which takes the host's launch cost out.
Weight bytes are computed from the shapes: 4 N K (fp32), 2 N K (bf16),
N Kp + N Kp / 32 (MXFP8 codes and scale bytes, Kp = K rounded up to 128) and
N Kp / 2 + N Kp / 32 (MXFP4).
Prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench import DENSE_ARCH, DLRM_EMB_ROWS, EMB_DIM, NUM_DENSE, OVER_ARCH  # noqa: E402
from torchrec_amd import ops  # noqa: E402


def _layers(in_size, sizes, last_is_perceptron):
    """(K, N, relu, quantized): the over arch ends in a plain nn.Linear."""
    dims = [in_size] + list(sizes)
    return [(dims[i], dims[i + 1], p, p)
            for i in range(len(sizes)) for p in [last_is_perceptron or i + 2 < len(dims)]]


def _window(fn, iters, graph):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    if graph:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(iters):
                fn()
        g.replay()
        torch.cuda.synchronize()
        run = g.replay
    else:
        def run():
            for _ in range(iters):
                fn()
    def timed():
        start.record()
        run()
        end.record()
        end.synchronize()
        return start.elapsed_time(end) * 1e3 / iters
    return timed


def _compare(paths, iters, warmup, repeats, graph):
    for fn in paths.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    timed = {k: _window(fn, iters, graph) for k, fn in paths.items()}
    times = {k: [] for k in paths}
    for _ in range(repeats):
        for k, t in timed.items():
            times[k].append(t())
    return {
        k: {"median_us": round(statistics.median(ts), 2), "spread_us": round(max(ts) - min(ts), 2)}
        for k, ts in times.items()
    }


def _paths(layers, M, as_served=True):
    """name -> fn running the whole chain of ``layers`` once at batch M."""
    ws = [torch.randn(n, k, device="cuda") / k ** 0.5 for k, n, _, _ in layers]
    bs = [torch.randn(n, device="cuda") / 8 for _, n, _, _ in layers]
    wh, bh = [w.bfloat16() for w in ws], [b.bfloat16() for b in bs]
    packed = {f: [ops.mx_linear_pack_weight(w, f) for w in ws] for f in ("mxfp8", "mxfp4")}
    x = torch.randn(M, layers[0][0], device="cuda")
    xh = x.bfloat16()

    def eager(x0, weights, biases):
        def run():
            h = x0
            for (_, _, relu, _), w, b in zip(layers, weights, biases):
                h = torch.nn.functional.linear(h, w, b)
                h = torch.relu(h) if relu else h
            return h
        return run

    # as_served, what quantize_dense builds: the layers of an MLP hand each
    # other ``dtype``, the last of them returns fp32, and the over arch's
    # final nn.Linear (not a Perceptron) stays an fp32 linear. A layer timed
    # on its own emits ``dtype``.
    last_q = max(i for i, layer in enumerate(layers) if layer[3]) if as_served else -1

    def mx(x0, dtype, fmt="mxfp8"):
        def run():
            h = x0
            for i, ((k, _, relu, quant), (c, s), w, b) in enumerate(
                    zip(layers, packed[fmt], ws, bs)):
                if quant:
                    h = ops.mx_linear(h, c, s, b, k, relu=relu, weight_format=fmt,
                                      output_dtype=torch.float32 if i == last_q else dtype)
                else:
                    h = torch.nn.functional.linear(h, w, b)
            return h
        return run

    # activation_format="mxfp8": the quantized layers hand each other the
    # MXFP8 pair. Served, the first reads fp32 and the last returns fp32; a
    # layer timed on its own reads a pair (x packed like a weight) and emits one.
    xq = ops.MxActivation(*ops.mx_linear_pack_weight(x), layers[0][0])

    def mx_act(fmt="mxfp8"):
        def run():
            h = x if as_served else xq
            for i, ((k, _, relu, quant), (c, s), w, b) in enumerate(
                    zip(layers, packed[fmt], ws, bs)):
                if quant:
                    h = ops.mx_linear(h, c, s, b, k, relu=relu, weight_format=fmt,
                                      output_format=None if i == last_q else "mxfp8")
                else:
                    h = torch.nn.functional.linear(h, w, b)
            return h
        return run

    return {
        "fp32": eager(x, ws, bs),
        "bf16": eager(xh, wh, bh),
        "mxfp8": mx(x, torch.float32),
        # served, the float neighbours hand the first layer fp32
        "mxfp8_bf16": mx(x if as_served else xh, torch.bfloat16),
        "mxfp8_act": mx_act(),
        "mxfp4": mx(x, torch.float32, "mxfp4"),
        "mxfp4_act": mx_act("mxfp4"),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--graph", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "mx_linear_bench needs a GPU"

    torch.manual_seed(0)
    F = len(DLRM_EMB_ROWS)
    archs = {
        "dense_arch": _layers(NUM_DENSE, DENSE_ARCH, True),
        "over_arch": _layers(EMB_DIM + (F + 1) * F // 2, OVER_ARCH, False),
    }
    out = {"iters": args.iters, "graph": args.graph, "weight_bytes": {}, "us_per_call": {}}
    for k, n, _, quant in archs["dense_arch"] + archs["over_arch"]:
        kp = -(-k // ops.MX_LINEAR_K_STEP) * ops.MX_LINEAR_K_STEP
        out["weight_bytes"][f"{k}x{n}"] = {
            "fp32": 4 * n * k, "bf16": 2 * n * k,
            "mxfp8": n * kp + n * kp // 32 if quant else 4 * n * k,
            "mxfp4": n * kp // 2 + n * kp // 32 if quant else 4 * n * k,
        }
    with torch.inference_mode():
        for M in args.batches:
            res = {}
            for name, layers in archs.items():
                res[name] = _compare(_paths(layers, M), args.iters, args.warmup, args.repeats,
                                     args.graph)
                for layer in layers:
                    if layer[3]:
                        res[f"{layer[0]}x{layer[1]}"] = _compare(
                            _paths([layer], M, as_served=False), args.iters, args.warmup,
                            args.repeats, args.graph)
            out["us_per_call"][f"M={M}"] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
