"""Micro-benchmarks for the CDNA4 HIP kernels (reference parity:
torchrec/distributed/benchmark/ + FBGEMM TBE device benchmarks).

Run on an MI355X:
    python benchmarks/tbe_bench.py            # all suites
    python benchmarks/tbe_bench.py --suite tbe
    python benchmarks/tbe_bench.py --update-rows   # in-place row update vs table reload
    python benchmarks/tbe_bench.py --checked       # bounds-checked / pruned quant lookup
Prints one JSON line per measurement.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch


def _time_kernel(fn, iters=50, warmup=10) -> float:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us


def _time_graph(fn, calls=50, replays=400) -> float:
    """Device time of one ``fn()``: ``calls`` of them captured in one graph,
    so the host's enqueue cost is paid once per replay, not per call."""
    fn()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(calls):
            fn()
    graph.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(replays):
        graph.replay()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (replays * calls) * 1e6  # us


def bench_tbe(B=8192, D=128, tables=26, rows=1_000_000, L=1, precision="fp32",
              id_pattern="random"):
    from torchrec_amd.ops.tbe import TableBatchedEmbeddingBags

    torch.manual_seed(0)
    specs = [(f"t{i}", rows, D) for i in range(tables)]
    tbe = TableBatchedEmbeddingBags(
        specs, device=torch.device("cuda"), fixed_bag_length=L,
        weights_precision=precision,
    )
    F = tables
    lengths = torch.full((F * B,), L, dtype=torch.int64)
    if id_pattern == "sequential":
        indices = (torch.arange(F * B * L) % rows).cuda()
    else:
        indices = torch.randint(0, rows, (F * B * L,)).cuda()
    offsets = torch.zeros(F * B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    offsets = offsets.cuda()

    fwd_us = _time_kernel(lambda: tbe(indices, offsets))
    out = tbe(indices, offsets)
    g = torch.ones_like(out)

    def step():
        o = tbe(indices, offsets)
        o.backward(g)

    full_us = _time_kernel(step)
    bytes_moved = F * B * L * D * 4 * 2 + B * F * D * 4  # read rows + write out
    elem = 4 if precision == "fp32" else 2
    bytes_moved = F * B * L * D * elem + B * F * D * 4
    print(json.dumps({
        "bench": "tbe", "B": B, "D": D, "tables": tables, "rows_per_table": rows,
        "precision": precision, "id_pattern": id_pattern,
        "fwd_us": round(fwd_us, 1), "fwd_bwd_opt_us": round(full_us, 1),
        "fwd_gb_s": round(bytes_moved / fwd_us / 1e3, 1),
    }))


def bench_interaction(B=8192, F=27, D=128):
    from torchrec_amd import ops

    ops.hip_ops()
    for variant, dtype in (("fp32-valu", torch.float32),
                           ("mfma-f32io", torch.float32),
                           ("mfma-bf16io", torch.bfloat16)):
        dense = torch.randn(B, D, device="cuda").to(dtype).requires_grad_(True)
        sparse = torch.randn(B, F - 1, D, device="cuda").to(dtype).requires_grad_(True)
        if variant == "fp32-valu":
            fn = ops._FusedInteraction.apply
        else:
            fn = ops._FusedInteractionMFMA.apply
        fwd_us = _time_kernel(lambda: fn(dense, sparse))
        out = fn(dense, sparse)
        g = torch.ones_like(out)

        def bwd():
            o = fn(dense, sparse)
            o.backward(g)

        both_us = _time_kernel(bwd)
        print(json.dumps({
            "bench": "interaction", "variant": variant, "B": B, "F": F, "D": D,
            "fwd_us": round(fwd_us, 1), "fwd_bwd_us": round(both_us, 1),
        }))


def bench_sort(N=213_000, segments=26):
    from torchrec_amd import ops
    ops.hip_ops()

    keys = torch.randint(0, 1 << 26, (N,), dtype=torch.int64).cuda()
    dev_us = _time_kernel(lambda: torch.ops.trec_amd.sort_pairs(keys, 26))
    B = N // segments
    lengths = torch.ones(segments * B, dtype=torch.int64)
    offsets = torch.zeros(segments * B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    offsets = offsets.cuda()
    # table-ordered disjoint segments for the block sort
    lin = torch.cat([
        torch.randint(0, 1 << 20, (B,), dtype=torch.int64) + (f << 20)
        for f in range(segments)
    ]).cuda()
    seg_us = _time_kernel(
        lambda: torch.ops.trec_amd.seg_sort_pairs(lin, offsets, B, segments, 26, B)
    )
    print(json.dumps({
        "bench": "radix_sort", "N": segments * B,
        "hipcub_us": round(dev_us, 1), "segmented_block_us": round(seg_us, 1),
    }))


def bench_col_sum(M=8192, N=1024):
    from torchrec_amd import ops
    ops.hip_ops()

    x = torch.randn(M, N, device="cuda", dtype=torch.bfloat16)
    ours = _time_kernel(lambda: torch.ops.trec_amd.col_sum(x))
    ref = _time_kernel(lambda: x.sum(0))
    print(json.dumps({
        "bench": "col_sum(bias grad)", "M": M, "N": N, "dtype": "bf16",
        "trec_us": round(ours, 1), "torch_us": round(ref, 1),
    }))


def bench_quant_tbe(B=8192, D=128, tables=26, rows=100_000, weight_dtype=None, repeats=1,
                    output_dtype=torch.float32, emit=True, mixed_kernel=False):
    """Quantized inference TBE forward at ``weight_dtype`` (default INT8) vs
    the fp32 training TBE forward, writing ``output_dtype``. Returns the
    ``repeats`` timings in us; ``emit=False`` leaves the printing to the caller.
    ``mixed_kernel`` sends an all-INT8 module through the mixed-format n-bit
    kernel (its 8-bit arm) instead of the INT8 kernel."""
    from torchrec_amd.modules.embedding_configs import DATA_TYPE_NUM_BITS, DataType
    from torchrec_amd.quant.embedding_modules import (
        QuantTableBatchedEmbeddingBags,
        nbit_row_stride,
    )
    from torchrec_amd.ops.tbe import TableBatchedEmbeddingBags

    weight_dtype = weight_dtype or DataType.INT8
    name = weight_dtype.name.lower()
    torch.manual_seed(0)
    specs = [(f"t{i}", rows, D) for i in range(tables)]
    q = QuantTableBatchedEmbeddingBags(
        specs, device=torch.device("cuda"), weight_dtypes=[weight_dtype] * tables,
        output_dtype=output_dtype,
    )
    for i in range(tables):
        q.load_float_table(i, torch.randn(rows, D, device="cuda"))
    if mixed_kernel:
        q._all_int8 = False
    F = tables
    indices = torch.randint(0, rows, (F * B,)).cuda()
    offsets = torch.arange(F * B + 1, dtype=torch.int64).cuda()
    # 5000 launches per timing: a window long enough not to measure the clock
    times = [
        _time_kernel(lambda: q(indices, offsets), iters=5000, warmup=20) for _ in range(repeats)
    ]
    if not emit:
        return times
    qt = sorted(times)[len(times) // 2]
    res = {
        "bench": "quant_tbe_fwd", "weight_dtype": weight_dtype.name, "B": B,
        "tables": tables, "D": D,
        "row_bytes": nbit_row_stride(D, DATA_TYPE_NUM_BITS[weight_dtype]),
        f"{name}_us": round(qt, 1), f"{name}_qps_m": round(B / qt, 1),
    }
    if repeats > 1:
        res[f"{name}_us_runs"] = [round(t, 1) for t in times]
        res[f"{name}_spread_us"] = round(max(times) - min(times), 1)
    if output_dtype != torch.float32:
        res["output_dtype"] = str(output_dtype).replace("torch.", "")
    if weight_dtype == DataType.INT8:
        f32 = TableBatchedEmbeddingBags(specs, device=torch.device("cuda"))
        res["fp32_us"] = round(_time_kernel(lambda: f32(indices, offsets)), 1)
    print(json.dumps(res))
    return times


def bench_quant_suite():
    """INT8 five times (median + max-min spread = the noise margin), then INT4
    and INT2, all in this process."""
    from torchrec_amd.modules.embedding_configs import DataType

    int8 = bench_quant_tbe(weight_dtype=DataType.INT8, repeats=5)
    med, spread = sorted(int8)[2], max(int8) - min(int8)
    for dt in (DataType.INT4, DataType.INT2):
        t = bench_quant_tbe(weight_dtype=dt, repeats=3)
        t_med = sorted(t)[1]
        print(json.dumps({
            "bench": "quant_tbe_fwd_vs_int8", "weight_dtype": dt.name,
            "us": round(t_med, 1), "int8_median_us": round(med, 1),
            "int8_spread_us": round(spread, 1),
            "within_noise_or_faster": bool(t_med <= med + spread),
        }))


def bench_quant_out_suite(B=8192, D=128, tables=26):
    """Per width: fp32 output five times (median + max-min spread = the noise
    margin of this run), then bf16 and fp16 output three times each, all in
    this process. One line per (width, output dtype)."""
    from torchrec_amd.modules.embedding_configs import DataType

    def line(dt, out, times, **extra):
        print(json.dumps({
            "bench": "quant_tbe_fwd_out", "weight_dtype": dt.name,
            "output_dtype": str(out).replace("torch.", ""), "B": B, "tables": tables, "D": D,
            "out_bytes": B * tables * D * torch.empty(0, dtype=out).element_size(),
            "us": round(sorted(times)[len(times) // 2], 1),
            "us_runs": [round(t, 1) for t in times], **extra,
        }))

    for dt in (DataType.INT8, DataType.INT4, DataType.INT2):
        f32 = bench_quant_tbe(B, D, tables, weight_dtype=dt, repeats=5, emit=False)
        med, spread = sorted(f32)[2], max(f32) - min(f32)
        line(dt, torch.float32, f32, spread_us=round(spread, 1))
        for out in (torch.bfloat16, torch.float16):
            t = bench_quant_tbe(
                B, D, tables, weight_dtype=dt, repeats=3, output_dtype=out, emit=False
            )
            line(dt, out, t, fp32_median_us=round(med, 1), fp32_spread_us=round(spread, 1),
                 within_noise_or_faster=bool(sorted(t)[1] <= med + spread))


def bench_quant_fp8_suite(B=8192, D=128, tables=26):
    """FP8 rows against INT8 rows, the same bytes per row and the same output
    write. Per output dtype: INT8 five times (median + max-min spread = the
    noise margin of this run), then FP8 three times, then the same INT8 rows
    three times through the mixed-format kernel FP8 runs in (its 8-bit arm),
    which tells the cost of that kernel from the cost of the FP8 arm. All in
    this process."""
    from torchrec_amd.modules.embedding_configs import DataType

    for out in (torch.float32, torch.bfloat16, torch.float16):
        int8 = bench_quant_tbe(
            B, D, tables, weight_dtype=DataType.INT8, repeats=5, output_dtype=out, emit=False
        )
        med, spread = sorted(int8)[2], max(int8) - min(int8)
        fp8 = bench_quant_tbe(
            B, D, tables, weight_dtype=DataType.FP8, repeats=3, output_dtype=out, emit=False
        )
        int8_mixed = bench_quant_tbe(
            B, D, tables, weight_dtype=DataType.INT8, repeats=3, output_dtype=out, emit=False,
            mixed_kernel=True,
        )
        print(json.dumps({
            "bench": "quant_tbe_fwd_fp8_vs_int8",
            "output_dtype": str(out).replace("torch.", ""), "B": B, "tables": tables, "D": D,
            "fp8_us": round(sorted(fp8)[1], 1), "fp8_us_runs": [round(t, 1) for t in fp8],
            "int8_median_us": round(med, 1), "int8_us_runs": [round(t, 1) for t in int8],
            "int8_spread_us": round(spread, 1),
            "int8_mixed_kernel_us_runs": [round(t, 1) for t in int8_mixed],
            "within_noise_or_faster": bool(sorted(fp8)[1] <= med + spread),
        }))


def bench_update_rows(N=4096, D=128, rows=100_000):
    """In-place update of N rows of one served table (``update_rows``, one
    kernel) per format, against the only alternative without it:
    ``load_float_table`` of the whole [rows, D] fp32 table (quantise into a
    second packed copy, then copy that over the served one). ``update_rows_us``
    is the eager call, host enqueue included; ``update_rows_graph_us`` is the
    device time of one update (50 of them replayed from a graph)."""
    from torchrec_amd.modules.embedding_configs import DataType
    from torchrec_amd.quant.embedding_modules import QuantTableBatchedEmbeddingBags

    torch.manual_seed(0)
    full = torch.randn(rows, D, device="cuda")
    ids = torch.randperm(rows, device="cuda")[:N].contiguous()
    new = torch.randn(N, D, device="cuda")
    for dt in (DataType.INT8, DataType.INT4, DataType.INT2, DataType.FP8):
        q = QuantTableBatchedEmbeddingBags(
            [("t0", rows, D)], device=torch.device("cuda"), weight_dtypes=[dt]
        )
        q.load_float_table(0, full)
        # three timings each, alternating; windows of a few tenths of a second
        upd, reload_us = [], []
        for _ in range(3):
            upd.append(
                _time_kernel(lambda: q.update_rows({0: (ids, new)}), iters=20000, warmup=20)
            )
            reload_us.append(
                _time_kernel(lambda: q.load_float_table(0, full), iters=1000, warmup=5)
            )
        in_graph = [_time_graph(lambda: q.update_rows({0: (ids, new)})) for _ in range(3)]
        applied = int(q.update_rows({0: (ids, new)})[0])
        print(json.dumps({
            "bench": "quant_tbe_update_rows", "weight_dtype": dt.name, "N": N, "D": D,
            "table_rows": rows, "applied": applied,
            "update_rows_us": round(sorted(upd)[1], 1),
            "update_rows_us_runs": [round(t, 1) for t in upd],
            "update_rows_graph_us": round(sorted(in_graph)[1], 2),
            "update_rows_graph_us_runs": [round(t, 2) for t in in_graph],
            "load_float_table_us": round(sorted(reload_us)[1], 1),
            "load_float_table_us_runs": [round(t, 1) for t in reload_us],
            "fp32_bytes_in": N * D * 4, "full_table_fp32_bytes": rows * D * 4,
        }))


def bench_checked_suite(B=8192, D=128, tables=26, rows=100_000):
    """What the bounds check / pruning remap in front of the quantized lookup
    costs, at the quant bench shape. Every time is the device time of one call
    (50 of them replayed from a graph). Per format (INT8, INT4):

    * ``unchecked``: the module built without checking, five times (median +
      max-min spread = the noise margin of this run);
    * ``checked``: ``bounds_check=True``, no remap; ``pruned``: every odd id
      pruned, the table at half its rows; three times each, alternating;
    * the remap kernel alone at the lookup's id count: all ids valid (with and
      without a remap) and all ids out of range, which is where serialised
      counting would show."""
    from torchrec_amd.modules.embedding_configs import DataType
    from torchrec_amd.quant.embedding_modules import QuantTableBatchedEmbeddingBags

    dev = torch.device("cuda")
    F = tables
    N = F * B
    torch.manual_seed(0)
    indices = torch.randint(0, rows, (N,)).cuda()
    offsets = torch.arange(N + 1, dtype=torch.int64).cuda()
    remap = torch.arange(rows, dtype=torch.int32) // 2
    remap[1::2] = -1
    for dt in (DataType.INT8, DataType.INT4):
        def build(n_rows, **kw):
            q = QuantTableBatchedEmbeddingBags(
                [(f"t{i}", n_rows, D) for i in range(tables)], device=dev,
                weight_dtypes=[dt] * tables, **kw,
            )
            for i in range(tables):
                q.load_float_table(i, torch.randn(n_rows, D, device="cuda"))
            return q

        plain = build(rows)
        checked = build(rows, bounds_check=True)
        pruned = build(rows // 2, index_remapping=[remap] * tables)
        base = [_time_graph(lambda: plain(indices, offsets)) for _ in range(5)]
        chk, prn = [], []
        for _ in range(3):
            chk.append(_time_graph(lambda: checked(indices, offsets)))
            prn.append(_time_graph(lambda: pruned(indices, offsets)))
        med = lambda xs: sorted(xs)[len(xs) // 2]
        runs = lambda xs: [round(t, 2) for t in xs]
        print(json.dumps({
            "bench": "quant_tbe_fwd_checked", "weight_dtype": dt.name, "B": B, "tables": tables,
            "D": D, "rows": rows, "ids": N,
            "unchecked_us": round(med(base), 2), "unchecked_us_runs": runs(base),
            "unchecked_spread_us": round(max(base) - min(base), 2),
            "checked_us": round(med(chk), 2), "checked_us_runs": runs(chk),
            "pruned_half_us": round(med(prn), 2), "pruned_half_us_runs": runs(prn),
        }))
        if dt is not DataType.INT8:
            continue
        all_bad = torch.full_like(indices, rows)
        alone = {}
        for key, q, ids in (
            ("valid", checked, indices), ("valid_remapped", pruned, indices),
            ("all_out_of_range", checked, all_bad),
        ):
            alone[key] = [
                _time_graph(lambda: q._remap_indices(ids, offsets, B, q._feat_table_t))
                for _ in range(3)
            ]
        print(json.dumps({
            "bench": "quant_tbe_remap_indices", "ids": N, "tables": tables,
            **{f"{k}_us": round(med(v), 2) for k, v in alone.items()},
            **{f"{k}_us_runs": runs(v) for k, v in alone.items()},
            "bytes_ids_in_out": N * 16, "bytes_remap_reads": N * 4,
            "out_of_range_counted": int(checked.out_of_range_counts().sum()),
        }))


if __name__ == "__main__":
    p = argparse.ArgumentParser()
    p.add_argument("--update-rows", action="store_true",
                   help="time the in-place row update against a whole-table reload, then exit")
    p.add_argument("--checked", action="store_true",
                   help="time the bounds-checked / pruned quantized lookup against the "
                        "unchecked one and the remap kernel alone, then exit")
    p.add_argument("--suite", default="all",
                   choices=["all", "tbe", "tbe_sweep", "interaction", "sort",
                            "col_sum", "quant", "quant_out", "quant_fp8"])
    a = p.parse_args()
    assert torch.cuda.is_available(), "run on a GPU box"
    if a.update_rows:
        bench_update_rows()
        sys.exit(0)
    if a.checked:
        bench_checked_suite()
        sys.exit(0)
    if a.suite in ("all", "tbe"):
        bench_tbe()
        bench_tbe(precision="bf16")
    if a.suite == "tbe_sweep":
        # backward access-pattern discriminator: random vs dense-coverage vs
        # sequential ids localize whether tbe_bwd_fused is random-DRAM-bound
        # or metadata-latency-bound
        bench_tbe(rows=1_000_000, id_pattern="random")
        bench_tbe(rows=131_072, id_pattern="random")
        bench_tbe(rows=1_000_000, id_pattern="sequential")
        bench_tbe(rows=1_000_000, id_pattern="random", B=65536)
    if a.suite in ("all", "interaction"):
        bench_interaction()
    if a.suite in ("all", "sort"):
        bench_sort()
    if a.suite in ("all", "col_sum"):
        bench_col_sum()
    if a.suite in ("all", "quant"):
        bench_quant_suite()
    if a.suite == "quant_out":
        bench_quant_out_suite()
    if a.suite == "quant_fp8":
        bench_quant_fp8_suite()
