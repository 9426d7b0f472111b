"""In-place row update of a served quantized table (``update_rows``, op
``quant_tbe_update_rows``): bytes, window, degenerate shapes, lookups, managed
tables, graph capture and the host-side errors.

The oracle is the contract itself: the first ``code_bytes + 4`` bytes of an
applied row are what the table's own whole-table quantiser (run on the device
the update runs on) writes for the new fp32 row, and no other byte of
``qweights`` changes. Every comparison is ``torch.equal`` on the whole buffer,
so a touched padding byte, neighbour row or other table fails it.

Shapes: D=20 INT8 has stride 32 with 8 padding bytes; D=8 INT4 has a 4-byte
code and stride 16; D=260 INT8 and D=520 INT4 have 65 code words, one more
than a wave, so the lane loops run twice; the all-INT8 CPU module has an odd
D=5 table (the INT8 stride rule takes any D)."""

import functools

import pytest
import torch

from torchrec_amd.distributed.model_tracker import UniqueRows
from torchrec_amd.modules.embedding_configs import DataType, EmbeddingBagConfig, PoolingType
from torchrec_amd.quant.embedding_modules import (
    EmbeddingBagCollection as QuantEBC,
    QuantTableBatchedEmbeddingBags,
    quantize_rowwise_fp8,
    quantize_rowwise_int8,
    quantize_rowwise_nbit,
)

INT8, INT4, INT2, FP8 = DataType.INT8, DataType.INT4, DataType.INT2, DataType.FP8

# kind -> (specs (name, rows, dim), formats, row windows of the Window case)
CASES = {
    "mixed": (
        [("t1", 9, 20), ("t2", 7, 8), ("t3", 5, 16), ("t4", 6, 4), ("t5", 5, 260), ("t6", 5, 520)],
        [INT8, INT4, INT2, FP8, INT8, INT4],
        [(2, 7), (3, 3), (0, 5), (4, 6), (0, 5), (0, 0)],
    ),
    # all INT8 (the module runs the INT8 lookup kernels); D=5 is odd: CPU only
    "int8_odd": (
        [("a", 9, 20), ("b", 6, 5), ("c", 5, 260)],
        [INT8, INT8, INT8],
        [(2, 7), (0, 0), (0, 5)],
    ),
    "int8": (
        [("a", 9, 20), ("b", 6, 8), ("c", 5, 260)],
        [INT8, INT8, INT8],
        [(2, 7), (0, 0), (0, 5)],
    ),
}

gpu = pytest.mark.gpu
KIND_DEV = [
    pytest.param("mixed", "cpu", id="mixed-cpu"),
    pytest.param("int8_odd", "cpu", id="int8_odd-cpu"),
    pytest.param("mixed", "cuda", id="mixed-gpu", marks=gpu),
    pytest.param("int8", "cuda", id="int8-gpu", marks=gpu),
]


@functools.lru_cache(maxsize=None)
def case_weights(kind):
    """The tables' fp32 weights, and per table the update: ids {last, 0, one
    middle row} in that (non-sorted) order with new rows [random, all-zero
    (scale 0), constant]. Computed once and never written to."""
    g = torch.Generator().manual_seed(1234)
    specs = CASES[kind][0]
    weights = [torch.randn(rows, dim, generator=g) for _, rows, dim in specs]
    updates = {}
    for t, (_, rows, dim) in enumerate(specs):
        ids = torch.tensor([rows - 1, 0, rows // 2])
        new = torch.randn(3, dim, generator=g) * 2.0
        new[1] = 0.0
        new[2] = 0.75
        updates[t] = (ids, new)
    return weights, updates


def make_tbe(kind, device, output_dtype=torch.float32, pooling=PoolingType.SUM, location="device"):
    specs, dtypes, _ = CASES[kind]
    tbe = QuantTableBatchedEmbeddingBags(
        specs,
        pooling=pooling,
        device=torch.device(device),
        weight_dtypes=dtypes,
        output_dtype=output_dtype,
        location=location,
    )
    for i, w in enumerate(case_weights(kind)[0]):
        tbe.load_float_table(i, w)
    return tbe


def on(device, updates):
    return {t: (ids.to(device), rows.to(device)) for t, (ids, rows) in updates.items()}


def quantize_like(dtype, w):
    if dtype is FP8:
        return quantize_rowwise_fp8(w)
    if dtype is INT8:
        return quantize_rowwise_int8(w)
    return quantize_rowwise_nbit(w, 4 if dtype is INT4 else 2)


def expected_qweights(tbe, updates, windows=None, quant_device=None):
    """The old buffer with ``[:code_bytes + 4]`` of every in-window row
    overwritten by the whole-table quantiser's bytes, and per-table counts."""
    exp = tbe.qweights.clone()
    quant_device = quant_device or exp.device
    starts = tbe._table_byte_offsets.tolist()
    counts = [0] * len(tbe._specs)
    for t, (ids, rows) in updates.items():
        _, R, D = tbe._specs[t]
        dtype = tbe._weight_dtypes[t]
        lo, hi = windows[t] if windows else (0, R)
        ids = ids.cpu()
        keep = (ids >= lo) & (ids < hi)
        counts[t] = int(keep.sum())
        if counts[t] == 0:
            continue
        packed = quantize_like(dtype, rows.cpu()[keep].float().to(quant_device))
        stride = packed.shape[1]
        nb = D * (8 if dtype in (INT8, FP8) else (4 if dtype is INT4 else 2)) // 8 + 4
        view = exp[starts[t] : starts[t] + R * stride].view(R, stride)
        view[(ids[keep] - lo).to(exp.device), :nb] = packed[:, :nb].to(exp.device)
    return exp, torch.tensor(counts)


def sync(device):
    if device == "cuda":
        torch.cuda.synchronize()


@pytest.mark.parametrize("kind,device", KIND_DEV)
def test_bytes(kind, device):
    tbe = make_tbe(kind, device)
    updates = case_weights(kind)[1]
    exp, counts = expected_qweights(tbe, updates)
    assert not torch.equal(exp, tbe.qweights)
    applied = tbe.update_rows(on(device, updates))
    sync(device)
    assert torch.equal(tbe.qweights, exp)
    assert applied.dtype == torch.int64 and torch.equal(applied.cpu(), counts)
    assert applied.device.type == device


@pytest.mark.parametrize("kind,device", KIND_DEV)
def test_bytes_from_half_rows(kind, device):
    """Rows of another float dtype are converted to fp32 first."""
    tbe = make_tbe(kind, device)
    updates = {t: (ids, rows.bfloat16()) for t, (ids, rows) in case_weights(kind)[1].items()}
    exp, _ = expected_qweights(tbe, updates)
    tbe.update_rows(on(device, updates))
    sync(device)
    assert torch.equal(tbe.qweights, exp)


@pytest.mark.parametrize("kind,device", KIND_DEV)
def test_window(kind, device):
    """Ids outside the table's window (ids >= rows and a negative id among
    them, and everything under an empty window) change nothing and are not
    counted; the others land in local row id - lo."""
    tbe = make_tbe(kind, device)
    specs, _, windows = CASES[kind]
    g = torch.Generator().manual_seed(7)
    updates = {}
    for t, (ids, rows) in case_weights(kind)[1].items():
        R, D = specs[t][1], specs[t][2]
        extra = torch.tensor([R, R + 91, -1])
        updates[t] = (torch.cat([ids, extra]), torch.cat([rows, torch.randn(3, D, generator=g)]))
    before = tbe.qweights.clone()
    exp, counts = expected_qweights(tbe, updates, windows)
    applied = tbe.update_rows(on(device, updates), row_windows=windows)
    sync(device)
    assert torch.equal(tbe.qweights, exp)
    assert torch.equal(applied.cpu(), counts)
    inside = [sum(lo <= int(i) < hi for i in updates[t][0]) for t, (lo, hi) in enumerate(windows)]
    assert applied.tolist() == inside and 0 in inside and max(inside) > 0
    # an empty window keeps the table, its local row 0 included, as it was
    starts = tbe._table_byte_offsets.tolist() + [tbe.qweights.numel()]
    for t, (lo, hi) in enumerate(windows):
        if lo == hi:
            assert torch.equal(tbe.qweights[starts[t] : starts[t + 1]], before[starts[t] : starts[t + 1]])


@pytest.mark.parametrize("kind,device", KIND_DEV)
def test_degenerate(kind, device):
    tbe = make_tbe(kind, device)
    specs = CASES[kind][0]
    T = len(specs)
    before = tbe.qweights.clone()
    # nothing to do
    applied = tbe.update_rows({})
    sync(device)
    assert torch.equal(tbe.qweights, before) and applied.tolist() == [0] * T
    # a table with zero ids among others with some
    updates = dict(case_weights(kind)[1])
    updates[1] = (torch.empty(0, dtype=torch.int64), torch.empty(0, specs[1][2]))
    exp, counts = expected_qweights(tbe, updates)
    applied = tbe.update_rows(on(device, updates))
    sync(device)
    assert torch.equal(tbe.qweights, exp) and torch.equal(applied.cpu(), counts)
    assert counts[1] == 0 and counts[0] == 3
    # every row of the last table, in a shuffled order
    t = T - 1
    R, D = specs[t][1], specs[t][2]
    g = torch.Generator().manual_seed(3)
    full = {t: (torch.randperm(R, generator=g), torch.randn(R, D, generator=g))}
    exp, counts = expected_qweights(tbe, full)
    applied = tbe.update_rows(on(device, full))
    sync(device)
    assert torch.equal(tbe.qweights, exp) and applied.tolist() == [0] * t + [R]


def lookup_inputs(kind):
    """B=3 bags per feature; bag 0 of every feature holds the updated ids."""
    specs = CASES[kind][0]
    g = torch.Generator().manual_seed(11)
    idx, lengths = [], []
    for _, rows, _ in specs:
        bags = [
            torch.tensor([0, rows - 1, rows // 2]),
            torch.randint(0, rows, (2,), generator=g),
            torch.empty(0, dtype=torch.int64),
        ]
        idx += bags
        lengths += [b.numel() for b in bags]
    indices = torch.cat(idx)
    offsets = torch.cat([torch.zeros(1, dtype=torch.int64), torch.tensor(lengths).cumsum(0)])
    psw = torch.rand(indices.numel(), generator=g) + 0.5
    return indices, offsets, psw


def sequence_lookup(tbe, t, idx, device):
    """Rows ``idx`` of table ``t`` at the module's output dtype."""
    if device == "cpu":
        return tbe.to_output_dtype(tbe.dequantized_table(t)[idx])
    T = len(tbe._specs)
    fvo = torch.tensor([0] * (t + 1) + [idx.numel()] * (T - t), device=device)
    return tbe.forward_sequence(idx.to(device), fvo, tbe._specs[t][2])


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("kind,device", KIND_DEV)
def test_lookup(kind, device, out_dtype):
    """Pooled (SUM / MEAN, with and without per-sample weights) and sequence
    lookups after the update are bit-identical to those of a module whose
    buffer is the expected one."""
    updates = case_weights(kind)[1]
    indices, offsets, psw = (x.to(device) for x in lookup_inputs(kind))
    exp = None
    for pooling in (PoolingType.SUM, PoolingType.MEAN):
        upd = make_tbe(kind, device, out_dtype, pooling)
        ref = make_tbe(kind, device, out_dtype, pooling)
        if exp is None:
            exp, _ = expected_qweights(ref, updates)
        stale = upd(indices, offsets).clone()
        upd.update_rows(on(device, updates))
        ref.qweights.copy_(exp)
        for w in (None, psw):
            got, want = upd(indices, offsets, w), ref(indices, offsets, w)
            sync(device)
            assert got.dtype == out_dtype and torch.equal(got, want)
        assert not torch.equal(upd(indices, offsets), stale)
    for t, (ids, _) in updates.items():
        idx = torch.cat([ids, ids.flip(0)])
        got = sequence_lookup(upd, t, idx, device)
        want = sequence_lookup(ref, t, idx, device)
        sync(device)
        assert got.dtype == out_dtype and torch.equal(got, want)


@gpu
@pytest.mark.parametrize("dtype,D", [(INT8, 20), (FP8, 12)], ids=["int8", "fp8"])
def test_managed(dtype, D):
    """A pinned-host (``location="managed"``) table updates the same way: the
    kernel writes it through its device pointer."""
    g = torch.Generator().manual_seed(5)
    tbe = QuantTableBatchedEmbeddingBags(
        [("m", 9, D)], device=torch.device("cuda"), weight_dtypes=[dtype], location="managed"
    )
    tbe.load_float_table(0, torch.randn(9, D, generator=g))
    assert not tbe.qweights.is_cuda and tbe.qweights.is_pinned()
    new = torch.randn(3, D, generator=g)
    new[1] = 0.0
    updates = {0: (torch.tensor([8, 0, 4]), new)}
    before = tbe.qweights.clone()
    exp, counts = expected_qweights(tbe, updates, quant_device=torch.device("cuda"))
    applied = tbe.update_rows(on("cuda", updates))
    torch.cuda.synchronize()
    assert torch.equal(tbe.qweights, exp) and not torch.equal(exp, before)
    assert torch.equal(applied.cpu(), counts) and counts.tolist() == [3]


@gpu
def test_graph_capture():
    """One update_rows plus one lookup captured in a graph (one stream, a
    single chain of kernels: no parallel branches), replayed twice with new
    values copied into the static input, matches eager each time."""
    kind = "mixed"
    base = case_weights(kind)[1]
    indices, offsets, _ = (x.cuda() for x in lookup_inputs(kind))
    captured, eager = make_tbe(kind, "cuda"), make_tbe(kind, "cuda")
    # the GPU INT8 quantiser leaves a row's padding bytes unwritten, so two
    # modules loaded from the same weights may differ there: start from one buffer
    eager.qweights.copy_(captured.qweights)
    static = on("cuda", base)
    captured.update_rows(static)  # warm-up: uploads the shape-only metadata
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        applied = captured.update_rows(static)
        out = captured(indices, offsets)
    g = torch.Generator().manual_seed(21)
    for _ in range(2):
        fresh = {t: (ids, torch.randn(rows.shape, generator=g)) for t, (ids, rows) in base.items()}
        for t, (_, rows) in fresh.items():
            static[t][1].copy_(rows)
        out.zero_()
        graph.replay()
        want_applied = eager.update_rows(on("cuda", fresh))
        want = eager(indices, offsets)
        torch.cuda.synchronize()
        differ = (captured.qweights != eager.qweights).nonzero().flatten().tolist()
        assert not differ, f"{len(differ)} bytes differ, the first at {differ[:8]}"
        assert torch.equal(out, want) and float(out.abs().max()) > 0
        assert torch.equal(applied, want_applied) and applied.tolist() == [3] * len(base)


def small_qebc(device):
    tables = [
        EmbeddingBagConfig(num_embeddings=6, embedding_dim=8, name="u0", feature_names=["f0"],
                           data_type=INT4),
        EmbeddingBagConfig(num_embeddings=5, embedding_dim=4, name="u1", feature_names=["f1"],
                           data_type=FP8),
    ]
    return QuantEBC(tables, device=torch.device(device))


DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=gpu)]


@pytest.mark.parametrize("device", DEVICES)
def test_errors(device):
    q = small_qebc(device)
    before = q._tbe.qweights.clone()
    ids = torch.tensor([1, 2], device=device)
    with pytest.raises(ValueError, match="rows"):
        q._tbe.update_rows({0: (ids, torch.zeros(2, 4, device=device))})  # dim is 8
    with pytest.raises(ValueError, match="rows"):
        q.update_embeddings({"u0": (ids, torch.zeros(3, 8, device=device))})
    with pytest.raises(IndexError):
        q._tbe.update_rows({2: (ids, torch.zeros(2, 8, device=device))})
    with pytest.raises(KeyError, match="nope"):
        q.update_embeddings({"nope": (ids, torch.zeros(2, 8, device=device))})
    with pytest.raises(ValueError, match="UpdateMode"):
        q.update_embeddings({"u0": UniqueRows(ids=ids)})
    with pytest.raises(ValueError, match="row_windows"):
        q._tbe.update_rows({}, row_windows=[(0, 6)])
    assert torch.equal(q._tbe.qweights, before)


@pytest.mark.parametrize("device", DEVICES)
def test_update_embeddings_by_name(device):
    """The EBC maps names to tables and takes UniqueRows or (ids, rows)."""
    q = small_qebc(device)
    g = torch.Generator().manual_seed(9)
    delta = {
        "u1": UniqueRows(ids=torch.tensor([4, 0]), rows=torch.randn(2, 4, generator=g)),
        "u0": (torch.tensor([5, 6]), torch.randn(2, 8, generator=g)),  # 6 is out of range
    }
    exp, _ = expected_qweights(q._tbe, {0: delta["u0"], 1: (delta["u1"].ids, delta["u1"].rows)})
    moved = {
        "u1": UniqueRows(ids=delta["u1"].ids.to(device), rows=delta["u1"].rows.to(device)),
        "u0": tuple(x.to(device) for x in delta["u0"]),
    }
    applied = q.update_embeddings(moved)
    sync(device)
    assert torch.equal(q._tbe.qweights, exp)
    assert {n: int(c) for n, c in applied.items()} == {"u0": 1, "u1": 2}
