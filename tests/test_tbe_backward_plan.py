"""The planned TBE backward: sort + bag metadata in one kernel, 4-way rank
merges, the chunk scan and the descriptors in one kernel, and no fill kernel
in the chain (the first kernel of the chain clears both lookback workspaces).

* ``tbe_backward_plan_sort`` against a CPU reference, exactly: keys and perm
  from a stable sort per segment, pos_row and pos_col from
  ``repeat_interleave`` over the bag lengths.
* the module through the planned op against the op-by-op chain
  (``TREC_BWD_PLAN=0``), bit for bit.
* graph replays and back-to-back eager calls: every call clears the
  workspaces again. A hang here means a scan started on a workspace that no
  kernel before it cleared; read ``tbe_backward_planned`` rather than re-run.
"""

import functools

import pytest
import torch

from torchrec_amd.ops.tbe import TableBatchedEmbeddingBags, _bits_needed

pytestmark = pytest.mark.gpu

F = 3
DIMS = [16, 32, 16]  # D-offsets from two different dims
D_OUT = [0, 16, 48]

# capacity -> what it exercises (2048-key base tiles, groups of four runs)
CAPACITIES = [
    2047,  # one tile, direct 64-bit output
    2048,
    2049,  # two tiles: a group of two
    4096,
    4097,  # three tiles, short last run
    8192,  # four tiles: the bench's shape for one segment
    8193,  # five tiles: two rounds, second group of one
    2048 * 17,  # rounds of 4, 4, 2
]
PATTERNS = ["equal", "descending", "rand10", "rand1m"]


def _pattern_indices(pattern, cap, gen):
    """[F * cap] indices, one id per bag, and the rows of each table."""
    if pattern == "equal":
        return torch.zeros(F * cap, dtype=torch.int64), 10
    if pattern == "descending":
        one = torch.arange(cap - 1, -1, -1, dtype=torch.int64)
        return one.repeat(F), cap
    rows = 10 if pattern == "rand10" else 1_000_000
    return torch.randint(0, rows, (F * cap,), generator=gen), rows


def _reference(indices, offsets, B, rows):
    """keys, perm, pos_row, pos_col on the CPU."""
    row_off = torch.tensor([f * rows for f in range(F)], dtype=torch.int64)
    lengths = offsets[1:] - offsets[:-1]
    bag = torch.repeat_interleave(torch.arange(F * B), lengths)
    f = bag // B
    pos_row = (bag - f * B).to(torch.int32)
    pos_col = torch.tensor(D_OUT, dtype=torch.int64)[f]
    linear = indices + row_off[f]
    keys = torch.empty_like(linear)
    perm = torch.empty(linear.numel(), dtype=torch.int32)
    for s in range(F):
        lo, hi = int(offsets[s * B]), int(offsets[(s + 1) * B])
        srt = torch.sort(linear[lo:hi], stable=True)
        keys[lo:hi] = srt.values
        perm[lo:hi] = (srt.indices + lo).to(torch.int32)
    return keys, perm, pos_row, pos_col, row_off


def _run_plan_sort(indices, offsets, B, rows, cap):
    dev = torch.device("cuda")
    keys, perm, pos_row, pos_col, row_off = _reference(indices, offsets, B, rows)
    got = torch.ops.trec_amd.tbe_backward_plan_sort(
        offsets.to(dev), indices.to(dev), torch.tensor(D_OUT, dtype=torch.int64, device=dev),
        row_off.to(dev), B, F, _bits_needed(F * rows), cap,
    )
    g_keys, g_perm, g_row, g_col, g_over = (t.cpu() for t in got)
    assert g_perm.dtype == torch.int32 and g_row.dtype == torch.int32
    assert g_keys.dtype == torch.int64 and g_col.dtype == torch.int64
    assert torch.equal(g_keys, keys)
    assert torch.equal(g_perm, perm)
    assert torch.equal(g_row, pos_row)
    assert torch.equal(g_col, pos_col)
    assert torch.equal(g_over, torch.zeros(F, dtype=torch.int32))


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("cap", CAPACITIES)
def test_sort_and_metadata_exact(cap, pattern):
    from torchrec_amd import ops

    ops.hip_ops()
    gen = torch.Generator().manual_seed(cap * 7 + len(pattern))
    indices, rows = _pattern_indices(pattern, cap, gen)
    offsets = torch.arange(F * cap + 1, dtype=torch.int64)  # one id per bag
    _run_plan_sort(indices, offsets, cap, rows, cap)


@pytest.mark.parametrize("rows", [10, 1_000_000])
def test_sort_and_metadata_variable_bags(rows):
    """Bag lengths in 0..L: segments shorter than the capacity, so the hinted
    bag is wrong and the bag search proper runs. Segment 1 is empty, and the
    bags on both sides of the segment boundaries are empty."""
    from torchrec_amd import ops

    ops.hip_ops()
    B, L = 1500, 3  # capacity 4500: three tiles
    gen = torch.Generator().manual_seed(31 + rows)
    lengths = torch.randint(0, L + 1, (F * B,), generator=gen)
    lengths[B : 2 * B] = 0  # an empty segment
    lengths[B - 1] = 0  # empty bags at the segment boundaries
    lengths[2 * B] = 0
    lengths[0] = L
    lengths[F * B - 1] = 0
    offsets = torch.zeros(F * B + 1, dtype=torch.int64)
    offsets[1:] = torch.cumsum(lengths, 0)
    indices = torch.randint(0, rows, (int(offsets[-1]),), generator=gen)
    _run_plan_sort(indices, offsets, B, rows, L * B)


# ---------------------------------------------------------------------------
# whole chain: planned op against the op-by-op chain
# ---------------------------------------------------------------------------


def _skewed(n, rows, gen):
    """ids with long and short duplicate runs."""
    u = torch.rand(n, generator=gen)
    return (u * u * u * rows).to(torch.int64).clamp_(max=rows - 1)


@functools.lru_cache(maxsize=None)
def _chain_case(name):
    """specs, B, indices (CPU) of a whole-chain case; one id per bag."""
    gen = torch.Generator().manual_seed(len(name) * 1000 + sum(map(ord, name)))
    if name == "n2047":
        return (("t", 500, 32),), 2047, _skewed(2047, 500, gen)
    if name == "n2049":
        return (("t", 500, 32),), 2049, _skewed(2049, 500, gen)
    if name == "n6145":
        # > 2048 runs: the chunk scan looks back over more than one run tile
        n = 2048 * 3 + 1
        ids = torch.randint(0, 100_000, (n,), generator=gen)
        ids[::3] = _skewed((n + 2) // 3, 40, gen)
        return (("t", 100_000, 32),), n, ids
    assert name == "hot3"
    # 3 rows under B = 2048: runs of about 683 occurrences, 22 chunks > 16
    B = 2048
    ids = torch.cat([
        torch.randint(0, 3, (B,), generator=gen),
        torch.randint(0, 1000, (B,), generator=gen),
    ])
    return (("hot", 3, 64), ("big", 1000, 32)), B, ids


def _run_module(name, optimizer, grad_dtype):
    specs, B, indices = _chain_case(name)
    dev = torch.device("cuda")
    tbe = TableBatchedEmbeddingBags(
        list(specs), optimizer=optimizer, learning_rate=0.05, device=dev,
        fixed_bag_length=1, output_dtype=grad_dtype,
    )
    g = torch.Generator().manual_seed(5)
    w0 = (torch.rand(tbe.weights.numel(), generator=g) - 0.5) * 0.2
    tbe.weights.data.copy_(w0)
    n_feat = len(specs)
    offsets = torch.arange(n_feat * B + 1, dtype=torch.int64, device=dev)
    grad = torch.randn(B, sum(s[2] for s in specs), generator=g)
    for _ in range(2):
        out = tbe(indices.to(dev), offsets)
        out.backward(grad.to(dev).to(out.dtype))
    torch.cuda.synchronize()
    got = {"weights": tbe.weights.detach().cpu(), "momentum": tbe.momentum.cpu()}
    if optimizer == "dense":
        got["grad_weights"] = tbe.weights.grad.cpu()
    return got


@pytest.mark.parametrize("grad_dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("optimizer", ["rowwise_adagrad", "dense"])
@pytest.mark.parametrize("name", ["n2047", "n2049", "n6145", "hot3"])
def test_whole_chain_unchanged(monkeypatch, name, optimizer, grad_dtype):
    monkeypatch.delenv("TREC_BWD_PLAN", raising=False)
    monkeypatch.delenv("TREC_SEG_SORT", raising=False)
    new = _run_module(name, optimizer, grad_dtype)
    monkeypatch.setenv("TREC_BWD_PLAN", "0")
    old = _run_module(name, optimizer, grad_dtype)
    assert sorted(new) == sorted(old)
    w0 = (torch.rand(new["weights"].numel(), generator=torch.Generator().manual_seed(5)) - 0.5) * 0.2
    moved = new["grad_weights"] if optimizer == "dense" else new["weights"] - w0
    assert bool((moved != 0).any()), "the backward did nothing"
    for key in new:
        assert torch.equal(new[key], old[key]), key


# ---------------------------------------------------------------------------
# every call and every replay clears the lookback workspaces again
# ---------------------------------------------------------------------------

REPLAY_SPECS = [("a", 7, 16), ("b", 3000, 32), ("c", 200, 16)]
REPLAY_B = 2049


def _replay_module():
    dev = torch.device("cuda")
    tbe = TableBatchedEmbeddingBags(
        REPLAY_SPECS, optimizer="rowwise_adagrad", learning_rate=0.05, device=dev,
        fixed_bag_length=1,
    )
    g = torch.Generator().manual_seed(11)
    w0 = (torch.rand(tbe.weights.numel(), generator=g) - 0.5) * 0.2
    tbe.weights.data.copy_(w0)
    return tbe


def _replay_batch(step):
    g = torch.Generator().manual_seed(400 + step)
    return torch.cat(
        [torch.randint(0, s[1], (REPLAY_B,), generator=g) for s in REPLAY_SPECS]
    )


def test_replays_and_repeated_calls_clear_workspaces(monkeypatch):
    monkeypatch.delenv("TREC_BWD_PLAN", raising=False)
    monkeypatch.delenv("TREC_SEG_SORT", raising=False)
    dev = torch.device("cuda")
    captured, eager = _replay_module(), _replay_module()
    offsets = torch.arange(F * REPLAY_B + 1, dtype=torch.int64, device=dev)
    grad = torch.randn(
        REPLAY_B, sum(s[2] for s in REPLAY_SPECS), generator=torch.Generator().manual_seed(3)
    ).to(dev)
    static_idx = _replay_batch(0).to(dev)

    def step(tbe, idx):
        tbe(idx, offsets).backward(grad)

    # warm-up on a side stream, mirrored on the eager twin (two eager calls
    # in a row on one stream)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            step(captured, static_idx)
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        step(eager, static_idx)
    torch.cuda.synchronize()
    assert torch.equal(captured.weights, eager.weights)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step(captured, static_idx)
    step(eager, static_idx)  # the capture pass does not run the kernels...
    graph.replay()  # ...so replay once with the same batch
    torch.cuda.synchronize()
    assert torch.equal(captured.weights, eager.weights)
    for i in range(1, 4):
        batch = _replay_batch(i).to(dev)
        static_idx.copy_(batch)
        graph.replay()
        step(eager, batch)
        torch.cuda.synchronize()
        assert torch.equal(captured.weights, eager.weights), f"replay {i}"
        assert torch.equal(captured.momentum, eager.momentum), f"replay {i}"
