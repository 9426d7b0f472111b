"""The TBE backward's floating-point summation order, pinned bit for bit.

``tests/test_tbe_backward_chain.py`` uses integer gradients, whose fp32 sums
are exact in every order; it cannot see a reassociated sum. Here gradients
are real-valued (``torch.randn``) and the dense-gradient mode of the chain
must equal, with ``torch.equal``, a CPU emulation of the order the kernels
promise:

- occurrences of a row are accumulated in sorted-position order (the sort is
  stable, so equal keys keep their original order);
- each step is ``acc = fma(s, g, acc)`` in fp32 from 0. Scales are ``None`` or
  drawn from {0.5, 1, 2}, so ``s * g`` is exact and the fma equals an IEEE
  fp32 add of the product;
- a run longer than 32 occurrences is accumulated in 32-occurrence chunks,
  and the chunk partials are added in ascending chunk order from 0.

The oracle was validated against the commit before the gather and fold loops
were pipelined (see profiles/PROFILE_r04.md): it is a statement about that
order, not about the code under test.

Boundary -> cases that cross it (a flight is the 4, 2 or 1 rows the gather and
the fold keep in flight; the lengths also cover flights of 8):

- run lengths round a flight and round the chunk size: TestRunLengths
- chunk counts round the fold's flight, one run of 100 chunks: TestChunkCounts
- the chunk descriptors (chunk -> run): TestChunkLookup (long run first /
  last / alone, long runs separated by 70 short ones, num_runs of 1, 31, 32,
  33, 1025, and a run of more chunks than one thread writes itself)
- the first-occurrence offset in the run descriptor: TestFirstOccurrence
- LPS/CHUNKS dispatch on max_D: TestDispatch
- grid-strided slots: TestGridCap
- optimizer paths, split into an Adagrad/SGD and an Adam kernel: TestOptimizerGolden
  against states recorded from the parent commit (tests/golden/tbe_backward_order)
"""

import functools
import os

import numpy as np
import pytest
import torch

from torchrec_amd import ops
from torchrec_amd.ops.tbe import (
    OPT_DENSE,
    EmbeddingLocation,
    TableBatchedEmbeddingBags,
    _bits_needed,
)

pytestmark = pytest.mark.gpu

CHUNK = 32  # kChunkSize
SCALES = torch.tensor([0.5, 1.0, 2.0])
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tbe_backward_order", "states.npz")


class Layout:
    def __init__(self, specs):
        self.rows = [s[1] for s in specs]
        self.dims = [s[2] for s in specs]
        self.row_off, self.elem_off, self.d_out = [0], [0], [0]
        for r, d in zip(self.rows, self.dims):
            self.row_off.append(self.row_off[-1] + r)
            self.elem_off.append(self.elem_off[-1] + r * d)
            self.d_out.append(self.d_out[-1] + d)
        self.total_rows, self.total_elems = self.row_off[-1], self.elem_off[-1]
        self.max_D = max(self.dims)


# ---------------------------------------------------------------------------
# the order oracle (CPU, fp32 tensor adds)
# ---------------------------------------------------------------------------


def order_oracle(lay, linear, pos_row, pos_col, grad, scale):
    order = torch.sort(linear, stable=True).indices
    lin_s = linear[order]
    uniq, counts = torch.unique_consecutive(lin_s, return_counts=True)
    starts = torch.cumsum(counts, 0) - counts
    gflat = grad.float().reshape(-1)  # bf16 -> fp32 is exact
    stride = grad.shape[1]
    out = torch.zeros(lay.total_elems, dtype=torch.float32)
    for t, D in enumerate(lay.dims):
        sel = (uniq >= lay.row_off[t]) & (uniq < lay.row_off[t + 1])
        if not bool(sel.any()):
            continue
        r_lin, r_start, r_len = uniq[sel], starts[sel], counts[sel]
        # sub-runs: a short run is one, a long run one per chunk
        n_sub = torch.where(r_len > CHUNK, (r_len + CHUNK - 1) // CHUNK, torch.ones_like(r_len))
        run_of = torch.repeat_interleave(torch.arange(r_len.numel()), n_sub)
        first_sub = torch.cumsum(n_sub, 0) - n_sub
        idx_in_run = torch.arange(run_of.numel()) - first_sub[run_of]
        s_start = r_start[run_of] + idx_in_run * CHUNK
        s_len = torch.minimum(r_len[run_of] - idx_in_run * CHUNK, torch.tensor(CHUNK))
        s_len = torch.where(r_len[run_of] > CHUNK, s_len, r_len[run_of])
        part = torch.zeros(run_of.numel(), D, dtype=torch.float32)
        for j in range(int(s_len.max())):
            m = s_len > j
            p = order[s_start[m] + j]
            src = pos_row[p].long() * stride + pos_col[p]
            rows = gflat[src.unsqueeze(1) + torch.arange(D)]
            if scale is not None:
                rows = rows * scale[p].unsqueeze(1)  # exact: scale is 0.5, 1 or 2
            part[m] = part[m] + rows
        acc = torch.zeros(r_len.numel(), D, dtype=torch.float32)
        long = r_len > CHUNK
        acc[~long] = part[first_sub[~long]]
        for j in range(int(n_sub[long].max()) if bool(long.any()) else 0):
            m = long & (n_sub > j)
            acc[m] = acc[m] + part[first_sub[m] + j]
        view = out[lay.elem_off[t] : lay.elem_off[t + 1]].view(lay.rows[t], D)
        view[r_lin - lay.row_off[t]] = acc
    return out


def run_chain(specs, linear, pos_row, pos_col, grad, scale):
    """sort_pairs -> tbe_backward_prep -> tbe_backward_fused (dense mode), the
    way ``TableBatchedEmbeddingBags._backward_pooled`` calls them."""
    ops.hip_ops()
    lay = Layout(specs)
    dev = torch.device("cuda")
    empty_f = torch.empty(0, dtype=torch.float32, device=dev)
    empty_i = torch.empty(0, dtype=torch.int32, device=dev)
    weights = torch.zeros(lay.total_elems, dtype=torch.float32, device=dev)
    grad_weights = torch.zeros_like(weights)
    sorted_lin, perm = torch.ops.trec_amd.sort_pairs(linear.to(dev), _bits_needed(lay.total_rows))
    seg_offsets, num_runs = torch.ops.trec_amd.tbe_backward_prep(sorted_lin)
    torch.ops.trec_amd.tbe_backward_fused(
        weights, empty_f, grad.to(dev), sorted_lin, perm, seg_offsets, num_runs,
        pos_row.to(dev), pos_col.to(dev), scale.to(dev) if scale is not None else empty_f,
        torch.tensor(lay.row_off, dtype=torch.int64, device=dev),
        torch.tensor(lay.elem_off[:-1], dtype=torch.int64, device=dev),
        torch.tensor(lay.dims, dtype=torch.int32, device=dev),
        lay.max_D, 0.0, 1e-8, OPT_DENSE, grad_weights, empty_f, empty_i, empty_f, empty_f,
        0.9, 0.999, empty_f, torch.empty(0, dtype=torch.int64, device=dev), False,
    )
    torch.cuda.synchronize()
    assert not bool(weights.any())
    return grad_weights.cpu()


def make_positions(specs, runs, seed, with_scale, dtype, grad_rows=48, layout="pooled"):
    """``runs``: list of (table, local row, length). Positions are shuffled.
    pooled: each reads a random row of a [grad_rows, total_D] gradient at its
    table's column offset. packed: the VBE layout, one gradient row, position
    k reads D values at its own multiple of D (one table only)."""
    lay = Layout(specs)
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([r[0] for r in runs])
    lin = torch.tensor([lay.row_off[r[0]] + r[1] for r in runs])
    lens = torch.tensor([r[2] for r in runs])
    n = int(lens.sum())
    order = torch.randperm(n, generator=g)
    linear = torch.repeat_interleave(lin, lens)[order]
    if layout == "packed":
        assert len(specs) == 1
        D = lay.dims[0]
        pos_row = torch.zeros(n, dtype=torch.int32)
        pos_col = torch.randperm(n, generator=g) * D
        grad = torch.randn(1, n * D, generator=g).to(dtype)
    else:
        pos_col = torch.repeat_interleave(torch.tensor(lay.d_out)[t], lens)[order]
        pos_row = torch.randint(0, grad_rows, (n,), generator=g, dtype=torch.int32)
        grad = torch.randn(grad_rows, lay.d_out[-1], generator=g).to(dtype)
    scale = SCALES[torch.randint(0, 3, (n,), generator=g)] if with_scale else None
    return linear, pos_row, pos_col, grad, scale


def check(specs, runs, seed, with_scale=True, dtype=torch.float32, layout="pooled"):
    args = make_positions(specs, runs, seed, with_scale, dtype, layout=layout)
    assert args[0].numel() < 8000
    want = order_oracle(Layout(specs), *args)
    got = run_chain(specs, *args)
    assert torch.equal(got, want), (
        f"{int((got != want).sum())} elements differ, max abs {float((got - want).abs().max())}"
    )
    return args, got


DTYPES = [torch.float32, torch.bfloat16]
DT_IDS = ["fp32", "bf16"]


def test_oracle_is_order_sensitive():
    """The oracle must tell orders apart on these inputs: a plain fp32 sum in
    another association differs from it (else the file pins nothing)."""
    specs = [("t", 8, 64)]
    runs = [(0, 0, 65), (0, 3, 31), (0, 5, 7)]
    linear, pos_row, pos_col, grad, scale = make_positions(specs, runs, 1, True, torch.float32)
    want = order_oracle(Layout(specs), linear, pos_row, pos_col, grad, scale)
    ref = torch.zeros(8, 64, dtype=torch.float64)
    rows = grad[pos_row.long()].double() * scale.double().unsqueeze(1)
    ref.index_add_(0, linear, rows)
    assert not torch.equal(want.double(), ref.reshape(-1))
    torch.testing.assert_close(want.double(), ref.reshape(-1), atol=1e-4, rtol=1e-4)


# ---------------------------------------------------------------------------
# run lengths and chunk counts
# ---------------------------------------------------------------------------

RUN_LENGTHS = [1, 2, 3, 4, 5, 7, 8, 9, 17, 31, 32, 33, 63, 64, 65]
CHUNK_COUNTS = [2, 3, 4, 5, 7, 8, 9, 11, 19]


class TestRunLengths:
    @pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
    @pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "scaled"])
    def test_lengths_round_flight_and_chunk(self, dtype, with_scale):
        specs = [("t", 40, 128)]
        runs = [(0, 2 * i + 1, ln) for i, ln in enumerate(RUN_LENGTHS)]
        check(specs, runs, 3, with_scale, dtype)

    def test_lps16_two_offset_rounds(self):
        """max_D = 64: 16 lanes a slot, so a 32-occurrence chunk takes two
        rounds of the coalesced offset load."""
        specs = [("t", 40, 64)]
        runs = [(0, 2 * i, ln) for i, ln in enumerate(RUN_LENGTHS)]
        check(specs, runs, 4)


class TestChunkCounts:
    @pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
    def test_counts_round_flight(self, dtype):
        specs = [("t", 24, 128)]
        # full last chunk on even rows, ragged on odd ones
        runs = [(0, i, c * CHUNK - (5 if i % 2 else 0)) for i, c in enumerate(CHUNK_COUNTS)]
        check(specs, runs, 5, True, dtype)

    def test_hundred_chunks(self):
        specs = [("t", 3, 32)]
        check(specs, [(0, 1, 100 * CHUNK - 3), (0, 2, 40)], 6)


# ---------------------------------------------------------------------------
# chunk -> run
# ---------------------------------------------------------------------------


class TestChunkLookup:
    def test_long_run_first(self):
        specs = [("t", 50, 32)]
        check(specs, [(0, 0, 70)] + [(0, i, 1 + i % 3) for i in range(1, 50)], 7)

    def test_long_run_last(self):
        specs = [("t", 50, 32)]
        check(specs, [(0, i, 1 + i % 3) for i in range(49)] + [(0, 49, 70)], 8)

    def test_single_run(self):
        check([("t", 5, 32)], [(0, 2, 200)], 9)

    def test_flat_stretch_between_long_runs(self):
        """Long runs separated by 70 short ones: a stretch of equal
        chunk_offsets wider than 64 entries."""
        specs = [("t", 300, 32)]
        runs, row = [], 0
        for block in range(3):
            runs.append((0, row, 40 + 33 * block))
            row += 1
            for _ in range(70):
                runs.append((0, row, 1 + row % 2))
                row += 1
        runs.append((0, row, 97))
        check(specs, runs, 10)

    @pytest.mark.parametrize("num_runs", [1, 31, 32, 33, 1025])
    def test_num_runs(self, num_runs):
        specs = [("t", 1100, 32)]
        # every 16th run is long, and so are the first and the last
        runs = [
            (0, i, 33 + i % 40 if (i % 16 == 0 or i == num_runs - 1) else 1 + i % 3)
            for i in range(num_runs)
        ]
        check(specs, runs, 11)

    def test_run_wider_than_one_writer(self):
        """A run of more than 16 chunks has its chunk descriptors written by
        the whole wave; two of them in one wave, among shorter long runs."""
        specs = [("t", 12, 32)]
        runs = [(0, 0, 40), (0, 2, 17 * CHUNK + 1), (0, 3, 16 * CHUNK), (0, 5, 3),
                (0, 7, 70 * CHUNK - 9), (0, 9, 33)]
        check(specs, runs, 12)


# ---------------------------------------------------------------------------
# first occurrence in the descriptor
# ---------------------------------------------------------------------------


class TestFirstOccurrence:
    @pytest.mark.parametrize("with_scale", [False, True], ids=["plain", "scaled"])
    @pytest.mark.parametrize("layout", ["pooled", "packed"])
    def test_single_occurrence_at_both_ends(self, layout, with_scale):
        """Length-1 runs at sorted positions 0 and n - 1 (lowest and highest
        row), more of them and longer runs in between."""
        specs = [("t", 64, 32)]
        runs = [(0, 0, 1), (0, 63, 1)] + [(0, i, [1, 2, 5, 40][i % 4]) for i in range(1, 63, 2)]
        (linear, *_), got = check(specs, runs, 13, with_scale, layout=layout)
        assert int((linear == 0).sum()) == 1 and int((linear == 63).sum()) == 1
        rows = got.view(64, 32)
        assert bool(rows[0].any()) and bool(rows[63].any()) and not bool(rows[2].any())

    def test_packed_bf16(self):
        specs = [("t", 30, 64)]
        runs = [(0, i, [1, 1, 3, 33, 9][i % 5]) for i in range(30)]
        check(specs, runs, 14, True, torch.bfloat16, layout="packed")


# ---------------------------------------------------------------------------
# dispatch and grid cap
# ---------------------------------------------------------------------------

DISPATCH_LENGTHS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 300]


def dispatch_runs(specs):
    runs = []
    for t, s in enumerate(specs):
        lens = DISPATCH_LENGTHS if t % 2 == 0 else DISPATCH_LENGTHS[::-1]
        step = s[1] // len(lens)
        assert step >= 1
        runs += [(t, k * step, ln) for k, ln in enumerate(lens)]
    return runs


class TestDispatch:
    @pytest.mark.parametrize(
        "dims",
        [[8, 64], [8, 64, 128], [192, 64], [320, 64], [1280, 8]],
        ids=["lps16", "lps32", "lps64x1", "lps64x2", "lps64x8"],
    )
    def test_dispatch_on_max_d(self, dims):
        """A narrow table shares the launch with the wide one: lanes past the
        row end take no part, and the scratch stride (max_D) differs from D."""
        specs = [(f"t{i}", 23 + 10 * i, d) for i, d in enumerate(dims)]
        check(specs, dispatch_runs(specs), 15)


@functools.lru_cache(maxsize=None)
def strided_case():
    specs = (("a", 400, 32), ("b", 300, 64))
    g = torch.Generator().manual_seed(16)
    runs = []
    for t, rows in ((0, 400), (1, 300)):
        lens = torch.randint(1, 4, (rows,), generator=g)
        lens[torch.arange(rows) % 9 == 4] = 60
        lens[rows // 2] = 20 * CHUNK + 7
        runs += [(t, i, int(ln)) for i, ln in enumerate(lens)]
    args = make_positions(specs, runs, 17, True, torch.float32)
    return specs, args, order_oracle(Layout(specs), *args)


class TestGridCap:
    def test_grid_stride_equals_uncapped(self, monkeypatch):
        """One block of the fused kernel strides over every run; bitwise the
        uncapped result and the oracle."""
        specs, args, want = strided_case()
        monkeypatch.delenv("TREC_BWD_GRID_CAP", raising=False)
        full = run_chain(specs, *args)
        monkeypatch.setenv("TREC_BWD_GRID_CAP", "1")
        capped = run_chain(specs, *args)
        assert torch.equal(full, want)
        assert torch.equal(capped, full)


# ---------------------------------------------------------------------------
# optimizer paths against the parent commit's states
# ---------------------------------------------------------------------------

GOLD_SPECS = [("hot", 3, 64), ("mid", 24, 128), ("big", 160, 32)]
GOLD_B = 64
LR, EPS, BETA1, BETA2 = 0.05, 1.0e-8, 0.9, 0.999
# name -> (optimizer, weights_precision, location)
GOLD_CONFIGS = {
    "sgd": ("sgd", "fp32", EmbeddingLocation.DEVICE),
    "rowwise_adagrad": ("rowwise_adagrad", "fp32", EmbeddingLocation.DEVICE),
    "adam": ("adam", "fp32", EmbeddingLocation.DEVICE),
    "partial_rowwise_adam": ("partial_rowwise_adam", "fp32", EmbeddingLocation.DEVICE),
    "bf16_stochastic": ("rowwise_adagrad", "bf16", EmbeddingLocation.DEVICE),
    "cached": ("rowwise_adagrad", "fp32", EmbeddingLocation.MANAGED_CACHING),
}


def gold_batch(seed):
    g = torch.Generator().manual_seed(seed)
    F = len(GOLD_SPECS)
    lengths = torch.randint(0, 7, (F * GOLD_B,), generator=g)
    offsets = torch.zeros(F * GOLD_B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    indices = torch.cat(
        [
            torch.randint(
                0, GOLD_SPECS[f][1], (int(lengths[f * GOLD_B : (f + 1) * GOLD_B].sum()),),
                generator=g,
            )
            for f in range(F)
        ]
    )
    grad = torch.randn(GOLD_B, sum(s[2] for s in GOLD_SPECS), generator=g)
    return indices, offsets, grad


def gold_states(name, grad_dtype):
    """Two steps from fixed inputs; every tensor the update writes, as raw
    bits (int32 / int16 views) keyed ``<config>/<grad dtype>/<tensor>``."""
    optim, wprec, location = GOLD_CONFIGS[name]
    dev = torch.device("cuda")
    tbe = TableBatchedEmbeddingBags(
        GOLD_SPECS, optimizer=optim, learning_rate=LR, eps=EPS, beta1=BETA1, beta2=BETA2,
        device=dev, weights_precision=wprec, location=location, cache_load_factor=0.5,
        output_dtype=grad_dtype, stochastic_rounding=(wprec == "bf16"),
    )
    g = torch.Generator().manual_seed(99)
    w0 = (torch.rand(tbe.weights.numel(), generator=g) - 0.5) * 0.2
    tbe.weights.data.copy_(w0.to(tbe.weights.dtype))
    tbe._rng.fill_(0x1234567)
    for step in range(2):
        indices, offsets, grad = gold_batch(70 + step)
        out = tbe(indices.to(dev), offsets.to(dev))
        out.backward(grad.to(dev).to(out.dtype))
    torch.cuda.synchronize()
    bits = {torch.float32: torch.int32, torch.bfloat16: torch.int16}
    got = {}
    tensors = {"weights": tbe.weights, "momentum": tbe.momentum, "m1": tbe.m1, "m2": tbe.m2}
    if location == EmbeddingLocation.MANAGED_CACHING:
        tensors["cache_weights"] = tbe.cache_weights
        tensors["cache_tags"] = tbe.cache_tags
    for key, t in tensors.items():
        if t.numel() == 0:
            continue
        t = t.detach().cpu().contiguous()
        arr = t.view(bits[t.dtype]).numpy() if t.dtype in bits else t.numpy()
        got[f"{name}/{grad_dtype}/{key}"] = arr
    return got


class TestOptimizerGolden:
    @pytest.mark.parametrize("grad_dtype", ["fp32", "bf16"])
    @pytest.mark.parametrize("name", list(GOLD_CONFIGS))
    def test_states_equal_parent(self, name, grad_dtype):
        gold = np.load(GOLDEN)
        got = gold_states(name, grad_dtype)
        assert got, "nothing recorded"
        prefix = f"{name}/{grad_dtype}/"
        assert sorted(got) == sorted(k for k in gold.files if k.startswith(prefix))
        differ = {}
        for key, arr in got.items():
            want = gold[key]
            assert arr.dtype == want.dtype and arr.shape == want.shape, key
            if not np.array_equal(arr, want):
                differ[key] = f"{int((arr != want).sum())} of {arr.size}"
        assert not differ, f"values that differ from the parent's: {differ}"
