"""TBE backward chain past one scan tile, against exact sums.

The chain is sort -> prep_runs_lookback -> prep_chunks_lookback -> build_desc
-> long_partial -> fused. With integer gradients in [-8, 8], scales from
{0.5, 1, 2} and every sum of magnitudes below 2^23, each fp32 partial sum is
exact whatever the order, so the dense-gradient mode (2) of the chain equals
an fp64 ``index_add`` bit for bit. ``run_chain`` asserts that condition on the
reference before it compares; a case that trips it has wrong inputs.

Boundary -> tests whose inputs cross it:

- 2048-position scan tile (kScanTile = 256 x 8)
    TestRunDetection.test_prep_and_run_heads at n = 2047 / 2048 / 2049 / 4097
    (pattern "tile_edges" starts runs exactly at 2047, 2048 and 2049; "equal"
    is one run over every tile); TestChainExact.test_chunk_scan_across_tiles
    (about 45 position tiles and three tiles of the chunk scan, where a chunk
    prefix crosses a tile); TestOptimizerModes (five tiles).
- 64-tile lookback window (131072 positions)
    TestRunDetection at n = 2048*65 + 3 and 2048*130 + 17;
    test_run_heads_grid_stride and TestChainExact.test_large_strided
    (265 tiles).
- 32-occurrence chunk threshold (kChunkSize)
    TestChainExact.test_chunk_threshold: runs of 1, 31, 32, 33, 63, 64, 65,
    96, 97 and 1000, with and without a scale vector, fp32/bf16/fp16 grads.
- 2048-block grid cap of grid_for (524288 threads)
    test_run_heads_grid_stride (gather_run_heads) and test_large_strided
    (build_desc over positions, long_partial over > 16000 chunks), both at
    n = 2048*264 + 5; TestPerSampleWeightGrad (N = 40000 > 32768 slots).
- a slot that strides to a second run
    TestChainExact.test_grid_stride_over_runs (TREC_BWD_GRID_CAP=1: one
    block walks about 5100 runs).
- LPS/CHUNKS dispatch on max_D
    TestChainExact.test_dispatch_on_max_d: LPS 16, 32, 64 and CHUNKS 1, 2, 4, 8,
    each with a narrow table in the same launch as the wide one.
- two-level segmented sort feeding prep and update
    TestOptimizerModes.test_fixed_length_two_level_sort (cap = 4096).

To add a case: integer gradients, dyadic scales, and let ``run_chain`` assert
the 2^23 bound.
"""

import functools

import pytest
import torch

from torchrec_amd import ops
from torchrec_amd.ops.tbe import (
    OPT_DENSE,
    PoolingMode,
    TableBatchedEmbeddingBags,
    _bits_needed,
)

pytestmark = pytest.mark.gpu

TILE = 2048  # kScanTile
BIG_N = TILE * 264 + 5  # > 524288: past the grid cap of grid_for
EXACT_LIMIT = float(1 << 23)
SCALES = torch.tensor([0.5, 1.0, 2.0])


# ---------------------------------------------------------------------------
# 0. direct harness
# ---------------------------------------------------------------------------


class Layout:
    """Flat-buffer layout of a table group, built as the module builds it."""

    def __init__(self, specs):
        self.rows = [s[1] for s in specs]
        self.dims = [s[2] for s in specs]
        assert all(d % 4 == 0 for d in self.dims)  # 16 B-aligned element offsets
        self.row_off = [0]
        self.elem_off = [0]
        self.d_out = [0]
        for r, d in zip(self.rows, self.dims):
            self.row_off.append(self.row_off[-1] + r)
            self.elem_off.append(self.elem_off[-1] + r * d)
            self.d_out.append(self.d_out[-1] + d)
        self.total_rows = self.row_off[-1]
        self.total_elems = self.elem_off[-1]
        self.max_D = max(self.dims)


def reference_dense(lay, linear, pos_row, pos_col, grad, scale):
    """fp64: ref[lin] += scale_k * grad[pos_row_k, pos_col_k : pos_col_k + D]."""
    ref = torch.zeros(lay.total_elems, dtype=torch.float64)
    gflat = grad.double().reshape(-1)
    stride = grad.shape[1]
    sc = torch.ones(linear.numel(), dtype=torch.float64) if scale is None else scale.double()
    for t, D in enumerate(lay.dims):
        m = (linear >= lay.row_off[t]) & (linear < lay.row_off[t + 1])
        if not bool(m.any()):
            continue
        start = pos_row[m].long() * stride + pos_col[m]
        rows = gflat[start.unsqueeze(1) + torch.arange(D)] * sc[m].unsqueeze(1)
        view = ref[lay.elem_off[t] : lay.elem_off[t + 1]].view(lay.rows[t], D)
        view.index_add_(0, linear[m] - lay.row_off[t], rows)
    return ref


def assert_exact_inputs(grad, scale, ref_abs):
    """The condition under which fp32 accumulation is exact in every order."""
    g = grad.double()
    assert bool((g == g.round()).all()) and float(g.abs().max()) <= 8
    if scale is not None:
        assert bool(torch.isin(scale, SCALES).all())
    # bound on the sum of magnitudes: covers every partial sum and |row sum|
    assert float(ref_abs.max()) < EXACT_LIMIT


def run_chain(linear, pos_row, pos_col, grad, scale, specs, mode=OPT_DENSE, ref=None,
              ref_abs=None):
    """sort_pairs -> tbe_backward_prep -> tbe_backward_fused, called the way
    ``TableBatchedEmbeddingBags._backward_pooled`` calls them. Inputs are CPU
    tensors; returns (grad_weights on the CPU, fp64 reference)."""
    ops.hip_ops()
    lay = Layout(specs)
    if ref is None:
        ref = reference_dense(lay, linear, pos_row, pos_col, grad, scale)
        ref_abs = reference_dense(
            lay, linear, pos_row, pos_col, grad.abs(), scale
        )
    assert_exact_inputs(grad, scale, ref_abs)
    dev = torch.device("cuda")
    empty_f = torch.empty(0, dtype=torch.float32, device=dev)
    empty_i = torch.empty(0, dtype=torch.int32, device=dev)
    weights = torch.zeros(lay.total_elems, dtype=torch.float32, device=dev)
    grad_weights = torch.zeros_like(weights)
    sorted_lin, perm = torch.ops.trec_amd.sort_pairs(
        linear.to(dev), _bits_needed(lay.total_rows)
    )
    seg_offsets, num_runs = torch.ops.trec_amd.tbe_backward_prep(sorted_lin)
    torch.ops.trec_amd.tbe_backward_fused(
        weights,
        empty_f,
        grad.to(dev),
        sorted_lin,
        perm,
        seg_offsets,
        num_runs,
        pos_row.to(dev),
        pos_col.to(dev),
        scale.to(dev) if scale is not None else empty_f,
        torch.tensor(lay.row_off, dtype=torch.int64, device=dev),
        torch.tensor(lay.elem_off[:-1], dtype=torch.int64, device=dev),
        torch.tensor(lay.dims, dtype=torch.int32, device=dev),
        lay.max_D,
        0.0,
        1e-8,
        mode,
        grad_weights,
        empty_f,
        empty_i,
        empty_f,
        empty_f,
        0.9,
        0.999,
        empty_f,
        torch.empty(0, dtype=torch.int64, device=dev),
        False,
    )
    torch.cuda.synchronize()
    assert not bool(weights.any())  # mode 2 leaves the table alone
    return grad_weights.cpu(), ref


def make_positions(specs, runs, seed, grad_rows=64, with_scale=False, dtype=torch.float32):
    """Pooled layout: ``runs`` is a list of (table, local row, length); the
    positions are shuffled, each reads a random row of an integer gradient
    [grad_rows, total_D] at its table's column offset."""
    lay = Layout(specs)
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([r[0] for r in runs])
    lin = torch.tensor([lay.row_off[r[0]] + r[1] for r in runs])
    lens = torch.tensor([r[2] for r in runs])
    order = torch.randperm(int(lens.sum()), generator=g)
    linear = torch.repeat_interleave(lin, lens)[order]
    pos_col = torch.repeat_interleave(torch.tensor(lay.d_out)[t], lens)[order]
    n = linear.numel()
    pos_row = torch.randint(0, grad_rows, (n,), generator=g, dtype=torch.int32)
    grad = torch.randint(-8, 9, (grad_rows, lay.d_out[-1]), generator=g).to(dtype)
    scale = SCALES[torch.randint(0, 3, (n,), generator=g)] if with_scale else None
    return linear, pos_row, pos_col, grad, scale


# ---------------------------------------------------------------------------
# 1. run detection
# ---------------------------------------------------------------------------


def sorted_keys(pattern, n, seed=0):
    i = torch.arange(n, dtype=torch.int64)
    if pattern == "distinct":
        return i * 3 + 1
    if pattern == "equal":
        return torch.full((n,), 7, dtype=torch.int64)
    if pattern == "tile_edges":
        # a run starts exactly at 2047, 2048 and 2049, and likewise round every
        # later tile boundary
        off = i % TILE
        starts = ((off <= 1) & (i >= TILE)) | (off == TILE - 1)
        return torch.cumsum(starts.long(), 0) * 2
    assert pattern == "geometric"
    g = torch.Generator().manual_seed(seed)
    # geometric run lengths: each position starts a new run with p = 1/5
    starts = torch.rand(n, generator=g) < 0.2
    return torch.cumsum(starts.long(), 0) * 5 + 2


def check_run_detection(keys):
    ops.hip_ops()
    n = keys.numel()
    uniq, counts = torch.unique_consecutive(keys, return_counts=True)
    want = torch.zeros(uniq.numel() + 1, dtype=torch.int64)
    torch.cumsum(counts, 0, out=want[1:])
    dk = keys.cuda()
    seg_offsets, num_runs = torch.ops.trec_amd.tbe_backward_prep(dk)
    heads = torch.ops.trec_amd.gather_run_heads(dk, seg_offsets, num_runs)
    torch.cuda.synchronize()
    assert seg_offsets.shape == (n + 1,) and heads.shape == (n,)
    r = int(num_runs.item())
    assert r == uniq.numel()
    # entries past num_runs + 1 are uninitialised by design
    assert torch.equal(seg_offsets[: r + 1].cpu().long(), want)
    heads = heads.cpu()
    assert torch.equal(heads[:r], uniq)
    assert bool((heads[r:] == -1).all())


class TestRunDetection:
    @pytest.mark.parametrize("pattern", ["distinct", "equal", "tile_edges", "geometric"])
    @pytest.mark.parametrize(
        "n", [1, 2047, 2048, 2049, 4097, TILE * 65 + 3, TILE * 130 + 17]
    )
    def test_prep_and_run_heads(self, n, pattern):
        keys = sorted_keys(pattern, n)
        if pattern == "tile_edges" and n > 2049:
            starts = torch.nonzero(keys[1:] != keys[:-1]).flatten() + 1
            assert starts[:3].tolist() == [2047, 2048, 2049]
        check_run_detection(keys)

    @pytest.mark.parametrize("pattern", ["distinct", "geometric"])
    def test_run_heads_grid_stride(self, pattern):
        """n above 524288: gather_run_heads strides, the run scan walks four
        lookback windows."""
        assert BIG_N > 2048 * 256
        check_run_detection(sorted_keys(pattern, BIG_N, seed=1))

    def test_empty(self):
        ops.hip_ops()
        keys = torch.empty(0, dtype=torch.int64, device="cuda")
        seg_offsets, num_runs = torch.ops.trec_amd.tbe_backward_prep(keys)
        heads = torch.ops.trec_amd.gather_run_heads(keys, seg_offsets, num_runs)
        assert int(num_runs.item()) == 0
        assert seg_offsets.numel() == 1 and heads.numel() == 0


# ---------------------------------------------------------------------------
# 2. chunking and the update kernels, exact
# ---------------------------------------------------------------------------

RUN_LENGTHS = [1, 31, 32, 33, 63, 64, 65, 96, 97, 1000]


def threshold_runs(specs):
    """Every run length of RUN_LENGTHS on one row each, in every table that
    has the rows for it (a narrow table with fewer rows takes the first ones,
    which still straddle the threshold)."""
    runs = []
    for t, s in enumerate(specs):
        # spread the rows over the table; reversed in odd tables so the long
        # run is not always the last of its table
        lens = RUN_LENGTHS if t % 2 == 0 else RUN_LENGTHS[::-1]
        assert s[1] >= len(lens)
        step = s[1] // len(lens)
        runs += [(t, k * step, ln) for k, ln in enumerate(lens)]
    return runs


@functools.lru_cache(maxsize=None)
def chunk_scan_case():
    """About 5100 runs (three 2048-run tiles of the chunk scan), every 7th of
    length 33..200 and the rest 1..3: about 90k positions. Sequence layout:
    grad row == position."""
    specs = (("a", 2500, 32), ("b", 2600, 32))
    lay = Layout(specs)
    g = torch.Generator().manual_seed(11)
    R = lay.total_rows
    lens = torch.randint(1, 4, (R,), generator=g)
    long = torch.arange(R) % 7 == 3
    lens[long] = torch.randint(33, 201, (int(long.sum()),), generator=g)
    n = int(lens.sum())
    linear = torch.repeat_interleave(torch.arange(R), lens)[torch.randperm(n, generator=g)]
    grad = torch.randint(-8, 9, (n, 32), generator=g).float()
    scale = SCALES[torch.randint(0, 3, (n,), generator=g)]
    pos_row = torch.arange(n, dtype=torch.int32)
    pos_col = torch.zeros(n, dtype=torch.int64)
    refs = {}
    for key, sc in (("plain", None), ("scaled", scale)):
        refs[key] = (
            reference_dense(lay, linear, pos_row, pos_col, grad, sc),
            reference_dense(lay, linear, pos_row, pos_col, grad.abs(), sc),
        )
    assert R > 2 * TILE and n > 50000
    # a chunk prefix crosses a tile of the chunk scan: long runs on both sides
    assert bool(long[:TILE].any()) and bool(long[2 * TILE :].any())
    return specs, linear, pos_row, pos_col, grad, scale, refs


class TestChainExact:
    @pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16])
    @pytest.mark.parametrize("with_scale", [False, True])
    def test_chunk_threshold(self, dtype, with_scale):
        """Runs of 32 and fewer are walked inline, longer ones go through the
        long-partial kernel in chunks of 32: a dropped or doubled occurrence
        at a chunk edge breaks equality."""
        specs = [("t", 40, 64)]
        linear, pos_row, pos_col, grad, scale = make_positions(
            specs, threshold_runs(specs), seed=3, with_scale=with_scale, dtype=dtype
        )
        got, ref = run_chain(linear, pos_row, pos_col, grad, scale, specs)
        assert torch.equal(got.double(), ref)
        # every run length is there, and untouched rows stay zero
        assert int((ref.view(40, 64).abs().amax(1) > 0).sum()) == len(RUN_LENGTHS)

    @pytest.mark.parametrize(
        "dims",
        [[8, 64], [8, 64, 128], [192, 64], [320, 64], [1024, 8], [1280, 8]],
        ids=["lps16", "lps32", "lps64x1", "lps64x2", "lps64x4", "lps64x8"],
    )
    def test_dispatch_on_max_d(self, dims):
        """The narrow table shares the launch with the wide one: the
        ``col4 * 4 < D`` masks and desc_d are exercised and the max_D stride
        of the scratch rows differs from D."""
        specs = [(f"t{i}", 23 + 10 * i, d) for i, d in enumerate(dims)]
        linear, pos_row, pos_col, grad, scale = make_positions(
            specs, threshold_runs(specs), seed=5, with_scale=True
        )
        got, ref = run_chain(linear, pos_row, pos_col, grad, scale, specs)
        assert torch.equal(got.double(), ref)

    @pytest.mark.parametrize("scaled", ["plain", "scaled"])
    def test_chunk_scan_across_tiles(self, scaled):
        specs, linear, pos_row, pos_col, grad, scale, refs = chunk_scan_case()
        ref, ref_abs = refs[scaled]
        got, _ = run_chain(
            linear, pos_row, pos_col, grad, scale if scaled == "scaled" else None,
            specs, ref=ref, ref_abs=ref_abs,
        )
        assert torch.equal(got.double(), ref)

    def test_vbe_layout(self):
        """The packed VBE layout: one gradient row, pos_col at multiples of D."""
        specs, linear, pos_row, pos_col, grad, scale, refs = chunk_scan_case()
        ref, ref_abs = refs["scaled"]
        n, D = grad.shape
        got, _ = run_chain(
            linear, torch.zeros(n, dtype=torch.int32), torch.arange(n) * D,
            grad.view(1, -1), scale, specs, ref=ref, ref_abs=ref_abs,
        )
        assert torch.equal(got.double(), ref)

    def test_grid_stride_over_runs(self, monkeypatch):
        """One block of the fused kernel: every slot strides over hundreds of
        runs. Equal to the reference and to the uncapped result, bitwise."""
        specs, linear, pos_row, pos_col, grad, scale, refs = chunk_scan_case()
        ref, ref_abs = refs["scaled"]
        monkeypatch.delenv("TREC_BWD_GRID_CAP", raising=False)
        full, _ = run_chain(
            linear, pos_row, pos_col, grad, scale, specs, ref=ref, ref_abs=ref_abs
        )
        monkeypatch.setenv("TREC_BWD_GRID_CAP", "1")  # read on every call
        capped, _ = run_chain(
            linear, pos_row, pos_col, grad, scale, specs, ref=ref, ref_abs=ref_abs
        )
        assert torch.equal(capped.double(), ref)
        assert torch.equal(capped, full)

    def test_large_strided(self):
        """n = 2048*264 + 5 positions on 40 rows of one D=160 table (LPS 64):
        more than 16000 chunks on a long-partial grid of 2048 blocks x 4
        slots, a run scan past a full lookback window, build_desc strided."""
        specs = [("hot", 40, 160)]
        lay = Layout(specs)
        g = torch.Generator().manual_seed(17)
        n = BIG_N
        linear = torch.randint(0, 40, (n,), generator=g)
        pos_row = torch.randint(0, 64, (n,), generator=g, dtype=torch.int32)
        pos_col = torch.zeros(n, dtype=torch.int64)
        grad = torch.randint(-8, 9, (64, 160), generator=g).float()
        scale = SCALES[torch.randint(0, 3, (n,), generator=g)]
        # (table row x gradient row) weight matrix; nothing n x D is built
        w = torch.zeros(40, 64, dtype=torch.float64)
        w.index_put_((linear, pos_row.long()), scale.double(), accumulate=True)
        ref = (w @ grad.double()).reshape(-1)
        ref_abs = (w @ grad.double().abs()).reshape(-1)
        counts = torch.bincount(linear, minlength=40)
        assert int(((counts + 31) // 32).sum()) > 16000
        got, _ = run_chain(
            linear, pos_row, pos_col, grad, scale, specs, ref=ref, ref_abs=ref_abs
        )
        assert lay.total_elems == ref.numel()
        assert torch.equal(got.double(), ref)


# ---------------------------------------------------------------------------
# 3. optimizer modes at multi-tile size (module level)
# ---------------------------------------------------------------------------

OPT_SPECS = [("hot", 3, 64), ("mid", 500, 128), ("big", 50000, 32)]
OPTIMIZERS = ["sgd", "rowwise_adagrad", "adam", "partial_rowwise_adam"]
LR, EPS, BETA1, BETA2 = 0.05, 1.0e-8, 0.9, 0.999
ATOL, RTOL = 1e-5, 1e-4  # the project's own: TestTBEAdam.test_gpu_matches_cpu


def ragged_batch(specs, B, max_len, seed):
    g = torch.Generator().manual_seed(seed)
    F = len(specs)
    lengths = torch.randint(0, max_len + 1, (F * B,), generator=g)
    offsets = torch.zeros(F * B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    indices = torch.cat(
        [
            torch.randint(0, specs[f][1], (int(lengths[f * B : (f + 1) * B].sum()),), generator=g)
            for f in range(F)
        ]
    )
    total_D = sum(s[2] for s in specs)
    grad = torch.randint(-4, 5, (B, total_D), generator=g).float()
    return indices, offsets, grad


def summed_grads(specs, B, indices, offsets, grad):
    """Per table: fp64 summed gradient per row (SUM pooling) and touched mask."""
    lengths = offsets[1:] - offsets[:-1]
    bag = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
    out, col = [], 0
    for f, (_, rows, D) in enumerate(specs):
        m = torch.div(bag, B, rounding_mode="floor") == f
        G = torch.zeros(rows, D, dtype=torch.float64)
        G.index_add_(0, indices[m], grad[bag[m] - f * B, col : col + D].double())
        touched = torch.zeros(rows, dtype=torch.bool)
        touched[indices[m]] = True
        # the oracle calls a row touched when its summed gradient is non-zero
        assert bool((G[touched].abs().amax(1) > 0).all())
        assert float(G.abs().max()) < EXACT_LIMIT
        out.append((G, touched))
        col += D
    return out


class Fp64Step:
    """The four fused update formulas in fp64; only rows touched in a step
    update their moments."""

    def __init__(self, optim, weights):
        self.optim = optim
        self.w = [w.double().clone() for w in weights]
        self.t = 0
        self.mom = [torch.zeros(w.shape[0], dtype=torch.float64) for w in weights]
        self.m1 = [torch.zeros_like(w) for w in self.w]
        self.m2 = [
            torch.zeros_like(w) if optim == "adam"
            else torch.zeros(w.shape[0], dtype=torch.float64)
            for w in self.w
        ]

    def step(self, grads):
        self.t += 1
        bc1 = 1.0 / (1.0 - BETA1 ** self.t)
        bc2 = 1.0 / (1.0 - BETA2 ** self.t)
        for i, (G, tch) in enumerate(grads):
            g, w = G[tch], self.w[i]
            if self.optim == "sgd":
                w[tch] -= LR * g
            elif self.optim == "rowwise_adagrad":
                self.mom[i][tch] += g.pow(2).mean(1)
                w[tch] -= LR * g / (self.mom[i][tch].sqrt() + EPS).unsqueeze(1)
            else:
                self.m1[i][tch] = BETA1 * self.m1[i][tch] + (1 - BETA1) * g
                if self.optim == "adam":
                    self.m2[i][tch] = BETA2 * self.m2[i][tch] + (1 - BETA2) * g.pow(2)
                    denom = (self.m2[i][tch] * bc2).sqrt() + EPS
                else:
                    self.m2[i][tch] = BETA2 * self.m2[i][tch] + (1 - BETA2) * g.pow(2).mean(1)
                    denom = ((self.m2[i][tch] * bc2).sqrt() + EPS).unsqueeze(1)
                w[tch] -= LR * (self.m1[i][tch] * bc1) / denom

    def states(self):
        if self.optim == "sgd":
            return [[] for _ in self.w]
        if self.optim == "rowwise_adagrad":
            return [[m] for m in self.mom]
        return [[a, b] for a, b in zip(self.m1, self.m2)]


def make_tbe(specs, optim, device, **kw):
    return TableBatchedEmbeddingBags(
        specs, optimizer=optim, learning_rate=LR, eps=EPS, beta1=BETA1, beta2=BETA2,
        device=torch.device(device), **kw,
    )


def assert_meets_reference(tbe, ref):
    for wt, wr in zip(tbe.split_embedding_weights(), ref.w):
        torch.testing.assert_close(wt.cpu().double(), wr, atol=ATOL, rtol=RTOL)
    got, want = tbe.split_optimizer_states(), ref.states()
    assert len(got) == len(want)
    for sg, sr in zip(got, want):
        assert len(sg) == len(sr)
        for a, b in zip(sg, sr):
            torch.testing.assert_close(a.cpu().double(), b, atol=ATOL, rtol=RTOL)


@functools.lru_cache(maxsize=None)
def optimizer_case(optim):
    """Two ragged steps at B = 512 (about 9k positions, hot-table runs of
    about 1000), the start weights and the fp64 reference after them."""
    B = 512
    torch.manual_seed(0)
    w0 = make_tbe(OPT_SPECS, optim, "cpu").weights.detach().clone()
    batches = [ragged_batch(OPT_SPECS, B, 12, seed=20 + s) for s in range(2)]
    assert all(4 * TILE < b[0].numel() for b in batches)
    e = Layout(OPT_SPECS).elem_off
    ref = Fp64Step(
        optim, [w0[e[i] : e[i + 1]].view(s[1], s[2]) for i, s in enumerate(OPT_SPECS)]
    )
    for indices, offsets, grad in batches:
        ref.step(summed_grads(OPT_SPECS, B, indices, offsets, grad))
    return w0, batches, ref


def run_steps(tbe, batches, device):
    for indices, offsets, grad in batches:
        out = tbe(indices.to(device), offsets.to(device))
        out.backward(grad.to(device))
    if device == "cuda":
        torch.cuda.synchronize()


class TestOptimizerModes:
    @pytest.mark.parametrize("optim", OPTIMIZERS)
    def test_cpu_oracle_meets_fp64(self, optim):
        """Needs no GPU: the project's CPU oracle against the same reference."""
        w0, batches, ref = optimizer_case(optim)
        tbe = make_tbe(OPT_SPECS, optim, "cpu")
        tbe.weights.data.copy_(w0)
        run_steps(tbe, batches, "cpu")
        assert_meets_reference(tbe, ref)

    @pytest.mark.parametrize("optim", OPTIMIZERS)
    def test_gpu_meets_fp64(self, optim):
        w0, batches, ref = optimizer_case(optim)
        tbe = make_tbe(OPT_SPECS, optim, "cuda")
        tbe.weights.data.copy_(w0)
        run_steps(tbe, batches, "cuda")
        assert_meets_reference(tbe, ref)

    def test_fixed_length_two_level_sort(self):
        """B = 4096 with one id per bag: cap = 4096 takes the two-level sort
        with 8-item tiles and a merge round. Bitwise equal to the hipCUB path,
        and both meet the fp64 reference."""
        specs = [("hot", 5, 64), ("mid", 700, 32), ("big", 60000, 16)]
        B = 4096
        g = torch.Generator().manual_seed(31)
        indices = torch.cat([torch.randint(0, s[1], (B,), generator=g) for s in specs])
        offsets = torch.arange(3 * B + 1, dtype=torch.int64)
        grad = torch.randint(-4, 5, (B, 112), generator=g).float()
        torch.manual_seed(0)
        a = make_tbe(specs, "rowwise_adagrad", "cuda")
        b = make_tbe(specs, "rowwise_adagrad", "cuda", fixed_bag_length=1)
        b.weights.data.copy_(a.weights.data)
        assert b._seg_sort_ok and b.fixed_bag_length * B == 4096
        ref = Fp64Step("rowwise_adagrad", [w.cpu() for w in a.split_embedding_weights()])
        ref.step(summed_grads(specs, B, indices, offsets, grad))
        run_steps(a, [(indices, offsets, grad)], "cuda")
        run_steps(b, [(indices, offsets, grad)], "cuda")
        assert torch.equal(a.weights, b.weights)
        assert torch.equal(a.momentum, b.momentum)
        assert_meets_reference(a, ref)
        assert_meets_reference(b, ref)


# ---------------------------------------------------------------------------
# 4. the two small kernels
# ---------------------------------------------------------------------------


def psw_bound(dot, absdot, D):
    """A D-term fp32 dot: 2 * D * 2^-24 * sum|w_d * g_d|, plus one fp32 ulp of
    the result."""
    r32 = dot.abs().float()
    ulp = (torch.nextafter(r32, torch.full_like(r32, float("inf"))) - r32).double()
    return 2.0 * D * 2.0 ** -24 * absdot + ulp


class TestPerSampleWeightGrad:
    @pytest.mark.parametrize("wdtype", [torch.float32, torch.bfloat16])
    def test_kernel_matches_fp64_dot(self, wdtype):
        ops.hip_ops()
        specs = [("a", 50, 8), ("b", 300, 64), ("c", 1000, 200)]
        lay = Layout(specs)
        N, R = 40000, 128  # 16 lanes a position: the launch strides above 32768
        g = torch.Generator().manual_seed(41)
        weights = torch.randn(lay.total_elems, generator=g).to(wdtype)
        grad = torch.randn(R, lay.d_out[-1], generator=g)
        pos_table = torch.randint(0, 3, (N,), generator=g, dtype=torch.int32)
        rows_t = torch.tensor(lay.rows)[pos_table.long()]
        indices = (torch.rand(N, generator=g) * rows_t).long().clamp(max=rows_t - 1)
        pos_row = torch.randint(0, R, (N,), generator=g, dtype=torch.int32)
        pos_col = torch.tensor(lay.d_out)[pos_table.long()]
        dev = torch.device("cuda")
        out = torch.ops.trec_amd.tbe_grad_per_sample_weights(
            weights.to(dev),
            torch.tensor(lay.elem_off[:-1], dtype=torch.int64, device=dev),
            torch.tensor(lay.dims, dtype=torch.int32, device=dev),
            grad.to(dev), indices.to(dev), pos_row.to(dev), pos_col.to(dev),
            pos_table.to(dev), lay.max_D,
        )
        torch.cuda.synchronize()
        out = out.cpu().double()
        gflat = grad.double().reshape(-1)
        for t, D in enumerate(lay.dims):
            m = pos_table == t
            assert int(m.sum()) > 1000
            w = weights[lay.elem_off[t] : lay.elem_off[t + 1]].double().view(-1, D)[indices[m]]
            start = pos_row[m].long() * grad.shape[1] + pos_col[m]
            prod = w * gflat[start.unsqueeze(1) + torch.arange(D)]
            dot, absdot = prod.sum(1), prod.abs().sum(1)
            err = (out[m] - dot).abs()
            assert bool((err <= psw_bound(dot, absdot, D)).all()), (
                f"D={D}: worst error/bound {float((err / psw_bound(dot, absdot, D)).max())}"
            )

    def test_module_reads_rows_before_update(self):
        """psw.grad through the module: the dot is taken with the rows as they
        were before the fused update rewrote them."""
        specs = [("a", 20, 8), ("b", 200, 64)]
        B = 64
        torch.manual_seed(0)
        # a step large enough that rows read after the update would miss by far
        tbe = TableBatchedEmbeddingBags(
            specs, optimizer="sgd", learning_rate=1.0, device=torch.device("cuda")
        )
        w0 = [w.cpu().double().clone() for w in tbe.split_embedding_weights()]
        indices, offsets, _ = ragged_batch(specs, B, 6, seed=43)
        g = torch.Generator().manual_seed(44)
        grad = torch.randn(B, 72, generator=g)
        psw = (torch.rand(indices.numel(), generator=g) + 0.5).cuda().requires_grad_(True)
        out = tbe(indices.cuda(), offsets.cuda(), psw)
        out.backward(grad.cuda())
        torch.cuda.synchronize()
        assert psw.grad is not None
        got = psw.grad.cpu().double()
        lengths = offsets[1:] - offsets[:-1]
        bag = torch.repeat_interleave(torch.arange(lengths.numel()), lengths)
        col, moved = 0, 0.0
        for f, (_, _, D) in enumerate(specs):
            m = torch.div(bag, B, rounding_mode="floor") == f
            gr = grad[bag[m] - f * B, col : col + D].double()
            prod = w0[f][indices[m]] * gr
            dot, absdot = prod.sum(1), prod.abs().sum(1)
            assert bool(((got[m] - dot).abs() <= psw_bound(dot, absdot, D)).all())
            w1 = tbe.split_embedding_weights()[f].cpu().double()
            after = (w1[indices[m]] * gr).sum(1)
            moved = max(moved, float((after - dot).abs().max()))
            col += D
        assert moved > 1.0  # the update did rewrite the rows this reads


class TestBoundsCheck:
    def test_clamps_and_counts(self):
        ops.hip_ops()
        rows = torch.tensor([100, 37])
        feat_table = torch.tensor([0, 0, 1], dtype=torch.int32)  # two share table 0
        fvo = torch.tensor([0, 1200, 1200, 3000])  # feature 1 is empty
        N = 3000
        g = torch.Generator().manual_seed(51)
        ids = torch.cat(
            [torch.randint(0, 100, (1200,), generator=g), torch.randint(0, 37, (1800,), generator=g)]
        )
        # position -> (planted id, id after the check); first and last value of
        # each feature included. 50 is valid in table 0 and not in table 1.
        planted = {
            0: (-5, 0), 1: (100, 99), 2: (99, 99), 3: (0, 0), 600: (107, 99), 1199: (-1, 0),
            1200: (37, 36), 1201: (36, 36), 1202: (50, 36), 2000: (-1, 0), 2998: (0, 0),
            2999: (44, 36),
        }
        want = ids.clone()
        for p, (bad, fixed) in planted.items():
            ids[p] = bad
            want[p] = fixed
        n_bad = sum(1 for bad, fixed in planted.values() if bad != fixed)
        assert n_bad == 8
        dev = torch.device("cuda")
        d_ids = ids.to(dev)
        count = torch.ops.trec_amd.bounds_check_indices(
            d_ids, fvo.to(dev), rows.to(dev), feat_table.to(dev)
        )
        torch.cuda.synchronize()
        assert int(count.item()) == n_bad
        assert torch.equal(d_ids.cpu(), want)  # valid ids untouched, bad ones clamped

    def test_empty(self):
        ops.hip_ops()
        dev = torch.device("cuda")
        count = torch.ops.trec_amd.bounds_check_indices(
            torch.empty(0, dtype=torch.int64, device=dev),
            torch.zeros(2, dtype=torch.int64, device=dev),
            torch.tensor([10], device=dev),
            torch.zeros(1, dtype=torch.int32, device=dev),
        )
        assert int(count.item()) == 0
