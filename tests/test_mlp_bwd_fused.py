"""Two-kernel MLP backward tail (@gpu): relu_bwd_colsum_partial (mask + small
fp32 bias-grad partials) and splitk_fold_bias (split-K chunk sum + bias fold),
their use from _LinearReLUFused, determinism and hipGraph capture.

References are plain PyTorch in fp32/fp64."""

import pytest
import torch

from torchrec_amd import ops

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
# one unit in the last place of the output dtype
ULP = {torch.float32: 1e-6, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
PARTIAL_BYTES = 256 * 1024


def _partial(dy, y):
    ops.hip_ops()
    return torch.ops.trec_amd.relu_bwd_colsum_partial(dy, y)


def _fold(parts, partial):
    ops.hip_ops()
    return torch.ops.trec_amd.splitk_fold_bias(parts, partial)


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


class TestPartialKernel:
    @pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
    @pytest.mark.parametrize(
        "M,N", [(1, 8), (3, 5), (257, 264), (500, 300), (4100, 136)]
    )
    def test_mask_and_partials(self, M, N, dtype):
        """g equals dy * (y > 0) (torch.equal), and is bit-for-bit the select
        form where(y > 0, dy, 0): kept lanes carry dy's bits, masked lanes are
        +0 (the product form yields -0 for negative dy there, which compares
        equal). partial.sum(0) is the column sum within M * eps_fp32 * max|g|
        ~ 4100 * 6e-8 * 5 ~ 1e-3."""
        torch.manual_seed(M * 1000 + N)
        y = torch.randn(M, N, device="cuda").to(dtype).relu()
        dy = torch.randn(M, N, device="cuda").to(dtype)
        g, partial = _partial(dy, y)
        torch.cuda.synchronize()
        assert g.dtype == dtype and g.shape == (M, N)
        assert torch.equal(g, dy * (y > 0))
        sel = torch.where(y > 0, dy, torch.zeros_like(dy))
        assert torch.equal(_bits(g), _bits(sel))
        assert partial.dtype == torch.float32 and partial.dim() == 2
        assert partial.shape[1] == N and partial.shape[0] >= 1
        assert partial.numel() * 4 <= PARTIAL_BYTES
        ref = sel.double().sum(0)
        got = partial.sum(0).double()
        print(f"partial M={M} N={N} {dtype}: G={partial.shape[0]} "
              f"max|err|={(got - ref).abs().max().item():.3e}")
        torch.testing.assert_close(got, ref, atol=1e-3, rtol=1e-5)

    @pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
    def test_empty_batch(self, dtype):
        z = torch.empty(0, 8, device="cuda", dtype=dtype)
        g, partial = _partial(z, z)
        torch.cuda.synchronize()
        assert g.shape == (0, 8)
        assert partial.shape[1] == 8 and partial.numel() == 0

    def test_partial_stays_small_at_layer_shapes(self):
        # the dense-arch / over-arch widths at the flagship batch
        for N in (128, 256, 512, 1024):
            y = torch.ones(8192, N, device="cuda", dtype=torch.bfloat16)
            _, partial = _partial(y, y)
            assert partial.numel() * 4 <= PARTIAL_BYTES
            # all-ones: every column sums to exactly M
            assert torch.equal(partial.sum(0), torch.full((N,), 8192.0, device="cuda"))


_GMAX = {}


def _largest_g(N):
    """Largest G the partial op produces for width N: G grows with the row
    count up to its cap, which M = 8192 (256 row tiles of 32) reaches."""
    if N not in _GMAX:
        z = torch.zeros(8192, N, device="cuda")
        _GMAX[N] = _partial(z, z)[1].shape[0]
    return _GMAX[N]


class TestFoldKernel:
    @pytest.mark.parametrize("dtype", DTYPES, ids=["fp32", "bf16", "fp16"])
    @pytest.mark.parametrize("gmode", ["g1", "gmax"])
    @pytest.mark.parametrize("S,N,K", [(1, 5, 3), (8, 96, 64), (8, 136, 479)])
    def test_matches_fp64(self, S, N, K, gmode, dtype):
        """dW vs the fp64 chunk sum and db vs the fp64 fold: rtol one output
        ulp, atol 1e-5 for cancellation. Inputs are scaled so that the fp32
        accumulation error sits well inside atol: the db fold is a chain of
        at most 31 fp32 adds (16 per row lane + 15 across lanes); with 0.25 *
        randn partials the running sums stay ~4, rounding ~1.4e-7 rms per add,
        ~8e-7 rms per column and ~3e-6 at the largest of 136 columns."""
        G = 1 if gmode == "g1" else _largest_g(N)
        torch.manual_seed(S * 100000 + N * 1000 + K + G)
        parts = torch.randn(S, N, K, device="cuda").to(dtype)
        partial = 0.25 * torch.randn(G, N, device="cuda")
        dw, db = _fold(parts, partial)
        torch.cuda.synchronize()
        assert dw.shape == (N, K) and dw.dtype == dtype
        assert db.shape == (N,) and db.dtype == dtype
        ref_dw = parts.double().sum(0)
        ref_db = partial.double().sum(0)
        print(f"fold S={S} N={N} K={K} G={G} {dtype}: "
              f"dW max|err|={(dw.double() - ref_dw).abs().max().item():.3e} "
              f"db max|err|={(db.double() - ref_db).abs().max().item():.3e}")
        torch.testing.assert_close(dw.double(), ref_dw, rtol=ULP[dtype], atol=1e-5)
        torch.testing.assert_close(db.double(), ref_db, rtol=ULP[dtype], atol=1e-5)


def test_bitwise_repeatable_at_layer_shape():
    torch.manual_seed(7)
    y = torch.randn(8192, 1024, device="cuda", dtype=torch.bfloat16).relu()
    dy = torch.randn(8192, 1024, device="cuda", dtype=torch.bfloat16)
    g1, p1 = _partial(dy, y)
    g2, p2 = _partial(dy, y)
    parts = torch.randn(8, 1024, 1024, device="cuda", dtype=torch.bfloat16)
    dw1, db1 = _fold(parts, p1)
    dw2, db2 = _fold(parts, p1)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(p1), _bits(p2))
    assert torch.equal(_bits(dw1), _bits(dw2)) and torch.equal(_bits(db1), _bits(db2))


def _fused_fwd_bwd(x, w, b, gout):
    from torchrec_amd.modules.mlp import _LinearReLUFused

    y = _LinearReLUFused.apply(x, w, b)
    dx, dw, db = torch.autograd.grad(y, (x, w, b), gout)
    return y, dx, dw, db


def _fused_env(monkeypatch):
    # the module reads these at call time
    monkeypatch.setenv("TREC_RELU_COLSUM", "1")
    monkeypatch.setenv("TREC_SPLITK_WGRAD", "1")
    monkeypatch.delenv("TREC_LT_MLP", raising=False)
    monkeypatch.delenv("TREC_LT_MLP_FWD", raising=False)


class TestAutograd:
    # B = 4096 takes the split-K path (partial + bmm + fold), B = 24 the
    # non-split one (relu_bwd_col_sum + plain wgrad)
    @pytest.mark.parametrize("B", [4096, 24], ids=["split", "nosplit"])
    def test_matches_fp32_eager(self, B, monkeypatch):
        _fused_env(monkeypatch)
        K, N = 72, 136
        torch.manual_seed(0)
        bf = dict(device="cuda", dtype=torch.bfloat16, requires_grad=True)
        x, w, b = torch.randn(B, K, **bf), torch.randn(N, K, **bf), torch.randn(N, **bf)
        gout = torch.randn(B, N, device="cuda", dtype=torch.bfloat16)
        y, dx, dw, db = _fused_fwd_bwd(x, w, b, gout)
        xr = x.detach().float().requires_grad_(True)
        wr = w.detach().float().requires_grad_(True)
        br = b.detach().float().requires_grad_(True)
        yr = torch.relu(torch.nn.functional.linear(xr, wr, br))
        dxr, dwr, dbr = torch.autograd.grad(yr, (xr, wr, br), gout.float())
        torch.cuda.synchronize()
        assert dw.dtype == torch.bfloat16 and db.dtype == torch.bfloat16
        for name, a, r in (("y", y, yr), ("dx", dx, dxr), ("dw", dw, dwr), ("db", db, dbr)):
            print(f"autograd B={B} {name}: max|err|={(a.float() - r).abs().max().item():.3e}")
        torch.testing.assert_close(y.float(), yr.detach(), atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(dx.float(), dxr, atol=5e-2, rtol=5e-2)
        torch.testing.assert_close(dw.float(), dwr, atol=1.0, rtol=5e-2)
        torch.testing.assert_close(db.float(), dbr, atol=1.0, rtol=5e-2)


def test_split_path_graph_capture_replays_bitwise(monkeypatch):
    _fused_env(monkeypatch)
    B, K, N = 4096, 72, 136
    torch.manual_seed(1)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    w = torch.randn(N, K, requires_grad=True, **bf)
    b = torch.randn(N, requires_grad=True, **bf)
    x_s = torch.randn(B, K, requires_grad=True, **bf)
    g_s = torch.randn(B, N, **bf)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _fused_fwd_bwd(x_s, w, b, g_s)
    torch.cuda.current_stream().wait_stream(side)

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _fused_fwd_bwd(x_s, w, b, g_s)

    for seed in (11, 12):
        torch.manual_seed(seed)
        x_new, g_new = torch.randn(B, K, **bf), torch.randn(B, N, **bf)
        with torch.no_grad():
            x_s.copy_(x_new)
            g_s.copy_(g_new)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.detach().clone() for o in outs]
        want = _fused_fwd_bwd(x_new.requires_grad_(True), w, b, g_new)
        torch.cuda.synchronize()
        for name, a, r in zip(("y", "dx", "dw", "db"), got, want):
            assert torch.equal(_bits(a), _bits(r.detach())), name
