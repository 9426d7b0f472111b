"""Pairwise-dot interaction kernels (interaction.hip, interaction_mfma.hip)
against a float64 oracle with a derived error bound.

Oracle. The MFMA kernels round their inputs to bf16 while staging; the VALU
kernels read fp32. The oracle applies the same rounding on the host
(``tensor.bfloat16()``, round-to-nearest-even), promotes to float64 and runs
the eager ``cat -> bmm -> triu gather -> cat`` chain with autograd. What is
left between kernel and oracle is the kernel's fp32 accumulation only.

The one input the MFMA backward does not round is ``grad_out[:, :D]``: it is
added to the dense gradient after the matrix product, in fp32, as given. The
oracle does the same, so a case with inputs that are not bf16-exact pins that
behaviour as well as the staging cast.

Bound (derived, not measured). Let u = 2^-24. A length-K fp32 accumulation in
any order, each step off by at most one ulp (this covers round-to-nearest and
chopping), errs by at most ``2 * K * u * sum_k |a_k b_k|``. Products of two
bf16 values are exact in fp32.
  forward:  K = D (MFMA), D + 1 (VALU, one more for the product rounding)
  backward: K = 32 (MFMA, the padded k-width), F1 + 1 (VALU, the dense
            passthrough counted as a term)
A 16-bit output adds one output ulp: ``2^-(p-1) * (|ref| + acc_bound)`` with
p = 8 (bf16) or 11 (fp16). Inputs have magnitudes in 2^-4..2^4 with random
signs, so no product is subnormal and nothing overflows fp16.

The CPU self-tests show that a plain fp32 ``bmm`` stays inside the bound at
every shape the GPU tests use and that each of six kernel mutants leaves it.
"""

import functools

import pytest
import torch

from torchrec_amd import ops

U = 2.0 ** -24
OUT_ULP = {torch.float64: 0.0, torch.float32: 0.0,
           torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}

MFMA_GRID = [(5, F1, D) for D in (32, 64, 96, 128, 160, 192, 224, 256)
             for F1 in (2, 15, 16, 17, 31, 32)]
MFMA_16BIT = [(5, F1, D) for D in (64, 128, 256) for F1 in (16, 17, 32)]
VALU_GRID = [(5, F1, D) for D in (4, 8, 36, 60, 128, 260) for F1 in (2, 5, 9, 33, 40)]
MFMA_LOOPS = [(8197, 4, 64), (2053, 4, 64)]
VALU_LOOPS = [(8197, 3, 4), (2053, 3, 4)]
VALU_BIG_LDS = (3, 33, 512)
VALU_WIDE = (2, 130, 4)  # F = 129
# every (mfma, B, F1, D) the GPU tests touch, for the CPU emulation self-test
ALL_SHAPES = (
    [(True,) + s for s in MFMA_GRID + MFMA_LOOPS + [(1, 17, 64), (6, 17, 64), (5, 8, 64)]]
    + [(False,) + s for s in VALU_GRID + VALU_LOOPS + [VALU_BIG_LDS, VALU_WIDE, (5, 6, 8)]]
)


# ------------------------------------------------------------------------
# inputs, oracle, bound
# ------------------------------------------------------------------------


def _draw(gen, *shape):
    mag = torch.exp2(torch.rand(*shape, generator=gen) * 8.0 - 4.0)
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2.0 - 1.0
    return mag * sign


def _inputs(B, F1, D, seed=0, bf16_exact=True):
    """fp32 CPU (dense, sparse, grad_out); bf16-exact unless asked otherwise."""
    gen = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + F1 * 263 + D)
    P = F1 * (F1 - 1) // 2
    xs = (_draw(gen, B, D), _draw(gen, B, F1 - 1, D), _draw(gen, B, D + P))
    if bf16_exact:
        xs = tuple(x.bfloat16().float() for x in xs)
    return xs


class Oracle:
    """float64 reference plus the |.|-companions the bound is built from."""

    def __init__(self, dense, sparse, grad_out, mfma):
        B, D = dense.shape
        F1 = sparse.shape[1] + 1
        self.B, self.D, self.F1, self.mfma = B, D, F1, mfma
        dense, sparse, grad_out = dense.cpu(), sparse.cpu(), grad_out.cpu()
        if mfma:
            dense, sparse = dense.bfloat16(), sparse.bfloat16()
            # the pair gradients are staged as bf16; the dense passthrough
            # columns are added in fp32 as given
            grad_out = torch.cat(
                [grad_out[:, :D].double(), grad_out[:, D:].bfloat16().double()], dim=1)
        self.dense_in = dense  # rounded input, for the passthrough check
        d = dense.double().requires_grad_(True)
        s = sparse.double().requires_grad_(True)
        g = grad_out.double()
        tri = torch.triu_indices(F1, F1, offset=1)
        T = torch.cat([d.unsqueeze(1), s], dim=1)
        Z = torch.bmm(T, T.transpose(1, 2))
        out = torch.cat([d, Z[:, tri[0], tri[1]]], dim=1)
        out.backward(g)
        self.out, self.d_dense, self.d_sparse = out.detach(), d.grad, s.grad
        Ta = T.detach().abs()
        self.T, self.g, self.tri = T.detach(), g, tri
        self.out_abs = torch.bmm(Ta, Ta.transpose(1, 2))[:, tri[0], tri[1]]
        Ga = torch.zeros(B, F1, F1, dtype=torch.float64)
        Ga[:, tri[0], tri[1]] = g[:, D:].abs()
        Ga = Ga + Ga.transpose(1, 2)
        grad_abs = torch.bmm(Ga, Ta)
        grad_abs[:, 0] += g[:, :D].abs()
        self.d_dense_abs, self.d_sparse_abs = grad_abs[:, 0], grad_abs[:, 1:]

    @property
    def k_fwd(self):
        return self.D if self.mfma else self.D + 1

    @property
    def k_bwd(self):
        return 32 if self.mfma else self.F1 + 1


def _bound(ref, ref_abs, K, out_dtype):
    acc = 2.0 * K * U * ref_abs
    return acc + OUT_ULP[out_dtype] * (ref.abs() + acc)


RATIOS = {}  # worst error / bound seen per kernel, printed for the record


def _check(kernel, what, got, ref, ref_abs, K, rows=None):
    out_dtype = got.dtype
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = _bound(ref, ref_abs, K, out_dtype)
    if rows is not None:
        got, ref, bound = got[rows], ref[rows], bound[rows]
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound, err)
    worst = float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0
    RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), worst)
    print(f"ratio {kernel} {what} {str(out_dtype)[6:]} shape={tuple(ref.shape)} "
          f"worst={worst:.4f}")
    bad = ~(err <= bound)  # NaN counts as bad
    assert not bool(bad.any()), (
        f"{kernel} {what}: {int(bad.sum())} of {bad.numel()} elements outside the bound, "
        f"worst error/bound {worst:.3g} at {bad.nonzero()[0].tolist()}")


def _check_all(orc, out, dd, ds, rows=None, tag=""):
    """out / dd / ds may be None (not computed or launch refused)."""
    D = orc.D
    kf, kb = ("mfma_fwd", "mfma_bwd") if orc.mfma else ("valu_fwd", "valu_bwd")
    kf, kb = tag + kf, tag + kb
    if out is not None:
        _check(kf, "out", out[:, D:], orc.out[:, D:], orc.out_abs, orc.k_fwd, rows)
        passthrough = orc.dense_in.to(out.dtype)
        got = out[:, :D].detach().cpu()
        if rows is not None:
            got, passthrough = got[rows], passthrough[rows]
        assert torch.equal(got, passthrough), "dense passthrough is not bit-equal"
    if dd is not None:
        _check(kb, "d_dense", dd, orc.d_dense, orc.d_dense_abs, orc.k_bwd, rows)
    if ds is not None:
        _check(kb, "d_sparse", ds, orc.d_sparse, orc.d_sparse_abs, orc.k_bwd, rows)


@functools.lru_cache(maxsize=None)
def _case(mfma, B, F1, D, seed=0, bf16_exact=True):
    """Inputs and oracle for one shape, computed once and shared; read-only."""
    dense, sparse, grad_out = _inputs(B, F1, D, seed, bf16_exact)
    return dense, sparse, grad_out, Oracle(dense, sparse, grad_out, mfma)


# ------------------------------------------------------------------------
# CPU self-tests of the oracle
# ------------------------------------------------------------------------


def _emulate_fp32(orc, io_dtype=torch.float32):
    """What a correct kernel may return: the same math in plain fp32 bmm."""
    T = orc.T.float()
    g = orc.g.float()
    D, F1, tri = orc.D, orc.F1, orc.tri
    Z = torch.bmm(T, T.transpose(1, 2))
    out = torch.cat([T[:, 0], Z[:, tri[0], tri[1]]], dim=1)
    G = torch.zeros(orc.B, F1, F1)
    G[:, tri[0], tri[1]] = g[:, D:]
    G = G + G.transpose(1, 2)
    dT = torch.bmm(G, T)
    dT[:, 0] += g[:, :D]
    return out.to(io_dtype), dT[:, 0].to(io_dtype), dT[:, 1:].to(io_dtype)


@pytest.mark.parametrize("mfma,B,F1,D", ALL_SHAPES)
def test_fp32_emulation_is_inside_the_bound(mfma, B, F1, D):
    orc = _case(mfma, B, F1, D)[3]
    _check_all(orc, *_emulate_fp32(orc), tag="emu_")


@pytest.mark.parametrize("io_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,F1,D", MFMA_16BIT)
def test_fp32_emulation_16bit_io_is_inside_the_bound(B, F1, D, io_dtype):
    orc = _case(True, B, F1, D)[3]
    _check_all(orc, *_emulate_fp32(orc, io_dtype), tag="emu_")


def _mutant(orc, name):
    """A float64 result that is exact except for one kernel-style mistake."""
    T, g, tri, D, F1 = orc.T.clone(), orc.g, orc.tri, orc.D, orc.F1
    Tz = T
    if name == "drop_last_k":
        Tz = T[:, :, :-1]
    elif name == "drop_k_chunk":
        Tz = T.clone()
        Tz[:, :, 8:16] = 0
    elif name == "zero_row_16":
        Tz = T.clone()
        Tz[:, 16] = 0
    Z = torch.bmm(Tz, Tz.transpose(1, 2))
    pairs = Z[:, tri[0], tri[1]]
    if name == "swap_pair_columns":
        p, q = 0, pairs.shape[1] - 1
        pairs = pairs.clone()
        pairs[:, [p, q]] = pairs[:, [q, p]]
    out = torch.cat([T[:, 0], pairs], dim=1)
    G = torch.zeros(orc.B, F1, F1, dtype=torch.float64)
    G[:, tri[0], tri[1]] = g[:, D:]
    if name != "upper_triangle_only":
        G = G + G.transpose(1, 2)
    dT = torch.bmm(G, Tz if Tz.shape == T.shape else T)
    if name != "no_passthrough":
        dT[:, 0] += g[:, :D]
    return out, dT[:, 0], dT[:, 1:]


MUTANTS = ["drop_last_k", "drop_k_chunk", "zero_row_16", "swap_pair_columns",
           "upper_triangle_only", "no_passthrough"]


@pytest.mark.parametrize("mfma,B,F1,D", [(True, 5, 17, 64), (True, 5, 32, 256),
                                        (False, 5, 33, 128)])
@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_is_caught(name, mfma, B, F1, D):
    orc = _case(mfma, B, F1, D)[3]
    out, dd, ds = _mutant(orc, name)
    _check_all(orc, *_mutant(orc, "none"), tag="exact_")  # unmutated passes
    with pytest.raises(AssertionError, match="outside the bound"):
        _check_all(orc, out, dd, ds, tag="mutant_")


def test_oracle_rounds_only_what_the_mfma_kernel_rounds():
    dense, sparse, grad_out = _inputs(3, 4, 32, seed=5, bf16_exact=False)
    orc = Oracle(dense, sparse, grad_out, mfma=True)
    assert torch.equal(orc.T[:, 0], dense.bfloat16().double())
    assert torch.equal(orc.g[:, :32], grad_out[:, :32].double())
    assert torch.equal(orc.g[:, 32:], grad_out[:, 32:].bfloat16().double())
    valu = Oracle(dense, sparse, grad_out, mfma=False)
    assert torch.equal(valu.T[:, 1:], sparse.double())


def test_pair_tables_hold_rows_above_127():
    F1 = VALU_WIDE[1]
    pi, pj, pair_col = ops._pair_tables(F1, torch.device("cpu"))
    tri = torch.triu_indices(F1, F1, offset=1)
    assert torch.equal(pi.long(), tri[0]) and torch.equal(pj.long(), tri[1])
    assert int(pj.max()) == F1 - 1
    p = torch.arange(pi.numel(), dtype=torch.int32)
    assert torch.equal(pair_col[tri[0] * F1 + tri[1]], p)
    assert torch.equal(pair_col[tri[1] * F1 + tri[0]], p)
    assert int((pair_col < 0).sum()) == F1  # the diagonal


# ------------------------------------------------------------------------
# GPU cases
# ------------------------------------------------------------------------

gpu = pytest.mark.gpu


def _fn(mfma):
    ops.hip_ops()
    return ops._FusedInteractionMFMA.apply if mfma else ops._FusedInteraction.apply


def _refused(e):
    return "HIP error" in str(e) or "LDS" in str(e)


def _run(fn, dense, sparse, grad_out, io_dtype=torch.float32, may_refuse=False):
    """Forward and backward on the GPU. With ``may_refuse`` a launch that is
    refused (it must raise) yields None for what it would have made."""
    d = dense.to("cuda", io_dtype).requires_grad_(True)
    s = sparse.to("cuda", io_dtype).requires_grad_(True)
    g = grad_out.to("cuda", io_dtype)
    try:
        out = fn(d, s)
        torch.cuda.synchronize()
    except RuntimeError as e:
        assert may_refuse and _refused(e), e
        return None, None, None
    try:
        out.backward(g)
        torch.cuda.synchronize()
    except RuntimeError as e:
        assert may_refuse and _refused(e), e
        return out.detach().cpu(), None, None
    return out.detach().cpu(), d.grad.cpu(), s.grad.cpu()


@gpu
@pytest.mark.parametrize("B,F1,D", MFMA_GRID + [(1, 17, 64)])
def test_mfma_grid_fp32_io(B, F1, D):
    dense, sparse, grad_out, orc = _case(True, B, F1, D)
    # 4 * (32*D*2 + 4096) bytes of LDS: above 64 KiB from D = 192 on, where
    # the launch may be refused but must then raise
    res = _run(_fn(True), dense, sparse, grad_out, may_refuse=D >= 192)
    _check_all(orc, *res)


@gpu
@pytest.mark.parametrize("io_dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("B,F1,D", MFMA_16BIT)
def test_mfma_grid_16bit_io(B, F1, D, io_dtype):
    dense, sparse, grad_out, orc = _case(True, B, F1, D)
    res = _run(_fn(True), dense, sparse, grad_out, io_dtype, may_refuse=D >= 192)
    assert res[0] is None or res[0].dtype == io_dtype
    _check_all(orc, *res)


@gpu
@pytest.mark.parametrize("B,F1,D", VALU_GRID)
def test_valu_grid(B, F1, D):
    dense, sparse, grad_out, orc = _case(False, B, F1, D)
    _check_all(orc, *_run(_fn(False), dense, sparse, grad_out))


@gpu
@pytest.mark.parametrize("mfma,B,F1,D", [(True,) + s for s in MFMA_LOOPS]
                         + [(False,) + s for s in VALU_LOOPS])
def test_grid_stride_second_trip(mfma, B, F1, D):
    """B just past the persistent grid's cap (4 * 2048 samples for the MFMA
    forward, 8192 for the VALU forward, 2048 for both backwards): some blocks
    stage a second sample over the first one's LDS tiles."""
    dense, sparse, grad_out, orc = _case(mfma, B, F1, D)
    _check_all(orc, *_run(_fn(mfma), dense, sparse, grad_out))


@gpu
@pytest.mark.parametrize("io_dtype", [torch.float32, torch.float16])
def test_mfma_rounds_inputs_to_nearest_even(io_dtype):
    """Inputs that are not bf16-exact: the staging cast must agree with
    ``tensor.bfloat16()``. fp16 inputs hit exact ties one time in eight."""
    dense, sparse, grad_out = (x.to(io_dtype) for x in _inputs(5, 17, 64, 3, False))
    assert not torch.equal(sparse.float(), sparse.bfloat16().float())
    orc = Oracle(dense.float(), sparse.float(), grad_out.float(), mfma=True)
    _check_all(orc, *_run(_fn(True), dense, sparse, grad_out, io_dtype))


@gpu
def test_valu_over_64k_lds_matches_or_raises():
    """F1 = 33, D = 512 needs 68 112 B of LDS forward and more backward."""
    B, F1, D = VALU_BIG_LDS
    dense, sparse, grad_out, orc = _case(False, B, F1, D)
    _check_all(orc, *_run(_fn(False), dense, sparse, grad_out, may_refuse=True))


@gpu
def test_valu_over_lds_capacity_raises():
    """A workgroup can have 160 KiB of LDS. 41 rows of D = 1024 need 168 592 B
    forward; 170 rows of D = 4 fit forward (5 440 B) but need 178 500 B
    backward. Either must raise instead of returning unwritten memory."""
    fn = _fn(False)
    dense, sparse, _ = _inputs(1, 41, 1024)
    with pytest.raises(RuntimeError, match="LDS"):
        fn(dense.cuda(), sparse.cuda())
    dense, sparse, grad_out = _inputs(1, 170, 4)
    d = dense.cuda().requires_grad_(True)
    out = fn(d, sparse.cuda().requires_grad_(True))
    with pytest.raises(RuntimeError, match="LDS"):
        out.backward(grad_out.cuda())
    torch.cuda.synchronize()
    assert d.grad is None


@gpu
def test_valu_pair_tables_above_127_rows():
    """F = 129: pair rows 128 and 129 do not fit a signed byte."""
    B, F1, D = VALU_WIDE
    dense, sparse, grad_out, orc = _case(False, B, F1, D)
    res = _run(_fn(False), dense, sparse, grad_out, may_refuse=True)
    assert res[0] is not None, "the forward needs 4 KiB of LDS and must launch"
    _check_all(orc, *res)


def _dispatch_expected(D, F1):
    return D % 32 == 0 and 64 <= D <= 256 and F1 <= 32


@gpu
@pytest.mark.parametrize("F1,D", [(8, 32), (8, 64), (8, 80), (8, 256), (8, 288),
                                  (32, 64), (33, 64)])
def test_dispatch_boundaries(F1, D, monkeypatch):
    """Which kernel ran shows in the passthrough columns: the MFMA kernel
    returns the dense input rounded to bf16, the VALU kernel returns it as
    given. Each side must also meet its own oracle."""
    monkeypatch.delenv("TREC_INTERACTION_FP32", raising=False)
    dense, sparse, grad_out = _inputs(5, F1, D, seed=4, bf16_exact=False)
    assert not torch.equal(dense, dense.bfloat16().float())
    mfma = _dispatch_expected(D, F1)
    assert ops._mfma_interaction_ok(dense, sparse) == mfma
    ops.hip_ops()
    out, dd, ds = _run(ops.fused_interaction, dense, sparse, grad_out)
    assert torch.equal(out[:, :D], dense.bfloat16().float() if mfma else dense)
    _check_all(Oracle(dense, sparse, grad_out, mfma), out, dd, ds)


@gpu
def test_dispatch_env_forces_valu(monkeypatch):
    dense, sparse, grad_out = _inputs(5, 8, 128, seed=4, bf16_exact=False)
    ops.hip_ops()
    monkeypatch.delenv("TREC_INTERACTION_FP32", raising=False)
    out = _run(ops.fused_interaction, dense, sparse, grad_out)[0]
    assert torch.equal(out[:, :128], dense.bfloat16().float())
    monkeypatch.setenv("TREC_INTERACTION_FP32", "1")
    assert not ops._mfma_interaction_ok(dense, sparse)
    out, dd, ds = _run(ops.fused_interaction, dense, sparse, grad_out)
    assert torch.equal(out[:, :128], dense)
    _check_all(Oracle(dense, sparse, grad_out, False), out, dd, ds)


@gpu
@pytest.mark.parametrize("mfma,B,F1,D", [(True, 5, 6, 64), (False, 5, 6, 8)])
def test_non_contiguous_inputs_and_grad(mfma, B, F1, D):
    """sparse, dense and grad_out as transposed views of other layouts. The
    backward writes its results contiguous, so it must not allocate them with
    the inputs' strides."""
    dense, sparse, grad_out, orc = _case(mfma, B, F1, D)
    d = dense.t().contiguous().cuda().t().requires_grad_(True)            # [D,B].t()
    s = sparse.transpose(0, 1).contiguous().cuda().transpose(0, 1).requires_grad_(True)
    g = grad_out.t().contiguous().cuda().t()                               # [D+P,B].t()
    assert not d.is_contiguous() and not s.is_contiguous() and not g.is_contiguous()
    out = _fn(mfma)(d, s)
    out.backward(g)
    torch.cuda.synchronize()
    _check_all(orc, out.detach().cpu(), d.grad.cpu(), s.grad.cpu())


@gpu
def test_permute_pooled_embs_non_contiguous():
    gen = torch.Generator().manual_seed(11)
    B, dims = 5, [4, 8, 4, 12]
    order = torch.tensor([2, 0, 3, 1])
    base = torch.randn(sum(dims), B, generator=gen)
    gbase = torch.randn(sum(dims), B, generator=gen)
    v_cpu = base.t().requires_grad_(True)
    ref = ops.permute_pooled_embs(v_cpu, dims, order)
    ref.backward(gbase.t())
    v_gpu = base.cuda().t().requires_grad_(True)
    assert not v_gpu.is_contiguous()
    got = ops.permute_pooled_embs(v_gpu, dims, order.cuda())
    got.backward(gbase.cuda().t())
    torch.cuda.synchronize()
    assert torch.equal(got.detach().cpu(), ref.detach())
    assert torch.equal(v_gpu.grad.cpu(), v_cpu.grad)


@gpu
def test_mfma_mixed_dtype_grads_keep_input_dtypes():
    B, F1, D = 5, 8, 64
    dense, sparse, grad_out, orc = _case(True, B, F1, D)
    d = dense.to("cuda", torch.bfloat16).requires_grad_(True)
    s = sparse.cuda().requires_grad_(True)
    out = _fn(True)(d, s)
    out.backward(grad_out.cuda())
    torch.cuda.synchronize()
    assert d.grad.dtype == torch.bfloat16 and s.grad.dtype == torch.float32
    _check_all(orc, out.detach().cpu(), d.grad.cpu(), s.grad.cpu())


@gpu
def test_mfma_nan_and_inf_samples_stay_in_their_tile():
    """Samples 1 (NaN) and 4 (+inf) share a block with clean samples."""
    B, F1, D = 6, 17, 64
    dense, sparse, grad_out, orc = _case(True, B, F1, D)
    dense, sparse, grad_out = dense.clone(), sparse.clone(), grad_out.clone()
    for x in (dense, sparse, grad_out):
        x[1] = float("nan")
        x[4] = float("inf")
    out, dd, ds = _run(_fn(True), dense, sparse, grad_out)
    _check_all(orc, out, dd, ds, rows=[0, 2, 3, 5])
    assert out[1].isnan().all() and not out[4].isfinite().any()


@gpu
@pytest.mark.parametrize("mfma,B,F1,D", [(True, 5, 17, 128), (False, 5, 9, 36)])
def test_two_runs_are_bit_equal(mfma, B, F1, D):
    dense, sparse, grad_out, _ = _case(mfma, B, F1, D)
    a = _run(_fn(mfma), dense, sparse, grad_out)
    b = _run(_fn(mfma), dense, sparse, grad_out)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
