"""The logit head ``Linear(K, 1)`` as vector kernels (mlp_ops.hip):
linear_out1_fwd, linear_out1_bwd and linear_out1_fold, and their wiring in
``LogitLinear`` / ``OverArch``.

Oracle. float64 on the operands the kernel computes on. Inputs are bf16-exact
(hence fp16-exact) with magnitudes 2^-4..2^4 and random signs, so every
product is exact in fp32 and nothing overflows fp16.

Bound (derived, not measured). With u = 2^-24, an fp32 accumulation of R terms
in any order errs by at most ``2 * (R + 1) * u * sum_r |a_r b_r|``; the bias
counts as one of the terms' magnitudes. R = K for the forward and for dx,
R = M for dw and db. A 16-bit output adds one output ulp,
``2^-(p-1) * (|ref| + acc_bound)`` with p = 8 (bf16) or 11 (fp16).

The CPU self-tests show that a plain fp32 torch computation stays inside the
bound at every shape the GPU tests use, and that two mutants (the last k term
dropped, the last row group dropped) leave it.

Worst error / bound seen on the MI355X is logged in docs/KERNELS.md, Round 6.
"""

import functools

import pytest
import torch

from torchrec_amd import ops

U = 2.0 ** -24
OUT_ULP = {torch.float64: 0.0, torch.float32: 0.0,
           torch.bfloat16: 2.0 ** -7, torch.float16: 2.0 ** -10}
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
DTYPE_IDS = ["bf16", "fp16", "fp32"]

HEAD_SHAPES = [(1, 8), (33, 256), (4099, 264)]  # (M, K)
ROW_GROUP = 8  # the smallest row group the backward kernel forms


def _draw(gen, *shape):
    mag = torch.exp2(torch.rand(*shape, generator=gen) * 8.0 - 4.0)
    sign = torch.randint(0, 2, shape, generator=gen).float() * 2.0 - 1.0
    return (mag * sign).bfloat16().float()


def _bits(t):
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _bound(ref, ref_abs, R, out_dtype):
    acc = 2.0 * (R + 1) * U * ref_abs
    return acc + OUT_ULP[out_dtype] * (ref.abs() + acc)


RATIOS = {}  # worst error / bound per output, printed for the record


def _ratio(got, ref, ref_abs, R, out_dtype):
    got = got.detach().cpu().double().reshape(ref.shape)
    bound = _bound(ref, ref_abs, R, out_dtype)
    err = (got - ref).abs()
    ratio = torch.where(bound > 0, err / bound, err)
    return float(ratio.nan_to_num(nan=float("inf")).max()) if ratio.numel() else 0.0


def _check(what, got, ref, ref_abs, R):
    assert got.numel() == ref.numel(), (what, got.shape, ref.shape)
    worst = _ratio(got, ref, ref_abs, R, got.dtype)
    RATIOS[what] = max(RATIOS.get(what, 0.0), worst)
    print(f"ratio {what} {str(got.dtype)[6:]} shape={tuple(ref.shape)} worst={worst:.4f}")
    assert worst <= 1.0, f"{what}: error is {worst:.3f} x the bound"


# ------------------------------------------------------------------------
# inputs and float64 oracles (CPU, computed once per case and never modified)
# ------------------------------------------------------------------------


@functools.lru_cache(maxsize=None)
def _head_case(M, K):
    gen = torch.Generator().manual_seed(M * 7919 + K)
    x, w, b, dy = _draw(gen, M, K), _draw(gen, 1, K), _draw(gen, 1), _draw(gen, M, 1)
    xd, wd, bd, dd = x.double(), w.double(), b.double(), dy.double()
    ref = dict(
        y=xd @ wd.t() + bd, y_abs=xd.abs() @ wd.abs().t() + bd.abs(),
        dx=dd * wd, dx_abs=(dd * wd).abs(),
        dw=dd.t() @ xd, dw_abs=dd.abs().t() @ xd.abs(),
        db=dd.sum(0), db_abs=dd.abs().sum(0),
    )
    return (x, w, b, dy), ref


# ------------------------------------------------------------------------
# CPU self-tests of the bound
# ------------------------------------------------------------------------


def _fp32_head(x, w, b, dy, drop_k=0, drop_rows=0):
    """Plain fp32 torch; drop_k / drop_rows build the two mutants."""
    K, M = x.shape[1] - drop_k, x.shape[0] - drop_rows
    return dict(
        y=x[:, :K] @ w[:, :K].t() + b, dx=dy * w,
        dw=dy[:M].t() @ x[:M], db=dy[:M].sum(0),
    )


def _worst(out, ref, name, R):
    return _ratio(out[name], ref[name], ref[name + "_abs"], R, torch.float32)


@pytest.mark.parametrize("M,K", HEAD_SHAPES)
def test_cpu_bound_holds_head_fp32_and_mutants_leave_it(M, K):
    (x, w, b, dy), ref = _head_case(M, K)
    good = _fp32_head(x, w, b, dy)
    for name, R in (("y", K), ("dx", K), ("dw", M), ("db", M)):
        assert _worst(good, ref, name, R) <= 1.0, name
    assert _worst(_fp32_head(x, w, b, dy, drop_k=1), ref, "y", K) > 1.0
    lost = _fp32_head(x, w, b, dy, drop_rows=min(M, ROW_GROUP))
    assert _worst(lost, ref, "dw", M) > 1.0 and _worst(lost, ref, "db", M) > 1.0


def test_over_arch_state_dict_unchanged():
    from torchrec_amd.models.dlrm import OverArch

    sd = OverArch(16, [8, 4, 1]).state_dict()
    assert list(sd.keys()) == [
        "model.0._mlp.0._linear.weight",
        "model.0._mlp.0._linear.bias",
        "model.0._mlp.1._linear.weight",
        "model.0._mlp.1._linear.bias",
        "model.1.weight",
        "model.1.bias",
    ]
    assert [tuple(v.shape) for v in sd.values()] == [
        (8, 16), (8,), (4, 8), (4,), (1, 4), (1,)
    ]
    assert isinstance(OverArch(16, [8, 1]).model[1], torch.nn.Linear)


def test_cpu_input_takes_nn_linear():
    from torchrec_amd.modules.mlp import LogitLinear

    torch.manual_seed(0)
    lin = LogitLinear(8, 1)
    x = torch.randn(5, 8)
    assert torch.equal(lin(x), torch.nn.functional.linear(x, lin.weight, lin.bias))


# ------------------------------------------------------------------------
# GPU: the ops against the oracle
# ------------------------------------------------------------------------


def _op(name):
    ops.hip_ops()
    return getattr(torch.ops.trec_amd, name)


def _cuda(ts, dtype):
    return [t.to("cuda", dtype) for t in ts]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("M,K", HEAD_SHAPES)
def test_head_forward(M, K, dtype):
    inputs, ref = _head_case(M, K)
    x, w, b, _ = _cuda(inputs, dtype)
    y = _op("linear_out1_fwd")(x, w, b)
    y2 = _op("linear_out1_fwd")(x, w, b)
    assert y.shape == (M, 1) and y.dtype == dtype
    _check("head.y", y, ref["y"], ref["y_abs"], K)
    assert torch.equal(_bits(y), _bits(y2))


@pytest.mark.gpu
@pytest.mark.parametrize("need_dx", [True, False], ids=["dx", "nodx"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
@pytest.mark.parametrize("M,K", HEAD_SHAPES)
def test_head_backward(M, K, dtype, need_dx):
    inputs, ref = _head_case(M, K)
    x, w, _, dy = _cuda(inputs, dtype)

    def run():
        dx, partial = _op("linear_out1_bwd")(dy, x, w, need_dx)
        dw, db = _op("linear_out1_fold")(partial, w)
        return dx, partial, dw, db

    dx, partial, dw, db = run()
    assert partial.dtype == torch.float32 and partial.shape[1] == K + 1
    assert 1 <= partial.shape[0] <= 256
    assert dw.shape == (1, K) and db.shape == (1,) and dw.dtype == db.dtype == dtype
    if need_dx:
        assert dx.shape == (M, K) and dx.dtype == dtype
        _check("head.dx", dx, ref["dx"], ref["dx_abs"], K)
    else:
        assert dx.numel() == 0
    _check("head.dw", dw, ref["dw"], ref["dw_abs"], M)
    _check("head.db", db, ref["db"], ref["db_abs"], M)
    for a, r in zip((dx, partial, dw, db), run()):
        assert torch.equal(_bits(a), _bits(r))


# ------------------------------------------------------------------------
# GPU: the modules
# ------------------------------------------------------------------------


def _grad_fn_name(t):
    return type(t.grad_fn).__name__


@pytest.mark.gpu
def test_head_fallback_is_nn_linear_bitwise(monkeypatch):
    """K = 13 is no multiple of 8: LogitLinear must be F.linear bit for bit."""
    from torchrec_amd.modules.mlp import LogitLinear

    monkeypatch.setenv("TREC_THIN_LAYERS", "1")
    torch.manual_seed(3)
    lin = LogitLinear(13, 1, device="cuda", dtype=torch.bfloat16)
    x = torch.randn(5, 13, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    gout = torch.randn(5, 1, device="cuda", dtype=torch.bfloat16)
    y = lin(x)
    assert "LinearOut1" not in _grad_fn_name(y)
    got = (y,) + torch.autograd.grad(y, (x, lin.weight, lin.bias), gout)
    xr = x.detach().clone().requires_grad_(True)
    yr = torch.nn.functional.linear(xr, lin.weight, lin.bias)
    want = (yr,) + torch.autograd.grad(yr, (xr, lin.weight, lin.bias), gout)
    for a, r in zip(got, want):
        assert torch.equal(_bits(a.detach()), _bits(r.detach()))


@pytest.mark.gpu
@pytest.mark.parametrize("autocast", [False, True], ids=["plain", "autocast"])
def test_head_module_routes_and_matches_fp32(monkeypatch, autocast):
    from torchrec_amd.modules.mlp import LogitLinear

    monkeypatch.setenv("TREC_THIN_LAYERS", "1")
    (x, w, b, dy), ref = _head_case(33, 256)
    lin = LogitLinear(256, 1, device="cuda", dtype=torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    xin = (x.cuda() if autocast else x.to("cuda", torch.bfloat16)).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        y = lin(xin)
    assert _grad_fn_name(y) == "_LinearOut1Backward" and y.dtype == torch.bfloat16
    dx, dw, db = torch.autograd.grad(y, (xin, lin.weight, lin.bias), dy.to("cuda", y.dtype))
    _check("head.y", y, ref["y"], ref["y_abs"], 256)
    _check("head.dx", dx.bfloat16(), ref["dx"], ref["dx_abs"], 256)
    _check("head.dw", dw, ref["dw"], ref["dw_abs"], 33)
    _check("head.db", db, ref["db"], ref["db_abs"], 33)
    monkeypatch.setenv("TREC_THIN_LAYERS", "0")
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        assert "LinearOut1" not in _grad_fn_name(lin(xin))


def _arch_step(dense_arch, over_arch, xd, xo, gd, go):
    with torch.autocast("cuda", dtype=torch.bfloat16):
        yd = dense_arch(xd)
        yo = over_arch(xo)
    params = list(dense_arch.parameters()) + list(over_arch.parameters())
    grads = torch.autograd.grad((yd, yo), params + [xo], (gd, go))
    return (yd, yo) + grads


@pytest.mark.gpu
def test_graph_capture_replays_equal_eager_bitwise(monkeypatch):
    from torchrec_amd.models.dlrm import DenseArch, OverArch

    monkeypatch.setenv("TREC_THIN_LAYERS", "1")
    B = 70
    torch.manual_seed(9)
    dense_arch = DenseArch(13, [24, 8], device="cuda").to(torch.bfloat16)
    over_arch = OverArch(16, [16, 1], device="cuda").to(torch.bfloat16)
    bf = dict(device="cuda", dtype=torch.bfloat16)
    xd_s = torch.randn(B, 13, device="cuda")  # loader data: fp32, no grad
    xo_s = torch.randn(B, 16, requires_grad=True, **bf)
    gd_s, go_s = torch.randn(B, 8, **bf), torch.randn(B, 1, **bf)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert _grad_fn_name(over_arch(xo_s)) == "_LinearOut1Backward"

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            _arch_step(dense_arch, over_arch, xd_s, xo_s, gd_s, go_s)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = _arch_step(dense_arch, over_arch, xd_s, xo_s, gd_s, go_s)

    for seed in (11, 12):
        torch.manual_seed(seed)
        new = (torch.randn(B, 13, device="cuda"), torch.randn(B, 16, **bf),
               torch.randn(B, 8, **bf), torch.randn(B, 1, **bf))
        with torch.no_grad():
            for s, n in zip((xd_s, xo_s, gd_s, go_s), new):
                s.copy_(n)
        graph.replay()
        torch.cuda.synchronize()
        got = [o.detach().clone() for o in outs]
        want = _arch_step(dense_arch, over_arch, new[0], new[1].requires_grad_(True),
                          new[2], new[3])
        torch.cuda.synchronize()
        for i, (a, r) in enumerate(zip(got, want)):
            assert torch.equal(_bits(a), _bits(r.detach())), i


@pytest.mark.gpu
def test_switch_off_equals_plain_modules_bitwise(monkeypatch):
    """TREC_THIN_LAYERS=0: one DLRMTrain step equals, bit for bit, a model whose
    head is a plain nn.Linear."""
    import copy

    from torchrec_amd.datasets.random import Batch
    from torchrec_amd.models.dlrm import DLRM, DLRMTrain
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    monkeypatch.setenv("TREC_THIN_LAYERS", "0")
    device = torch.device("cuda:0")
    torch.manual_seed(0)
    keys, rows, B = ["f0", "f1"], [50, 70], 16
    ebc = EmbeddingBagCollection(
        tables=[
            EmbeddingBagConfig(num_embeddings=r, embedding_dim=16, name=f"t{i}",
                               feature_names=[keys[i]])
            for i, r in enumerate(rows)
        ]
    ).to(device)
    model = DLRMTrain(
        DLRM(embedding_bag_collection=ebc, dense_in_features=13,
             dense_arch_layer_sizes=[24, 16], over_arch_layer_sizes=[16, 1])
    ).to(device)
    plain = copy.deepcopy(model)
    head = plain.model.over_arch.model[1]
    lin = torch.nn.Linear(head.in_features, 1, device=device)
    lin.load_state_dict(head.state_dict())
    plain.model.over_arch.model[1] = lin
    assert type(plain.model.over_arch.model[1]) is torch.nn.Linear

    g = torch.Generator().manual_seed(1)
    batch = Batch(
        dense_features=torch.rand(B, 13, generator=g).to(device),
        sparse_features=KeyedJaggedTensor(
            keys=keys,
            values=torch.cat([torch.randint(0, r, (B,), generator=g) for r in rows]),
            lengths=torch.ones(2 * B, dtype=torch.int64),
            stride=B,
        ).to(device),
        labels=torch.randint(0, 2, (B,), generator=g).float().to(device),
    )

    def step(m):
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss, _ = m(batch)
        dense = [p for n, p in m.named_parameters() if "embedding_bag" not in n]
        return [loss] + list(torch.autograd.grad(loss, dense))

    for a, r in zip(step(model), step(plain)):
        assert torch.equal(_bits(a.detach()), _bits(r.detach()))
