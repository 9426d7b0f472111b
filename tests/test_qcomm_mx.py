"""MXFP8 / MXFP4 qcomm wire: the plain-PyTorch reference against a float64
error bound, the wire layout, the pooled a2a over gloo, and the HIP codec
kernels (flat and slab addressing) byte for byte against the reference."""

import os

import pytest
import torch
import torch.distributed as dist

from tests.dist_utils import run_multi_process
from torchrec_amd import ops
from torchrec_amd.distributed import comm_ops
from torchrec_amd.distributed.qcomm_codecs import CommType, QCommsConfig, QuantizedCommCodec

FMTS = ["mxfp8", "mxfp4"]
# fmt -> (elem_max, mantissa bits m, emin, code bytes per group)
SPEC = {"mxfp8": (448.0, 3, -6, 32), "mxfp4": (6.0, 1, 0, 16)}
SPECIAL = 8  # groups 0..7 of _inputs are the hand-made ones


def _inputs(n_groups, fmt):
    """[n_groups * 32] fp32: magnitudes from 1e-30 to 1e30 (across and inside
    groups), then the special groups written over the first ones."""
    g = torch.Generator().manual_seed(n_groups)
    n = max(n_groups, SPECIAL)
    x = torch.randn(n, 32, generator=g) * torch.logspace(-30, 30, n).unsqueeze(1)
    x[n // 2 :: 7, ::3] *= 1e-12  # mixed magnitudes inside a group
    elem_max = SPEC[fmt][0]
    top = torch.tensor(elem_max * 2.0**5)
    x[0] = torch.linspace(-0.9, 1, 32) * top  # amax exactly elem_max * 2^5
    x[1] = x[0]
    x[1, 31] = torch.nextafter(top, torch.tensor(float("inf")))  # one ulp above
    x[2] = 0.0  # all zero
    x[3] = 1.0
    x[3, 5] = float("inf")
    x[4] = -1e-9  # negatives that round to zero next to amax 1
    x[4, 0] = 1.0
    x[5] = 3e-40  # subnormal amax: E clamps to -127
    x[6, 9] = float("nan")
    x[7] = -x[0]
    return x[:n_groups].reshape(-1)


@pytest.mark.parametrize("fmt", FMTS)
def test_reference_obeys_float64_bound(fmt):
    elem_max, m, emin, cb = SPEC[fmt]
    codec = QuantizedCommCodec(CommType(fmt))
    x = _inputs(64, fmt)
    wire = codec.encode(x)
    dec = codec.decode(wire, x.numel()).reshape(64, 32)
    sb = wire.view(torch.uint8).reshape(64, cb + 1)[:, cb].to(torch.int64)
    assert sb[0] == 127 + 5 and sb[1] == 127 + 6 and sb[7] == 127 + 5 and sb[5] == 0
    assert not wire.reshape(64, cb + 1)[2].any()  # zero group: scale 0, codes 0
    assert sb[3] == 255 and sb[6] == 255 and dec[3].isnan().all() and dec[6].isnan().all()
    assert (torch.signbit(dec[4, 1:]) & (dec[4, 1:] == 0)).all()  # -0.0: sign kept
    fin = sb != 255
    xd, dd = x.reshape(64, 32).double()[fin], dec.double()[fin]
    s = torch.pow(2.0, (sb[fin] - 127).double()).unsqueeze(1)
    bound = torch.maximum(2.0 ** -(m + 1) * xd.abs(), 2.0 ** (emin - m - 1) * s)
    assert ((dd - xd).abs() <= bound).all()
    ratio = xd.abs().amax(dim=1, keepdim=True) / s
    assert (ratio <= elem_max).all()
    unclamped = (sb[fin] > 0).unsqueeze(1)  # E = -127 is the clamp, not the smallest E
    assert (ratio[unclamped] > elem_max / 2).all()


@pytest.mark.parametrize("fmt", FMTS)
def test_wire_layout(fmt):
    _, _, _, cb = SPEC[fmt]
    codec = QuantizedCommCodec(CommType(fmt))
    grid = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])  # e2m1 values, amax 6
    a = torch.cat([grid, -grid, grid.flip(0), -grid.flip(0)])
    b = torch.randn(96)
    wa = codec.encode(a).view(torch.uint8)
    assert wa.numel() == codec.encoded_numel(32) == cb + 1
    assert codec.encoded_numel(5 * 32) == 5 * (cb + 1)
    code = torch.arange(8, dtype=torch.uint8)
    nib = torch.cat([code, code | 8, code.flip(0), code.flip(0) | 8])
    if fmt == "mxfp4":  # E = 0: the codes are the grid indices, low nibble first
        assert torch.equal(wa[:16], nib[0::2] | (nib[1::2] << 4)) and wa[16] == 127
    else:  # E = 2 - 8: element i is the e4m3 byte of a_i * 64, in byte i
        assert torch.equal(wa[:32], (a * 64).to(torch.float8_e4m3fn).view(torch.uint8))
        assert wa[32] == 127 - 6
    assert torch.equal(codec.encode(torch.cat([a, b])), torch.cat([codec.encode(a), codec.encode(b)]))
    with pytest.raises(ValueError, match="multiple of 32"):
        comm_ops.alltoall_pooled(torch.zeros(2, 48), [48], None, codec=codec)


def _run_tw_forward(rank, world_size, fmt):
    from tests.test_model_parallel import LR, SparseModel, _golden, kjt_local_slice, make_global_kjt
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.planner.planners import EmbeddingShardingPlanner
    from torchrec_amd.distributed.planner.types import ParameterConstraints, Topology
    from torchrec_amd.distributed.types import ShardingType
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig

    B = 4
    tables = [
        EmbeddingBagConfig(num_embeddings=20, embedding_dim=32, name="t0", feature_names=["f0"]),
        EmbeddingBagConfig(num_embeddings=30, embedding_dim=64, name="t1", feature_names=["f1"]),
    ]
    torch.manual_seed(42)
    model = SparseModel(list(tables))
    planner = EmbeddingShardingPlanner(
        topology=Topology(world_size=world_size, compute_device="cpu", hbm_cap=1 << 40),
        constraints={
            cfg.name: ParameterConstraints(sharding_types=[ShardingType.TABLE_WISE.value])
            for cfg in tables
        },
    )
    sharder = EmbeddingBagCollectionSharder(
        fused_params={
            "optimizer": "rowwise_adagrad",
            "learning_rate": LR,
            "qcomms_config": QCommsConfig(forward_precision=CommType(fmt)),
        }
    )
    plan = planner.collective_plan(model, [sharder], dist.group.WORLD)
    dmp = DistributedModelParallel(model, plan=plan, sharders=[sharder], init_data_parallel=False)
    golden = _golden(tables, None, world_size)
    dmp.load_state_dict(
        {
            f"sparse.embedding_bags.{cfg.name}.weight": w
            for cfg, w in zip(tables, golden.split_embedding_weights())
        },
        strict=False,
    )
    kjt_global = make_global_kjt(tables, B * world_size)
    vals = dmp(kjt_local_slice(kjt_global, rank * B, (rank + 1) * B)).values()
    expected = golden(kjt_global).values()[rank * B : (rank + 1) * B]
    # per element 2^-(m+1) * (amax of its group) <= 2^-(m+1) * max|expected|,
    # plus 2^-20 relative for the fp32 pooling order
    tol = (2.0 ** -(SPEC[fmt][1] + 1) + 2.0**-20) * float(expected.abs().max())
    assert float((vals - expected).abs().max()) <= tol


@pytest.mark.parametrize("fmt", FMTS)
def test_tw_forward_two_ranks(fmt):
    run_multi_process(_run_tw_forward, 2, "gloo", fmt)


def _run_a2a_backward(rank, world_size, fmt):
    B, dims = 3, [32, 64]
    codec = QuantizedCommCodec(CommType(fmt))
    g = torch.Generator().manual_seed(rank)
    x = torch.randn(world_size * B, dims[rank], generator=g)
    gout = torch.randn(B, sum(dims), generator=g) * 100.0
    grads = []
    for c in (codec, None):
        xin = x.clone().requires_grad_(True)
        out = comm_ops.alltoall_pooled(xin, dims, dist.group.WORLD, codec=c).wait()
        (out * gout).sum().backward()
        grads.append(xin.grad)
    assert comm_ops.get_gradient_division()
    blocks = grads[1] * world_size  # what the uncompressed a2a delivered
    rt = codec.decode(codec.encode(blocks.reshape(-1)), blocks.numel()).view_as(blocks)
    assert torch.equal(grads[0], rt / world_size)
    assert not torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("fmt", FMTS)
def test_a2a_backward_two_ranks(fmt):
    run_multi_process(_run_a2a_backward, 2, "gloo", fmt)


T = ops.QCOMM_MX_TILE_GROUPS


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("n_groups", [1, T - 1, T, T + 1, 3 * T + 5])
def test_hip_flat_equals_reference(fmt, n_groups):
    x = _inputs(n_groups, fmt)
    wire = ops.qcomm_mx_encode(x, fmt)
    dev_wire = ops.qcomm_mx_encode(x.cuda(), fmt)
    assert torch.equal(dev_wire.cpu(), wire)
    dec = ops.qcomm_mx_decode(wire, x.numel(), fmt)
    dev_dec = ops.qcomm_mx_decode(dev_wire, x.numel(), fmt).cpu()
    assert torch.equal(dev_dec.view(torch.int32), dec.view(torch.int32))  # NaN and -0.0 too


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize(
    "B,dims",
    [(b, d) for b in (1, 5) for d in ([32], [32, 96, 64], [160, 32])]
    # 6 groups a row, 18 T / 16 groups: the first tile runs through row ends
    # and all three blocks, the second starts inside the last block
    + [(3 * T // 16, [96, 32, 64])],
)
def test_hip_slab_equals_reference(fmt, B, dims):
    mat = _inputs(B * sum(dims) // 32, fmt).view(B, sum(dims))
    wire = ops.qcomm_mx_encode(mat, fmt, block_dims=dims)
    dev_wire = ops.qcomm_mx_encode(mat.cuda(), fmt, block_dims=dims)
    assert torch.equal(dev_wire.cpu(), wire)
    dec = ops.qcomm_mx_decode(wire, mat.numel(), fmt, block_dims=dims, B=B)
    # decode into NaN-filled memory: every element must be written
    poison = torch.full((B, sum(dims)), float("nan"), device="cuda")
    dev_dec = ops.qcomm_mx_decode(dev_wire, mat.numel(), fmt, block_dims=dims, B=B, out=poison).cpu()
    assert torch.equal(dev_dec.view(torch.int32), dec.view(torch.int32))


@pytest.mark.gpu
def test_alltoall_pooled_one_gpu_mxfp8():
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29573")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
    pg = dist.group.WORLD if dist.get_backend() == "nccl" else dist.new_group(backend="nccl")
    codec = QuantizedCommCodec(CommType.MXFP8)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(5, 96, generator=g) * 1e3
    gout = torch.randn(5, 96, generator=g) * 1e-3
    xin = x.cuda().requires_grad_(True)
    out = comm_ops.alltoall_pooled(xin, [96], pg, codec=codec).wait()
    (out * gout.cuda()).sum().backward()
    assert torch.equal(out.detach().cpu(), codec.decode(codec.encode(x.reshape(-1)), x.numel()).view(5, 96))
    rt = codec.decode(codec.encode(gout.reshape(-1)), gout.numel()).view(5, 96)
    assert torch.equal(xin.grad.cpu(), rt)
