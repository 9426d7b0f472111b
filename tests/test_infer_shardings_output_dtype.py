"""``output_dtype`` through the sharded quantized inference modules (gloo,
world 2, CPU lookups).

TW: a rank runs the unsharded module's arithmetic on whole tables and the
output all-to-all only moves the rounded values, so sharded == unsharded
exactly. RW: each rank rounds its partial pool to the output type, then the
reduce-scatter adds the W partials in that type. Every partial and every
running sum is at most ``S`` in magnitude (``S`` over the whole bag, as in
tests/test_quant_output_dtype.py), which gives at most ``W`` roundings of
``u * S``; the bound used is ``(W + 1) * u * S`` plus the fp32 term
``(n + 6) * 2^-24 * S * (1 + u)``.
"""

import pytest
import torch
import torch.distributed as dist

from tests.dist_utils import run_multi_process
from tests.test_infer_shardings_nbit import MIXED, UNIFORM, QuantSparseModel, make_nbit_tables
from tests.test_model_parallel import kjt_local_slice, make_global_kjt
from tests.test_quant_output_dtype import UNIT_ROUNDOFF, pooled_oracle
from torchrec_amd.distributed.model_parallel import DistributedModelParallel
from torchrec_amd.distributed.planner.planners import EmbeddingShardingPlanner
from torchrec_amd.distributed.planner.types import ParameterConstraints, Topology
from torchrec_amd.distributed.quant_embeddingbag import (
    QuantEmbeddingBagCollectionSharder,
    ShardedQuantEmbeddingBagCollection,
)
from torchrec_amd.distributed.types import ShardingType
from torchrec_amd.modules.embedding_configs import DataType
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
from torchrec_amd.quant.embedding_modules import EmbeddingBagCollection as QuantEBC

TW = ShardingType.TABLE_WISE.value
RW = ShardingType.ROW_WISE.value
B = 4


def _sharded_lookup_dtypes(dmp):
    sharded = [m for m in dmp.modules() if isinstance(m, ShardedQuantEmbeddingBagCollection)]
    assert len(sharded) == 1
    return [
        qtbe.output_dtype for lookup in sharded[0]._lookups for qtbe in lookup._emb_modules
    ]


def _run_ebc(rank, world_size, sharding_type, from_float_kwargs, module_dtype, fused_params, want):
    """Shard a ``module_dtype`` quant EBC with ``fused_params``; the output and
    every local lookup must be ``want``."""
    tables = make_nbit_tables()
    torch.manual_seed(42)
    float_ebc = EmbeddingBagCollection(tables=make_nbit_tables())
    qebc_ref = QuantEBC.from_float(float_ebc, output_dtype=want, **from_float_kwargs)
    model = QuantSparseModel(
        QuantEBC.from_float(float_ebc, output_dtype=module_dtype, **from_float_kwargs)
    )
    planner = EmbeddingShardingPlanner(
        topology=Topology(world_size=world_size, compute_device="cpu", hbm_cap=1 << 40),
        constraints={
            cfg.name: ParameterConstraints(sharding_types=[sharding_type]) for cfg in tables
        },
    )
    sharder = QuantEmbeddingBagCollectionSharder(fused_params=fused_params)
    plan = planner.collective_plan(model, [sharder], dist.group.WORLD)
    dmp = DistributedModelParallel(model, plan=plan, sharders=[sharder], init_data_parallel=False)
    assert all(dt == want for dt in _sharded_lookup_dtypes(dmp))
    kjt_global = make_global_kjt(tables, B * world_size)
    kjt_local = kjt_local_slice(kjt_global, rank * B, (rank + 1) * B)
    vals = dmp(kjt_local).values()
    assert vals.dtype == want, f"rank {rank}: {vals.dtype}"
    ref = qebc_ref(kjt_global).values()
    assert ref.dtype == want and float(ref.float().abs().max()) > 0
    if sharding_type == TW:
        assert torch.equal(vals, ref[rank * B : (rank + 1) * B])
        return
    y, S, n = pooled_oracle(
        qebc_ref._tbe, kjt_global.values(), kjt_global.offsets(), None, False
    )
    sl = slice(rank * B, (rank + 1) * B)
    y, S, n = y[sl], S[sl], n[sl]
    u = UNIT_ROUNDOFF[want]
    tol = (world_size + 1) * u * S + (n + 6) * 2.0**-24 * S * (1 + u)
    err = (vals.double() - y).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"rank {rank} RW {want}: worst err/tol {worst:.4f}")
    assert (err <= tol).all(), f"rank {rank}: worst err/tol {worst}"
    assert (vals[n == 0] == 0).all()


@pytest.mark.parametrize("widths", [UNIFORM, MIXED], ids=["int4", "mixed"])
@pytest.mark.parametrize("sharding_type", [TW, RW])
def test_sharded_bf16(sharding_type, widths):
    run_multi_process(
        _run_ebc, 2, "gloo", sharding_type, widths, torch.bfloat16,
        {"output_dtype": "bf16"}, torch.bfloat16,
    )


@pytest.mark.parametrize("sharding_type", [TW, RW])
def test_sharded_inherits_module_dtype(sharding_type):
    """No ``output_dtype`` in fused_params: the unsharded module's is taken."""
    run_multi_process(
        _run_ebc, 2, "gloo", sharding_type, UNIFORM, torch.bfloat16, None, torch.bfloat16
    )


def test_fused_params_override_module_dtype():
    run_multi_process(
        _run_ebc, 2, "gloo", TW, UNIFORM, torch.bfloat16, {"output_dtype": "fp16"},
        torch.float16,
    )


def _run_no_shard_rank(rank, world_size):
    """Every table on rank 0: rank 1's zero-column placeholder is bf16 like its
    peer's pooled output, and both ranks get the unsharded values."""
    from torchrec_amd.distributed.types import (
        EmbeddingModuleShardingPlan,
        ParameterSharding,
        ShardingEnv,
    )

    tables = make_nbit_tables()
    torch.manual_seed(42)
    qebc = QuantEBC.from_float(
        EmbeddingBagCollection(tables=make_nbit_tables()), output_dtype=torch.bfloat16, **UNIFORM
    )
    plan = EmbeddingModuleShardingPlan(
        {
            t.name: ParameterSharding(sharding_type=TW, compute_kernel="quant", ranks=[0])
            for t in tables
        }
    )
    env = ShardingEnv.from_process_group(dist.group.WORLD)
    sharded = ShardedQuantEmbeddingBagCollection(qebc, plan, env)
    n_local = sum(len(lookup._emb_modules) for lookup in sharded._lookups)
    assert (n_local > 0) == (rank == 0)
    assert all(lookup._out_torch_dtype == torch.bfloat16 for lookup in sharded._lookups)
    kjt_global = make_global_kjt(tables, B * world_size)
    out = sharded(kjt_local_slice(kjt_global, rank * B, (rank + 1) * B))
    vals = (out.wait() if hasattr(out, "wait") else out).values()
    assert vals.dtype == torch.bfloat16
    assert torch.equal(vals, qebc(kjt_global).values()[rank * B : (rank + 1) * B])


def test_rank_without_shards_agrees_on_dtype():
    run_multi_process(_run_no_shard_rank, 2, "gloo")


def _run_ec(rank, world_size, sharding_type, module_dtype, fused_params, want):
    from torchrec_amd.distributed.quant_embedding import ShardedQuantEmbeddingCollection
    from torchrec_amd.distributed.types import (
        EmbeddingModuleShardingPlan,
        ParameterSharding,
        ShardingEnv,
    )
    from torchrec_amd.modules.embedding_configs import EmbeddingConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingCollection
    from torchrec_amd.quant.embedding_modules import EmbeddingCollection as QuantEC
    from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

    torch.manual_seed(0)
    tables = [
        EmbeddingConfig(num_embeddings=40, embedding_dim=8, name="t0", feature_names=["f0"]),
        EmbeddingConfig(num_embeddings=24, embedding_dim=8, name="t1", feature_names=["f1"]),
    ]
    float_ec = EmbeddingCollection(tables=tables)
    qec = QuantEC.from_float(float_ec, output_dtype=module_dtype, weight_dtype=DataType.INT4)
    qec_ref = QuantEC.from_float(float_ec, output_dtype=want, weight_dtype=DataType.INT4)
    tw = sharding_type == TW
    plan = EmbeddingModuleShardingPlan(
        {
            t.name: ParameterSharding(
                sharding_type=sharding_type,
                compute_kernel="quant",
                ranks=[i % world_size] if tw else list(range(world_size)),
            )
            for i, t in enumerate(tables)
        }
    )
    env = ShardingEnv.from_process_group(dist.group.WORLD)
    sharded = ShardedQuantEmbeddingCollection(qec, plan, env, fused_params=fused_params)
    for lookup in sharded._lookups:
        assert lookup._qtbe.output_dtype == want
    Bl = 3
    g = torch.Generator().manual_seed(5 + rank)
    lengths = torch.randint(0, 3, (2 * Bl,), generator=g)
    values = torch.cat([
        torch.randint(0, tables[i // Bl].num_embeddings, (int(l),), generator=g)
        for i, l in enumerate(lengths)
    ])
    kjt = KeyedJaggedTensor(keys=["f0", "f1"], values=values, lengths=lengths, stride=Bl)
    out = sharded(kjt)
    ref = qec_ref(kjt)
    assert sum(ref[k].values().numel() for k in ref) > 0
    for k in ("f0", "f1"):
        assert out[k].values().dtype == want
        # a row is looked up on one rank and only moved: exact under TW and RW
        assert torch.equal(out[k].values(), ref[k].values())
        assert torch.equal(out[k].lengths(), ref[k].lengths())


@pytest.mark.parametrize("sharding_type", [TW, RW])
def test_sharded_ec_bf16(sharding_type):
    run_multi_process(_run_ec, 2, "gloo", sharding_type, torch.bfloat16, None, torch.bfloat16)


def test_sharded_ec_fused_params_override():
    run_multi_process(
        _run_ec, 2, "gloo", TW, torch.bfloat16, {"output_dtype": "fp16"}, torch.float16
    )
