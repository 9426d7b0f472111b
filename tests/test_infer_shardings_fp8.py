"""Sharded FP8 and FP8-mixed quantized inference (gloo, world 2, CPU).

Sharded and unsharded modules dequantise the same packed bytes, so they agree
to the tolerance of tests/test_infer_shardings_nbit.py, whose EBC worker and
tables are reused as they are."""

import pytest
import torch
import torch.distributed as dist

from tests.dist_utils import run_multi_process
from tests.test_infer_shardings_nbit import TW_RW, _run_quant_shard_test
from torchrec_amd.modules.embedding_configs import DataType
from torchrec_amd.distributed.types import ShardingType

UNIFORM_FP8 = {"weight_dtype": DataType.FP8}
MIXED_FP8 = {
    "per_table_weight_dtype": {
        "t0": DataType.FP8,
        "t1": DataType.INT8,
        "t2": DataType.INT2,
        "t3": DataType.INT4,
    }
}
EC_UNIFORM = {"t0": DataType.FP8, "t1": DataType.FP8, "t2": DataType.FP8, "t3": DataType.FP8}
EC_MIXED = {"t0": DataType.FP8, "t1": DataType.INT8, "t2": DataType.INT4, "t3": DataType.INT2}


@pytest.mark.parametrize("sharding_type", TW_RW)
def test_sharded_fp8_inference(sharding_type):
    run_multi_process(_run_quant_shard_test, 2, "gloo", sharding_type, UNIFORM_FP8)


@pytest.mark.parametrize("sharding_type", TW_RW)
def test_sharded_fp8_mixed_inference(sharding_type):
    run_multi_process(_run_quant_shard_test, 2, "gloo", sharding_type, MIXED_FP8)


def _run_quant_ec_fp8(rank, world_size, sharding_type, dtypes):
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
    rows = {"t0": 40, "t1": 24, "t2": 31, "t3": 17}
    tables = [
        EmbeddingConfig(num_embeddings=rows[n], embedding_dim=16, name=n, feature_names=[f"f{i}"])
        for i, n in enumerate(rows)
    ]
    qec = QuantEC.from_float(EmbeddingCollection(tables=tables), per_table_weight_dtype=dtypes)
    assert {c.name: c.data_type for c in qec.embedding_configs()} == dtypes
    tw = sharding_type == ShardingType.TABLE_WISE.value
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
    sharded = ShardedQuantEmbeddingCollection(qec, plan, env)
    served = {
        name: dt
        for lookup in sharded._lookups
        for (name, _, _), dt in zip(lookup._qtbe._specs, lookup._qtbe._weight_dtypes)
    }
    assert served and all(dtypes[name] is dt for name, dt in served.items())
    B = 3
    keys = [t.feature_names[0] for t in tables]
    g = torch.Generator().manual_seed(5 + rank)
    lengths = torch.randint(0, 3, (len(keys) * B,), generator=g)
    values = torch.cat([
        torch.randint(0, tables[i // B].num_embeddings, (int(l),), generator=g)
        for i, l in enumerate(lengths)
    ])
    kjt = KeyedJaggedTensor(keys=keys, values=values, lengths=lengths, stride=B)
    out = sharded(kjt)
    ref = qec(kjt)
    assert sum(ref[k].values().abs().sum() for k in keys) > 0
    for k in keys:
        torch.testing.assert_close(out[k].values(), ref[k].values(), atol=1e-5, rtol=1e-5)
        assert torch.equal(out[k].lengths(), ref[k].lengths())


@pytest.mark.parametrize("dtypes", [EC_UNIFORM, EC_MIXED], ids=["uniform", "mixed"])
@pytest.mark.parametrize("sharding_type", TW_RW)
def test_sharded_fp8_ec(sharding_type, dtypes):
    run_multi_process(_run_quant_ec_fp8, 2, "gloo", sharding_type, dtypes)
