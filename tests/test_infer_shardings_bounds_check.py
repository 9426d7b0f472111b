"""``bounds_check`` on sharded quantized inference modules (gloo, world 2,
CPU; the harness of tests/test_infer_shardings_update.py): the local quant
TBEs are built checked, a local id past a shard's rows is dropped and counted
on the rank that holds the shard, and everything else equals the unsharded
checked module. A pruned table is not sharded.

Out-of-range ids: TW takes -1 and ``rows + 1`` on every table. RW buckets an
id by ``id // block``, so only an id whose bucket exists reaches a shard: id
31 of the 31-row table (block 16: rank 1, local row 15 of 15) and id 17 of
the 17-row table (block 9: rank 1, local row 8 of 8)."""

import pytest
import torch
import torch.distributed as dist

from tests.dist_utils import run_multi_process
from tests.test_infer_shardings_nbit import TW_RW, QuantSparseModel
from tests.test_infer_shardings_update import DTYPES, ROWS, D
from tests.test_model_parallel import kjt_local_slice
from torchrec_amd.distributed.types import ShardingType
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

B = 3


def out_of_range_ids(sharding_type):
    if sharding_type == ShardingType.TABLE_WISE.value:
        return {n: [-1, r + 1] for n, r in ROWS.items()}
    return {"t0": [], "t1": [], "t2": [31], "t3": [17]}


def make_kjt(world_size, sharding_type):
    """Per rank: sample 0 mixes valid and out-of-range ids, sample 1 holds
    only out-of-range ids (or nothing), sample 2 is valid."""
    g = torch.Generator().manual_seed(23)
    bad = out_of_range_ids(sharding_type)
    lengths, values = [], []
    for n, rows in ROWS.items():
        for b in range(B * world_size):
            valid = torch.randint(0, rows, (2,), generator=g)
            oob = torch.tensor(bad[n], dtype=torch.int64)
            v = [torch.cat([valid[:1], oob, valid[1:]]), oob, valid][b % B]
            lengths.append(v.numel())
            values.append(v)
    return KeyedJaggedTensor(
        keys=[f"f{i}" for i in range(len(ROWS))],
        values=torch.cat(values),
        lengths=torch.tensor(lengths),
        stride=B * world_size,
    )


def assert_counts(qtbes, world_size, sharding_type):
    """The local counters, summed per table over shards and ranks."""
    names = sorted(ROWS)
    total = torch.zeros(len(names), dtype=torch.int64)
    for qtbe in qtbes:
        assert qtbe._checked
        for (name, _, _), c in zip(qtbe._specs, qtbe.out_of_range_counts().tolist()):
            total[names.index(name)] += c
    dist.all_reduce(total)
    bad = out_of_range_ids(sharding_type)
    # every sample 0 and every sample 1 carries the table's out-of-range ids
    assert total.tolist() == [2 * world_size * len(bad[n]) for n in names]
    assert int(total.sum()) > 0


def _run_ebc(rank, world_size, sharding_type):
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.planner.planners import EmbeddingShardingPlanner
    from torchrec_amd.distributed.planner.types import ParameterConstraints, Topology
    from torchrec_amd.distributed.quant_embeddingbag import (
        QuantEmbeddingBagCollectionSharder,
        ShardedQuantEmbeddingBagCollection,
    )
    from torchrec_amd.distributed.types import ShardingEnv
    from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
    from torchrec_amd.quant.embedding_modules import EmbeddingBagCollection as QuantEBC

    torch.manual_seed(42)
    tables = [
        EmbeddingBagConfig(num_embeddings=r, embedding_dim=D, name=n, feature_names=[f"f{i}"])
        for i, (n, r) in enumerate(ROWS.items())
    ]
    float_ebc = EmbeddingBagCollection(tables=tables)
    ref = QuantEBC.from_float(float_ebc, per_table_weight_dtype=DTYPES, bounds_check=True)
    # the sharded module inherits the unsharded module's setting
    model = QuantSparseModel(
        QuantEBC.from_float(float_ebc, per_table_weight_dtype=DTYPES, bounds_check=True)
    )
    planner = EmbeddingShardingPlanner(
        topology=Topology(world_size=world_size, compute_device="cpu", hbm_cap=1 << 40),
        constraints={n: ParameterConstraints(sharding_types=[sharding_type]) for n in ROWS},
    )
    sharder = QuantEmbeddingBagCollectionSharder()
    plan = planner.collective_plan(model, [sharder], dist.group.WORLD)
    dmp = DistributedModelParallel(model, plan=plan, sharders=[sharder], init_data_parallel=False)
    sharded = dmp.module.sparse
    assert isinstance(sharded, ShardedQuantEmbeddingBagCollection)
    kjt_global = make_kjt(world_size, sharding_type)
    out = dmp(kjt_local_slice(kjt_global, rank * B, (rank + 1) * B)).values()
    want = ref(kjt_global).values()[rank * B : (rank + 1) * B]
    torch.testing.assert_close(out, want, atol=1e-5, rtol=1e-5)
    bad = out_of_range_ids(sharding_type)
    for i, n in enumerate(ROWS):
        if bad[n]:  # sample 1 holds only out-of-range ids: exactly zero
            assert int(out[1, i * D : (i + 1) * D].count_nonzero()) == 0
    assert float(out[2].abs().min()) > 0
    assert_counts(
        [q for lookup in sharded._lookups for q in lookup._emb_modules], world_size, sharding_type
    )

    # a pruned table is not sharded yet
    remap = torch.arange(ROWS["t1"])
    remap[3] = -1
    remap[4:] -= 1
    pruned = QuantEBC.from_float(float_ebc, index_remapping={"t1": remap})
    with pytest.raises(NotImplementedError, match="t1"):
        ShardedQuantEmbeddingBagCollection(
            pruned, plan.plan["sparse"], ShardingEnv.from_process_group(dist.group.WORLD)
        )


@pytest.mark.parametrize("sharding_type", TW_RW)
def test_sharded_ebc_bounds_check(sharding_type):
    run_multi_process(_run_ebc, 2, "gloo", sharding_type)


def _run_ec(rank, world_size, sharding_type):
    from torchrec_amd.distributed.quant_embedding import ShardedQuantEmbeddingCollection
    from torchrec_amd.distributed.types import (
        EmbeddingModuleShardingPlan,
        ParameterSharding,
        ShardingEnv,
    )
    from torchrec_amd.modules.embedding_configs import EmbeddingConfig
    from torchrec_amd.modules.embedding_modules import EmbeddingCollection
    from torchrec_amd.quant.embedding_modules import EmbeddingCollection as QuantEC

    torch.manual_seed(0)
    tables = [
        EmbeddingConfig(num_embeddings=r, embedding_dim=D, name=n, feature_names=[f"f{i}"])
        for i, (n, r) in enumerate(ROWS.items())
    ]
    float_ec = EmbeddingCollection(tables=tables)
    ref = QuantEC.from_float(float_ec, per_table_weight_dtype=DTYPES, bounds_check=True)
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
    # an unchecked module sharded with the fused parameter set
    src = QuantEC.from_float(float_ec, per_table_weight_dtype=DTYPES)
    assert not src._tbe._checked
    sharded = ShardedQuantEmbeddingCollection(src, plan, env, fused_params={"bounds_check": True})
    kjt_global = make_kjt(world_size, sharding_type)
    kjt = kjt_local_slice(kjt_global, rank * B, (rank + 1) * B)
    out, want = sharded(kjt), ref(kjt)
    bad = out_of_range_ids(sharding_type)
    for k, n in zip(kjt.keys(), ROWS):
        torch.testing.assert_close(out[k].values(), want[k].values(), atol=1e-5, rtol=1e-5)
        assert torch.equal(out[k].lengths(), want[k].lengths())
        rows = out[k].values()
        # sample 0 is [valid, out of range..., valid], sample 1 out of range only
        nb = len(bad[n])
        dropped = list(range(1, 1 + nb)) + list(range(2 + nb, 2 + 2 * nb))
        assert int(rows[dropped].count_nonzero()) == 0
        assert float(rows[0].abs().max()) > 0
    assert_counts([lookup._qtbe for lookup in sharded._lookups], world_size, sharding_type)

    remap = torch.arange(ROWS["t2"])
    remap[0] = -1
    remap[1:] -= 1
    pruned = QuantEC.from_float(float_ec, index_remapping={"t2": remap})
    with pytest.raises(NotImplementedError, match="t2"):
        ShardedQuantEmbeddingCollection(pruned, plan, env)


@pytest.mark.parametrize("sharding_type", TW_RW)
def test_sharded_ec_bounds_check(sharding_type):
    run_multi_process(_run_ec, 2, "gloo", sharding_type)
