"""Training delta -> served quantized model (CPU): after ``apply_model_delta``
of the tracker's ``UniqueRows`` the served ``qweights`` equal, byte for byte,
those of a model freshly quantised from the trained float model. Untouched
rows did not change on either side and a touched row requantises through the
table's own quantiser, so the equality is exact.

The tracker records a row as it is LOOKED UP (a forward pre-hook, so before
that batch's optimizer update). After the two optimizer steps the float model
therefore serves one more, evaluation-only, batch over the touched ids: in
``UpdateMode.LAST`` that is the row the delta carries, and it is current."""

import torch

from tests.dist_utils import run_multi_process
from torchrec_amd.modules.embedding_configs import DataType, EmbeddingBagConfig
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

TABLES = [("t0", 50, 8, DataType.INT8), ("t1", 30, 16, DataType.INT4), ("t2", 20, 12, DataType.FP8)]
FORMATS = {n: dt for n, _, _, dt in TABLES}
# ids looked up by the two training batches (per table); the rest stays untouched
BATCHES = [
    {"t0": [3, 7, 3, 49], "t1": [0, 29], "t2": [5]},
    {"t0": [7, 11], "t1": [29, 4, 4], "t2": [19, 0]},
]


def make_tables():
    return [
        EmbeddingBagConfig(num_embeddings=r, embedding_dim=d, name=n, feature_names=[f"f_{n}"])
        for n, r, d, _ in TABLES
    ]


class SparseModel(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.sparse = EmbeddingBagCollection(tables=make_tables())

    def forward(self, kjt):
        return self.sparse(kjt)


def one_bag_kjt(ids_by_table):
    values = [torch.tensor(ids_by_table[n]) for n, _, _, _ in TABLES]
    return KeyedJaggedTensor(
        keys=[f"f_{n}" for n, _, _, _ in TABLES],
        values=torch.cat(values),
        lengths=torch.tensor([v.numel() for v in values]),
        stride=1,
    )


def _run(rank, world_size):
    from torchrec_amd.distributed.embeddingbag import EmbeddingBagCollectionSharder
    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.model_tracker import ModelDeltaTracker, UpdateMode
    from torchrec_amd.distributed.planner.planners import EmbeddingShardingPlanner
    from torchrec_amd.distributed.planner.types import Topology
    from torchrec_amd.inference import apply_model_delta, quantize_inference_model

    torch.manual_seed(3)
    model = SparseModel()
    sharder = EmbeddingBagCollectionSharder(fused_params={"learning_rate": 0.5})
    planner = EmbeddingShardingPlanner(
        topology=Topology(world_size=1, compute_device="cpu", hbm_cap=1 << 40)
    )
    dmp = DistributedModelParallel(
        model, plan=planner.plan(model, [sharder]), sharders=[sharder], init_data_parallel=False
    )
    (sharded,) = dmp.sharded_modules().values()

    def quantized_copy():
        """The float model as it stands (sharding initialises the tables
        anew, so the weights are read back from it), quantised for serving."""
        current = {
            spec.name: w.detach().clone()
            for tbe in sharded.tbes()
            for spec, w in zip(tbe.embedding_specs, tbe.split_embedding_weights())
        }
        float_copy = SparseModel()
        for n, _, _, _ in TABLES:
            float_copy.sparse.embedding_bags[n].weight.data.copy_(current[n])
        return quantize_inference_model(float_copy, per_table_weight_dtype=FORMATS)

    served = quantized_copy()
    served_before = served.sparse._tbe.qweights.clone()
    tracker = ModelDeltaTracker(dmp, mode=UpdateMode.LAST)
    g = torch.Generator().manual_seed(8)
    for batch in BATCHES:  # two optimizer steps (the optimizer is fused into backward)
        out = dmp(one_bag_kjt(batch)).values()
        (out * torch.randn(out.shape, generator=g)).sum().backward()
        tracker.step()
    touched = {n: sorted({i for b in BATCHES for i in b[n]}) for n, _, _, _ in TABLES}
    with torch.no_grad():
        dmp(one_bag_kjt(touched))

    delta = tracker.get_unique()
    assert {n: u.ids.tolist() for n, u in delta.items()} == touched
    applied = apply_model_delta(served, delta)
    assert {n: int(c) for n, c in applied.items()} == {n: len(i) for n, i in touched.items()}

    fresh = quantized_copy()  # freshly quantised from the trained float weights
    assert torch.equal(served.sparse._tbe.qweights, fresh.sparse._tbe.qweights)
    assert not torch.equal(served.sparse._tbe.qweights, served_before)


def test_apply_model_delta_matches_fresh_quantisation():
    run_multi_process(_run, 1, "gloo")
