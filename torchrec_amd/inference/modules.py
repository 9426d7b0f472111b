"""Inference build path: quantize + shard a trained model for serving.

Reference parity: torchrec/inference/modules.py (quantize_inference_model
:372, shard_quant_model :490, PredictFactory :189 / PredictModule :266).
"""

from __future__ import annotations

import abc
from typing import Any, Dict, List, Optional, Tuple, Type

import torch
import torch.nn as nn

from torchrec_amd.modules.embedding_configs import DataType
from torchrec_amd.modules.embedding_modules import (
    EmbeddingBagCollection as FloatEBC,
    EmbeddingCollection as FloatEC,
)
from torchrec_amd.quant.embedding_modules import (
    EmbeddingBagCollection as QuantEBC,
    EmbeddingCollection as QuantEC,
)


def quantize_inference_model(
    model: nn.Module,
    quantization_mapping: Optional[Dict[Type[nn.Module], Any]] = None,
    output_dtype: torch.dtype = torch.float32,
    weight_dtype: DataType = DataType.INT8,
    per_table_weight_dtype: Optional[Dict[str, DataType]] = None,
    bounds_check: bool = False,
    index_remapping: Optional[Dict[str, torch.Tensor]] = None,
) -> nn.Module:
    """Swap float embedding modules for rowwise-quantized ones in-place
    (reference inference/modules.py:372). Tables are packed at
    ``weight_dtype`` (INT8/INT4/INT2/FP8) unless ``per_table_weight_dtype``
    names another format for them.

    ``bounds_check`` makes every quantized module drop (and count) ids outside
    its tables instead of reading them; ``index_remapping`` (table name ->
    int32/int64 ``[num_embeddings]`` tensor of physical rows, -1 = pruned)
    serves the named tables pruned. Both are
    ``QuantTableBatchedEmbeddingBags``'s arguments, by table name."""
    mapping = quantization_mapping or {
        FloatEBC: QuantEBC,
        FloatEC: QuantEC,
    }
    # custom mappings only need the original from_float signature: an
    # argument is passed on only when it is set
    kwargs: Dict[str, Any] = {}
    if weight_dtype != DataType.INT8 or per_table_weight_dtype:
        kwargs.update(weight_dtype=weight_dtype, per_table_weight_dtype=per_table_weight_dtype)
    if bounds_check:
        kwargs["bounds_check"] = True
    if index_remapping:
        kwargs["index_remapping"] = index_remapping

    def _swap(parent: nn.Module) -> None:
        for name, child in list(parent.named_children()):
            qcls = mapping.get(type(child))
            if qcls is not None:
                q = qcls.from_float(child, output_dtype=output_dtype, **kwargs)
                setattr(parent, name, q)
            else:
                _swap(child)

    _swap(model)
    return model


def apply_model_delta(model: nn.Module, delta: Dict[str, Any]) -> Dict[str, torch.Tensor]:
    """Publish a training delta into a served model, in place.

    ``delta`` maps a table name to the model tracker's ``UniqueRows`` (
    ``ModelDeltaTracker.get_unique`` in ``UpdateMode.FIRST`` / ``LAST``) or to
    ``(ids, rows)`` with global row ids. Every quant EBC / EC in ``model``,
    sharded or not, requantises the rows of the tables it serves
    (``update_embeddings``); on a sharded model every rank passes the same
    delta and keeps its own rows. Returns table name -> entries applied on
    this rank (0 is fine: the rows may live on another rank). A table of
    ``delta`` that no module serves is an error, raised before anything is
    written. Lookups on other streams are not ordered against the update (see
    ``QuantTableBatchedEmbeddingBags.update_rows``)."""
    targets = []
    served: set = set()
    for m in model.modules():
        if not callable(getattr(m, "update_embeddings", None)):
            continue
        if isinstance(m, QuantEBC):
            names = [t.name for t in m.embedding_bag_configs()]
        elif isinstance(m, QuantEC):
            names = [t.name for t in m.embedding_configs()]
        else:
            names = getattr(m, "_quant_table_names", None)
            if names is None:
                continue
        targets.append((m, names))
        served.update(names)
    missing = [n for n in delta if n not in served]
    if missing:
        raise KeyError(
            f"apply_model_delta: no quantized module of the model serves {missing} "
            f"(served: {sorted(served)})"
        )
    applied: Dict[str, torch.Tensor] = {}
    for m, names in targets:
        part = {n: delta[n] for n in names if n in delta}
        if not part:
            continue
        for n, c in m.update_embeddings(part).items():
            applied[n] = applied[n] + c.to(applied[n].device) if n in applied else c
    return applied


def shard_quant_model(
    model: nn.Module,
    world_size: int = 1,
    compute_device: str = "cuda",
    sharding_device: str = "cuda",
    constraints: Optional[Dict[str, Any]] = None,
) -> Tuple[nn.Module, Any]:
    """Place the quantized model for serving (reference inference/modules.py:490).

    Single-host inference: world_size==1 moves the quantized modules onto the
    target device. Multi-GPU single-host sharding (TW + all_to_one over xGMI)
    is the next milestone; the plan object records the placement decisions.
    """
    device = torch.device(compute_device if compute_device != "cuda" else "cuda:0")
    if world_size == 1:
        model = model.to(device)
        plan = {"world_size": 1, "placement": str(device)}
        return model, plan
    # multi-rank serving: shard quant EBCs with the training dists (TW/RW)
    import torch.distributed as dist

    from torchrec_amd.distributed.model_parallel import DistributedModelParallel
    from torchrec_amd.distributed.planner.planners import EmbeddingShardingPlanner
    from torchrec_amd.distributed.planner.types import Topology
    from torchrec_amd.distributed.quant_embedding import (
        QuantEmbeddingCollectionSharder,
    )
    from torchrec_amd.distributed.quant_embeddingbag import (
        QuantEmbeddingBagCollectionSharder,
    )
    from torchrec_amd.distributed.types import ShardingEnv

    assert dist.is_initialized(), "multi-rank quant sharding needs torch.distributed"
    env = ShardingEnv.from_process_group(dist.group.WORLD)
    sharders = [QuantEmbeddingBagCollectionSharder(), QuantEmbeddingCollectionSharder()]
    planner = EmbeddingShardingPlanner(
        topology=Topology(
            world_size=world_size,
            compute_device=compute_device,
            hbm_cap=None if compute_device == "cuda" else 1 << 40,
        ),
        constraints=constraints,
    )
    plan = planner.collective_plan(model, sharders, dist.group.WORLD)
    dmp = DistributedModelParallel(
        model, env=env, plan=plan, sharders=sharders, device=device,
        init_data_parallel=False,
    )
    return dmp, plan


class PredictModule(nn.Module):
    """Serving wrapper contract (reference inference/modules.py:266):
    forward(batch dict) -> predictions dict."""

    def __init__(self, module: nn.Module) -> None:
        super().__init__()
        self._module = module
        self._module.eval()

    @property
    def predict_module(self) -> nn.Module:
        return self._module

    @abc.abstractmethod
    def predict_forward(self, batch: Dict[str, Any]) -> Any:
        ...

    def forward(self, batch: Dict[str, Any]) -> Any:
        with torch.inference_mode():
            return self.predict_forward(batch)


class PredictFactory(abc.ABC):
    """Packaging contract for serving artifacts (reference :189)."""

    @abc.abstractmethod
    def create_predict_module(self) -> nn.Module:
        ...

    def batching_metadata(self) -> Dict[str, str]:
        return {"float_features": "dense", "id_list_features": "sparse"}

    def result_metadata(self) -> str:
        return "dict_of_tensor"
