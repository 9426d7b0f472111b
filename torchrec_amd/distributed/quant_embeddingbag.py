"""Sharded quantized EBC for multi-GPU inference.

Reference parity: torchrec/distributed/quant_embeddingbag.py
(ShardedQuantEmbeddingBagCollection) and the infer shardings
(tw_sharding.py:543 InferTwEmbeddingSharding): the training dists are reused
(one process per GPU over RCCL/xGMI); lookups run the quantized TBE at each
table's own format (INT8/INT4/INT2/FP8).
"""

from __future__ import annotations

from typing import Any, Dict, Iterable, List, Optional, Tuple, Type

import torch

from torchrec_amd.distributed.embeddingbag import (
    EmbeddingBagCollectionSharder,
    ShardedEmbeddingBagCollection,
)
from torchrec_amd.distributed.types import (
    EmbeddingModuleShardingPlan,
    ModuleSharder,
    ShardingEnv,
    ShardingType,
)
from torchrec_amd.quant.embedding_modules import (
    EmbeddingBagCollection as QuantEmbeddingBagCollection,
    QuantTableBatchedEmbeddingBags,
    check_delta_tables,
    int8_row_stride,
    update_tbe_from_delta,
)


_OUT_DTYPE_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}


def with_module_output_dtype(
    fused_params: Optional[Dict[str, Any]], module: Any
) -> Dict[str, Any]:
    """``fused_params`` with the unsharded quant module's ``output_dtype`` where
    the caller named none: sharding a bf16 module gives a bf16 sharded module."""
    fused_params = dict(fused_params or {})
    if "output_dtype" not in fused_params:
        fused_params["output_dtype"] = _OUT_DTYPE_NAME[module.output_dtype()]
    return fused_params


def with_module_bounds_check(
    fused_params: Optional[Dict[str, Any]], module: Any, kind: str
) -> Dict[str, Any]:
    """``fused_params`` with ``bounds_check`` defaulting to the unsharded quant
    module's setting: the local quant TBEs of a checked module are built
    checked, so a local id past a shard's rows is dropped and counted on the
    rank that holds the shard. Pruned tables are not sharded yet."""
    pruned = [
        name
        for (name, _, _), ro in zip(module._tbe._specs, getattr(module._tbe, "_remap_offsets_t", []))
        if int(ro) >= 0
    ]
    if pruned:
        raise NotImplementedError(
            f"sharding a quant {kind} with pruned tables (index_remapping on {pruned}) "
            f"is not supported yet"
        )
    fused_params = dict(fused_params or {})
    if "bounds_check" not in fused_params:
        fused_params["bounds_check"] = bool(module._tbe._checked)
    return fused_params


def apply_delta_to_shards(
    shards: Iterable[Tuple[QuantTableBatchedEmbeddingBags, List[Tuple[int, int]]]],
    delta: Dict[str, Any],
    device: torch.device,
) -> Dict[str, torch.Tensor]:
    """``update_rows`` on each local quant TBE with its tables' global row
    windows; table name -> entries applied on this rank, for every table of
    ``delta`` (0 for one this rank holds no rows of)."""
    applied = {name: torch.zeros((), dtype=torch.int64, device=device) for name in delta}
    for qtbe, windows in shards:
        for name, n in update_tbe_from_delta(qtbe, delta, windows).items():
            applied[name] = applied[name] + n.to(device)
    return applied


class ShardedQuantEmbeddingBagCollection(ShardedEmbeddingBagCollection):
    """Shards a quantized EBC; packed rows (any width: the slice is by whole
    rows at the table's own stride) are sliced per shard."""

    def __init__(
        self,
        module: QuantEmbeddingBagCollection,
        table_name_to_parameter_sharding: EmbeddingModuleShardingPlan,
        env: ShardingEnv,
        fused_params: Optional[Dict[str, Any]] = None,
        device: Optional[torch.device] = None,
    ) -> None:
        fused_params = with_module_output_dtype(fused_params, module)
        fused_params = with_module_bounds_check(fused_params, module, "EBC")
        super().__init__(module, table_name_to_parameter_sharding, env, fused_params, device)
        # load packed rows into the quant lookups (TW: whole table; RW: row slice)
        src = module._tbe
        by_name = {s[0]: i for i, s in enumerate(src._specs)}
        for lookup in self._lookups:
            for group, qtbe in zip(lookup._grouped_tables, lookup._emb_modules):
                for ti, t in enumerate(group):
                    packed = src.packed_table(by_name[t.name])
                    shard = packed[t.row_offset : t.row_offset + t.local_rows]
                    dst = qtbe.packed_table(ti)
                    dst.copy_(shard.to(dst.device))
        self._quant_table_names = [s[0] for s in src._specs]

    def update_embeddings(self, delta: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        """Apply a model delta (table name -> ``UniqueRows`` or ``(ids, rows)``,
        GLOBAL ids) to this rank's shards. Every rank passes the same delta:
        each local quant TBE takes its shard's own global row range as the
        window (TW: ``[0, rows)`` on the owner, the other ranks do not hold the
        table; RW: ``[row_offset, row_offset + local_rows)``) and drops the
        rest on the device, so there is no collective and no host-side
        filtering. Returns table name -> entries applied on THIS rank (0 where
        the rows live elsewhere)."""
        check_delta_tables(delta, self._quant_table_names, "this sharded quant EBC")
        return apply_delta_to_shards(
            (
                (qtbe, [(t.row_offset, t.row_offset + t.local_rows) for t in group])
                for lookup in self._lookups
                for group, qtbe in zip(lookup._grouped_tables, lookup._emb_modules)
            ),
            delta,
            self._device,
        )

    def forward(self, features):  # inference: no autograd
        with torch.no_grad():
            return super().forward(features)


class QuantEmbeddingBagCollectionSharder(ModuleSharder[QuantEmbeddingBagCollection]):
    def __init__(self, fused_params: Optional[Dict[str, Any]] = None) -> None:
        self._fused_params = fused_params or {}

    def shard(
        self,
        module: QuantEmbeddingBagCollection,
        params: EmbeddingModuleShardingPlan,
        env: ShardingEnv,
        device: Optional[torch.device] = None,
    ) -> ShardedQuantEmbeddingBagCollection:
        return ShardedQuantEmbeddingBagCollection(
            module, params, env, fused_params=self._fused_params, device=device
        )

    @property
    def module_type(self) -> Type[QuantEmbeddingBagCollection]:
        return QuantEmbeddingBagCollection

    def sharding_types(self, compute_device_type: str):
        # CW would split packed rows mid-scale; TW/RW keep rows whole
        return [ShardingType.TABLE_WISE.value, ShardingType.ROW_WISE.value]

    def compute_kernels(self, sharding_type: str, compute_device_type: str):
        return ["quant"]
