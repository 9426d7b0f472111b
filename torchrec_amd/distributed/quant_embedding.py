"""Sharded quantized sequence EC for multi-GPU inference.

Reference parity: torchrec/distributed/quant_embedding.py
(ShardedQuantEmbeddingCollection) — the training sequence dists (feature a2a
in, per-row embedding a2a out) reused over the rowwise-quantized
(INT8/INT4/INT2/FP8 per table) sequence lookups."""

from __future__ import annotations

from typing import Any, Dict, List, Optional, Type

import torch
import torch.nn as nn

from torchrec_amd.distributed.embedding import ShardedEmbeddingCollection
from torchrec_amd.distributed.embedding_sharding import ShardedTableLocal
from torchrec_amd.distributed.quant_embeddingbag import (
    apply_delta_to_shards,
    with_module_bounds_check,
    with_module_output_dtype,
)
from torchrec_amd.distributed.types import (
    EmbeddingModuleShardingPlan,
    ModuleSharder,
    ShardingEnv,
    ShardingType,
)
from torchrec_amd.quant.embedding_modules import (
    EmbeddingCollection as QuantEmbeddingCollection,
    QuantTableBatchedEmbeddingBags,
    check_delta_tables,
    quant_data_type,
)


class _QuantSeqLookup(nn.Module):
    """Sequence (per-row) quantized lookup over a quant TBE group."""

    def __init__(self, qtbe: QuantTableBatchedEmbeddingBags, dim: int) -> None:
        super().__init__()
        self._qtbe = qtbe
        self._dim = dim

    def forward(self, indices: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
        qtbe = self._qtbe
        F = qtbe._num_features
        B = (offsets.numel() - 1) // max(F, 1)
        if qtbe.qweights.is_cuda or qtbe.qweights.is_pinned():
            feat_val_offsets = offsets[::B][: F + 1].contiguous()
            if feat_val_offsets.numel() < F + 1:
                feat_val_offsets = torch.cat([feat_val_offsets, offsets[-1:]])
            return qtbe.forward_sequence(indices, feat_val_offsets, self._dim)
        # CPU reference: dequantize rows per feature
        outs: List[torch.Tensor] = []
        for f in range(F):
            t = qtbe._feature_table_map[f]
            w = qtbe._cpu_lookup_table(t)
            lo, hi = int(offsets[f * B]), int(offsets[(f + 1) * B])
            idx = indices[lo:hi]
            if qtbe._checked:
                idx = qtbe._map_ids_cpu(t, idx)  # -1 indexes the appended zero row
            outs.append(w[idx])
        rows = (
            torch.cat(outs, dim=0)
            if outs
            else torch.zeros(0, self._dim, device=indices.device)
        )
        return qtbe.to_output_dtype(rows)


class ShardedQuantEmbeddingCollection(ShardedEmbeddingCollection):
    """TW / RW / DP sequence sharding of a quantized EC (inference)."""

    def __init__(
        self,
        module: QuantEmbeddingCollection,
        table_name_to_parameter_sharding: EmbeddingModuleShardingPlan,
        env: ShardingEnv,
        fused_params: Optional[Dict[str, Any]] = None,
        device: Optional[torch.device] = None,
    ) -> None:
        object.__setattr__(self, "_quant_device_pre", device)
        fused_params = with_module_output_dtype(fused_params, module)
        fused_params = with_module_bounds_check(fused_params, module, "EC")
        object.__setattr__(self, "_quant_bounds_check_pre", bool(fused_params["bounds_check"]))
        object.__setattr__(
            self,
            "_quant_out_dtype_pre",
            {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[
                fused_params["output_dtype"]
            ],
        )
        super().__init__(
            module, table_name_to_parameter_sharding, env, fused_params, device
        )
        # load packed rows into the local shards
        src = module._tbe
        by_name = {s[0]: i for i, s in enumerate(src._specs)}
        W = env.world_size
        for lookup in self._lookups:
            qtbe = lookup._qtbe
            # each table's global row range on this rank, from its REAL local
            # row count: a rank that owns no row of a table serves a one-row
            # placeholder, which an update must not touch
            lookup._row_windows = []
            for ti, (name, local_rows, dim) in enumerate(qtbe._specs):
                si = by_name[name]
                packed = src.packed_table(si)
                ps = table_name_to_parameter_sharding[name]
                if ps.sharding_type == ShardingType.ROW_WISE.value:
                    full = src._specs[si][1]
                    block = (full + W - 1) // W
                    lo = min(env.rank * block, full)
                else:
                    lo = 0
                shard = packed[lo : lo + local_rows]
                dst = qtbe.packed_table(ti)
                dst[: shard.shape[0]].copy_(shard.to(dst.device))
                lookup._row_windows.append((lo, lo + lookup._real_rows[ti]))
        self._quant_table_names = [s[0] for s in src._specs]

    def update_embeddings(self, delta: Dict[str, Any]) -> Dict[str, torch.Tensor]:
        """Apply a model delta (table name -> ``UniqueRows`` or ``(ids, rows)``,
        GLOBAL ids) to this rank's shards; every rank passes the same delta.
        The window of a local table is the shard's own global row range (TW:
        ``[0, rows)`` on the owner; RW: ``[lo, lo + local_rows)`` with ``lo =
        rank * ceil(rows / W)``), the rest is dropped on the device: no
        collective. Returns table name -> entries applied on THIS rank."""
        check_delta_tables(delta, self._quant_table_names, "this sharded quant EC")
        return apply_delta_to_shards(
            ((lookup._qtbe, lookup._row_windows) for lookup in self._lookups),
            delta,
            self._device,
        )

    def _make_lookup(
        self, tables: List[ShardedTableLocal], D: int, dense: bool = False
    ) -> nn.Module:
        qtbe = QuantTableBatchedEmbeddingBags(
            [(t.name, max(t.local_rows, 1), t.local_dim) for t in tables],
            feature_table_map=[i for i, t in enumerate(tables) for _ in t.feature_names],
            device=self._quant_device_pre,
            weight_dtypes=[quant_data_type(t.data_type) for t in tables],
            output_dtype=self._quant_out_dtype_pre,
            bounds_check=self._quant_bounds_check_pre,
        )
        lookup = _QuantSeqLookup(qtbe, D)
        lookup._real_rows = [t.local_rows for t in tables]
        return lookup

    def forward(self, features):
        with torch.no_grad():
            return super().forward(features)


class QuantEmbeddingCollectionSharder(ModuleSharder[QuantEmbeddingCollection]):
    def __init__(self, fused_params: Optional[Dict[str, Any]] = None) -> None:
        self._fused_params = fused_params or {}

    def shard(
        self,
        module: QuantEmbeddingCollection,
        params: EmbeddingModuleShardingPlan,
        env: ShardingEnv,
        device: Optional[torch.device] = None,
    ) -> ShardedQuantEmbeddingCollection:
        return ShardedQuantEmbeddingCollection(
            module, params, env, fused_params=self._fused_params, device=device
        )

    @property
    def module_type(self) -> Type[QuantEmbeddingCollection]:
        return QuantEmbeddingCollection

    def sharding_types(self, compute_device_type: str):
        return [ShardingType.TABLE_WISE.value, ShardingType.ROW_WISE.value]

    def compute_kernels(self, sharding_type: str, compute_device_type: str):
        return ["quant"]
