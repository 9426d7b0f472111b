"""Two-tower retrieval model (BASELINE config #5).

Reference analogue: torchrec examples' two-tower retrieval (query tower +
candidate tower over EmbeddingBagCollections, dot-product scoring); the
sequence variant consumes an EmbeddingCollection history. TwoTowerRetrieval
is the serving side: the query tower, an exhaustive top-k search of a
FlatIndex of candidate embeddings, and the candidate tower on the hits.
Serves as the flagship for the sequence-embedding + int8-quantized-inference
path.
"""

from __future__ import annotations

import dataclasses
from typing import Dict, Iterable, List, Optional, Tuple, Union

import torch
import torch.nn as nn

from torchrec_amd.modules.embedding_modules import (
    EmbeddingBagCollection,
    EmbeddingCollection,
)
from torchrec_amd.modules.knn_index import FlatIndex, IVFFlatIndex
from torchrec_amd.modules.mlp import MLP
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

KnnIndex = Union[FlatIndex, IVFFlatIndex]


class TwoTower(nn.Module):
    """Query/candidate towers over one EBC; returns (query_emb, cand_emb)."""

    def __init__(
        self,
        embedding_bag_collection: EmbeddingBagCollection,
        query_features: List[str],
        candidate_features: List[str],
        layer_sizes: List[int],
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__()
        self.ebc = embedding_bag_collection
        self._query_features = query_features
        self._candidate_features = candidate_features
        dims = {
            f: cfg.embedding_dim
            for cfg in embedding_bag_collection.embedding_bag_configs()
            for f in cfg.feature_names
        }
        q_in = sum(dims[f] for f in query_features)
        c_in = sum(dims[f] for f in candidate_features)
        self.query_proj = MLP(q_in, layer_sizes, device=device)
        self.candidate_proj = MLP(c_in, layer_sizes, device=device)

    def forward(self, kjt: KeyedJaggedTensor) -> Tuple[torch.Tensor, torch.Tensor]:
        kt = self.ebc(kjt)
        q = torch.cat([kt[f] for f in self._query_features], dim=1)
        c = torch.cat([kt[f] for f in self._candidate_features], dim=1)
        return self.query_proj(q), self.candidate_proj(c)


class TwoTowerTrain(nn.Module):
    """In-batch-negatives training: logits = Q @ C^T, labels = diagonal."""

    def __init__(self, two_tower: TwoTower) -> None:
        super().__init__()
        self.two_tower = two_tower
        self.loss_fn = nn.CrossEntropyLoss()

    def forward(self, kjt: KeyedJaggedTensor) -> torch.Tensor:
        q, c = self.two_tower(kjt)
        logits = q @ c.t()
        labels = torch.arange(q.shape[0], device=q.device)
        return self.loss_fn(logits, labels)


def _tower_ebc(ebc: EmbeddingBagCollection, features: List[str]) -> EmbeddingBagCollection:
    """An EBC over the tables of ``ebc`` that serve ``features`` (and only
    those features of them). The tables are SHARED with ``ebc``, not copied:
    no second copy of a large item table, and further training of ``ebc``
    shows through."""
    tables = [
        dataclasses.replace(cfg, feature_names=[f for f in cfg.feature_names if f in features])
        for cfg in ebc.embedding_bag_configs()
        if any(f in features for f in cfg.feature_names)
    ]
    out = EmbeddingBagCollection(tables=tables, device=torch.device("meta"))  # no storage
    for cfg in tables:
        out.embedding_bags[cfg.name] = ebc.embedding_bags[cfg.name]
    out._device = ebc.device
    return out


def _tower_input(ebc: EmbeddingBagCollection, features: List[str], kjt: KeyedJaggedTensor):
    kt = ebc(kjt)
    return torch.cat([kt[f] for f in features], dim=1)


class TwoTowerRetrieval(nn.Module):
    """Serving side of TwoTower (reference: examples/retrieval
    TwoTowerRetrieval): embed the queries, take the k nearest items from a
    FlatIndex of candidate-tower outputs, and score them with the candidate
    tower. Returns ([B, k] logits, [B, k] item ids); slots the index could not
    fill (fewer than k items) carry id -1 and logit -inf."""

    def __init__(
        self,
        index: KnnIndex,
        query_ebc: EmbeddingBagCollection,
        candidate_ebc: EmbeddingBagCollection,
        query_features: List[str],
        candidate_features: List[str],
        layer_sizes: List[int],
        k: int,
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__()
        self.index = index
        self.query_ebc = query_ebc
        self.candidate_ebc = candidate_ebc
        self._query_features = query_features
        self._candidate_features = candidate_features
        self.k = k
        q_in = sum(c.embedding_dim for c in query_ebc.embedding_bag_configs() for _ in c.feature_names)
        c_in = sum(
            c.embedding_dim for c in candidate_ebc.embedding_bag_configs() for _ in c.feature_names
        )
        self.query_proj = MLP(q_in, layer_sizes, device=device)
        self.candidate_proj = MLP(c_in, layer_sizes, device=device)

    @classmethod
    def from_two_tower(cls, two_tower: TwoTower, index: KnnIndex, k: int) -> "TwoTowerRetrieval":
        """Split a trained TwoTower's single EBC into the two collections and
        take over its projections. Tables and projections are shared with
        ``two_tower``, not copied, so the towers follow further training; the
        index does not, and has to be rebuilt after it."""
        qf, cf = two_tower._query_features, two_tower._candidate_features
        layer_sizes = [p._out_size for p in two_tower.query_proj._mlp]
        device = next(two_tower.query_proj.parameters()).device
        m = cls(index, _tower_ebc(two_tower.ebc, qf), _tower_ebc(two_tower.ebc, cf), qf, cf,
                layer_sizes, k, device=device)
        m.query_proj, m.candidate_proj = two_tower.query_proj, two_tower.candidate_proj
        return m

    def forward(self, query_kjt: KeyedJaggedTensor) -> Tuple[torch.Tensor, torch.Tensor]:
        q = self.query_proj(_tower_input(self.query_ebc, self._query_features, query_kjt))
        B, k = q.shape[0], self.k
        _, ids = self.index.search(q, k)
        flat = ids.reshape(-1).clamp(min=0)
        nf = len(self._candidate_features)
        candidate_kjt = KeyedJaggedTensor(
            keys=self._candidate_features,
            values=flat.repeat(nf),
            lengths=torch.ones(nf * B * k, dtype=torch.int64, device=flat.device),
            stride=B * k,
            length_per_key=[B * k] * nf,
        )
        c = self.candidate_proj(
            _tower_input(self.candidate_ebc, self._candidate_features, candidate_kjt)
        )
        logits = (q.unsqueeze(1) * c.view(B, k, -1)).sum(dim=2)
        return logits.masked_fill(ids < 0, float("-inf")), ids


@torch.no_grad()
def build_candidate_index(
    two_tower: TwoTower, item_kjt_batches: Iterable[KeyedJaggedTensor], index: KnnIndex
) -> KnnIndex:
    """Run the candidate tower over batches of items (one id per row and
    candidate feature) and add the embeddings to ``index`` under the ids of the
    first candidate feature. An index that has to be trained and is not yet is
    trained on all of those embeddings first."""
    cf = two_tower._candidate_features
    ebc = _tower_ebc(two_tower.ebc, cf)
    embedded = (
        (two_tower.candidate_proj(_tower_input(ebc, cf, kjt)), kjt[cf[0]].values())
        for kjt in item_kjt_batches
    )
    if not getattr(index, "is_trained", True):
        embedded = list(embedded)
        index.train(torch.cat([emb for emb, _ in embedded]))
    for emb, ids in embedded:
        index.add(emb, ids=ids)
    return index


class SequenceTwoTower(nn.Module):
    """Query tower over a user's id-list history via EmbeddingCollection
    (sequence embeddings mean-pooled after per-id projection)."""

    def __init__(
        self,
        embedding_collection: EmbeddingCollection,
        history_feature: str,
        candidate_ebc: EmbeddingBagCollection,
        candidate_features: List[str],
        layer_sizes: List[int],
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__()
        self.ec = embedding_collection
        self.candidate_ebc = candidate_ebc
        self._history_feature = history_feature
        self._candidate_features = candidate_features
        D = embedding_collection.embedding_dim()
        c_in = sum(
            cfg.embedding_dim
            for cfg in candidate_ebc.embedding_bag_configs()
            for _ in cfg.feature_names
        )
        self.query_proj = MLP(D, layer_sizes, device=device)
        self.candidate_proj = MLP(c_in, layer_sizes, device=device)

    def forward(
        self, history: KeyedJaggedTensor, candidates: KeyedJaggedTensor
    ) -> Tuple[torch.Tensor, torch.Tensor]:
        seq = self.ec(history)  # Dict[str, JaggedTensor] of per-id rows
        jt = seq[self._history_feature]
        # mean over each user's history (segment mean via padded dense)
        from torchrec_amd import ops as _ops

        lengths = jt.lengths().clamp(min=1)
        sums = torch.zeros(
            lengths.numel(), jt.values().shape[1], device=jt.values().device
        )
        bag_ids = torch.repeat_interleave(
            torch.arange(lengths.numel(), device=jt.values().device),
            jt.lengths(),
            output_size=jt.values().shape[0],
        )
        sums.index_add_(0, bag_ids, jt.values())
        q = sums / lengths.unsqueeze(1).float()
        kt = self.candidate_ebc(candidates)
        c = torch.cat([kt[f] for f in self._candidate_features], dim=1)
        return self.query_proj(q), self.candidate_proj(c)
