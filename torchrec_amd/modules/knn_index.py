"""Exhaustive nearest-neighbour index over ops.mips_topk.

Reference analogue: the FAISS index of examples/retrieval (knn_index.py,
TwoTowerRetrieval). The corpus is stored once, in bf16, in the layout the
kernel reads; a search is one fused score-and-select pass over it.
"""

from __future__ import annotations

from typing import Any, Dict, Optional, Tuple

import torch
import torch.nn as nn

from torchrec_amd import ops


class FlatIndex(nn.Module):
    """Flat (exact) index. ``metric="ip"`` searches by inner product, ``"l2"``
    by squared euclidean distance, as argmax of q.c - 0.5 * ||c||^2 on the same
    kernel. Equal distances come back in ascending row order.

    The bf16 corpus (rows padded to a multiple of 32 columns), the fp32 bias and
    the optional external-id map are buffers: the index follows ``.to()`` and
    saves with ``state_dict``.
    """

    def __init__(
        self,
        embedding_dim: int,
        metric: str = "ip",
        device: Optional[torch.device] = None,
        capacity: int = 0,
    ) -> None:
        super().__init__()
        if metric not in ("ip", "l2"):
            raise ValueError(f"FlatIndex: metric must be 'ip' or 'l2', got {metric!r}")
        if not 1 <= embedding_dim <= ops.MIPS_TOPK_MAX_D:
            raise ValueError(
                f"FlatIndex: embedding_dim {embedding_dim} is outside 1..{ops.MIPS_TOPK_MAX_D}"
            )
        self.embedding_dim = embedding_dim
        self.metric = metric
        self._padded_dim = (embedding_dim + 31) // 32 * 32
        self._n = 0
        self.register_buffer(
            "corpus", torch.zeros(capacity, self._padded_dim, dtype=torch.bfloat16, device=device)
        )
        self.register_buffer("bias", torch.zeros(capacity, dtype=torch.float32, device=device))
        # external ids; stays empty while every row's id is its row number
        self.register_buffer("ids", torch.zeros(0, dtype=torch.int64, device=device))

    def __len__(self) -> int:
        return self._n

    def reset(self) -> None:
        self._n = 0
        self.ids = self.ids[:0]

    def _reserve(self, n: int) -> None:
        cap = self.corpus.shape[0]
        if n <= cap:
            return
        new_cap = max(n, 2 * cap, 1024)
        for name in ("corpus", "bias") + (("ids",) if self.ids.numel() else ()):
            old = getattr(self, name)
            new = old.new_zeros((new_cap,) + tuple(old.shape[1:]))
            new[: self._n] = old[: self._n]
            setattr(self, name, new)

    @torch.no_grad()
    def add(self, embeddings: torch.Tensor, ids: Optional[torch.Tensor] = None) -> None:
        """Append rows [n, embedding_dim], rounded to bf16 once. ``ids`` are the
        item ids a search returns for them (default: the row number)."""
        if embeddings.dim() != 2 or embeddings.shape[1] != self.embedding_dim:
            raise ValueError(f"FlatIndex.add: expected [n, {self.embedding_dim}] embeddings")
        n0, n1 = self._n, self._n + embeddings.shape[0]
        dev = self.corpus.device
        self._reserve(n1)
        if ids is not None and self.ids.numel() == 0:
            # first external ids: earlier rows keep their row numbers
            self.ids = torch.arange(self.corpus.shape[0], dtype=torch.int64, device=dev)
        rows = embeddings.to(device=dev, dtype=torch.bfloat16)
        self.corpus[n0:n1, : self.embedding_dim] = rows
        if self.metric == "l2":
            self.bias[n0:n1] = -0.5 * rows.float().square().sum(dim=1)
        if self.ids.numel():
            self.ids[n0:n1] = (
                ids.to(device=dev, dtype=torch.int64).reshape(-1)
                if ids is not None
                else torch.arange(n0, n1, dtype=torch.int64, device=dev)
            )
        self._n = n1

    @torch.no_grad()
    def search(self, queries: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(distances [B, k], ids [B, k]): inner products, best first, for "ip";
        squared distances, ascending, for "l2". With fewer than k rows the tail
        is -inf (ip) / +inf (l2) and id -1."""
        if self._n == 0:
            raise RuntimeError("FlatIndex.search: the index is empty")
        n = self._n
        l2 = self.metric == "l2"
        scores, rows = ops.mips_topk(
            queries, self.corpus[:n], k, row_bias=self.bias[:n] if l2 else None
        )
        if l2:
            q_norm = queries.bfloat16().float().square().sum(dim=1, keepdim=True)
            scores = q_norm - 2.0 * scores
        if self.ids.numel():
            rows = torch.where(rows >= 0, self.ids[rows.clamp(min=0)], rows)
        return scores, rows

    # the row count and the buffers' sizes travel with the state dict
    def get_extra_state(self) -> Dict[str, Any]:
        return {"n": self._n}

    def set_extra_state(self, state: Dict[str, Any]) -> None:
        self._n = int(state["n"])

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs) -> None:
        for name in ("corpus", "bias", "ids"):
            src = state_dict.get(prefix + name)
            if src is not None and src.shape != getattr(self, name).shape:
                setattr(self, name, getattr(self, name).new_zeros(src.shape))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
