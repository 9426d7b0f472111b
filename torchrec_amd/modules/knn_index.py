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


class IVFFlatIndex(nn.Module):
    """Inverted-file index over bf16 rows (reference analogue: the IVF index of
    knn_index.py with its ``num_centroids`` / ``num_probe``, without the product
    quantisation). ``train`` places ``nlist`` centroids by k-means, ``add``
    files each row under its nearest centroid, and a search scores only the
    rows of the ``nprobe`` lists whose centroids are best for the query:
    ``ops.mips_topk`` over the centroids, then ``ops.ivf_topk`` over the lists.

    Metrics and the distances returned are those of ``FlatIndex``; equal
    distances come back in ascending storage order (lists in order, a list in
    insertion order). Rows are always filed by L2 distance to the centroids.
    Buffers: ``centroids`` / ``centroid_bias`` (bf16 padded rows and their
    -0.5 ||c||^2), ``corpus`` / ``bias`` / ``ids`` stored list by list, and
    ``list_offsets``.
    """

    _BUFFERS = ("centroids", "centroid_bias", "corpus", "bias", "list_offsets", "ids")

    def __init__(
        self,
        embedding_dim: int,
        nlist: int,
        nprobe: int = 1,
        metric: str = "ip",
        device: Optional[torch.device] = None,
    ) -> None:
        super().__init__()
        if metric not in ("ip", "l2"):
            raise ValueError(f"IVFFlatIndex: metric must be 'ip' or 'l2', got {metric!r}")
        if not 1 <= embedding_dim <= ops.MIPS_TOPK_MAX_D:
            raise ValueError(
                f"IVFFlatIndex: embedding_dim {embedding_dim} is outside 1..{ops.MIPS_TOPK_MAX_D}"
            )
        if not 1 <= nlist <= ops.IVF_TOPK_MAX_LISTS:
            raise ValueError(f"IVFFlatIndex: nlist {nlist} is outside 1..{ops.IVF_TOPK_MAX_LISTS}")
        self.embedding_dim = embedding_dim
        self.nlist = nlist
        self.metric = metric
        self.nprobe = nprobe
        self.is_trained = False
        self._padded_dim = (embedding_dim + 31) // 32 * 32
        self._n = 0
        # list of every stored row while rows wait to be regrouped, else None
        self._row_list: Optional[torch.Tensor] = None
        dp = self._padded_dim
        self.register_buffer("centroids", torch.zeros(nlist, dp, dtype=torch.bfloat16, device=device))
        self.register_buffer("centroid_bias", torch.zeros(nlist, dtype=torch.float32, device=device))
        self.register_buffer("corpus", torch.zeros(0, dp, dtype=torch.bfloat16, device=device))
        self.register_buffer("bias", torch.zeros(0, dtype=torch.float32, device=device))
        self.register_buffer("list_offsets", torch.zeros(nlist + 1, dtype=torch.int64, device=device))
        self.register_buffer("ids", torch.zeros(0, dtype=torch.int64, device=device))

    @property
    def nprobe(self) -> int:
        return self._nprobe

    @nprobe.setter
    def nprobe(self, value: int) -> None:
        top = min(self.nlist, ops.IVF_TOPK_MAX_PROBE)
        if not 1 <= value <= top:
            raise ValueError(f"IVFFlatIndex: nprobe {value} is outside 1..{top}")
        self._nprobe = int(value)

    def __len__(self) -> int:
        return self._n

    def reset(self) -> None:
        """Drop the rows; the centroids stay."""
        self._n = 0
        self._row_list = None
        self.list_offsets.zero_()

    def _pad(self, rows: torch.Tensor) -> torch.Tensor:
        out = rows.new_zeros(rows.shape[0], self._padded_dim)
        out[:, : self.embedding_dim] = rows
        return out

    def _assign(self, rows: torch.Tensor, centroids: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
        """Nearest centroid (L2) of bf16 rows: argmax of x.c - 0.5 ||c||^2."""
        return ops.mips_topk(rows, centroids, 1, row_bias=bias)[1][:, 0]

    @torch.no_grad()
    def train(self, embeddings=True, niter: int = 10, seed: int = 0):
        """Lloyd's k-means on the bf16-rounded rows from ``nlist`` distinct rows
        drawn by a generator seeded with ``seed``. A cluster that loses all its
        rows keeps its centroid. (With a bool it is ``nn.Module.train(mode)``,
        which ``eval()`` of an enclosing model calls.)"""
        if isinstance(embeddings, bool):
            return super().train(embeddings)
        if embeddings.dim() != 2 or embeddings.shape[1] != self.embedding_dim:
            raise ValueError(f"IVFFlatIndex.train: expected [n, {self.embedding_dim}] embeddings")
        if embeddings.shape[0] < self.nlist:
            raise ValueError(
                f"IVFFlatIndex.train: {embeddings.shape[0]} rows for {self.nlist} centroids"
            )
        if self._n:
            raise RuntimeError("IVFFlatIndex.train: reset() the index before training it again")
        dev = self.centroids.device
        x16 = embeddings.to(device=dev, dtype=torch.bfloat16)
        x = x16.float()
        pick = torch.randperm(x.shape[0], generator=torch.Generator().manual_seed(seed))
        cent = x[pick[: self.nlist].to(dev)]
        for it in range(niter + 1):
            c16 = self._pad(cent.bfloat16())
            c_bias = -0.5 * c16.float().square().sum(dim=1)
            if it == niter:
                break
            assign = self._assign(x16, c16, c_bias)
            sums = torch.zeros_like(cent).index_add_(0, assign, x)
            counts = torch.bincount(assign, minlength=self.nlist).unsqueeze(1)
            cent = torch.where(counts > 0, sums / counts.clamp(min=1), cent)
        self.centroids, self.centroid_bias = c16, c_bias
        self.is_trained = True

    def _reserve(self, n: int) -> None:
        cap = self.corpus.shape[0]
        if n <= cap:
            return
        new_cap = max(n, 2 * cap, 1024)
        for name in ("corpus", "bias", "ids"):
            old = getattr(self, name)
            new = old.new_zeros((new_cap,) + tuple(old.shape[1:]))
            new[: self._n] = old[: self._n]
            setattr(self, name, new)

    def _stored_row_list(self) -> torch.Tensor:
        if self._row_list is not None:
            return self._row_list.to(self.corpus.device)
        lists = torch.arange(self.nlist, device=self.corpus.device)
        return torch.repeat_interleave(lists, self.list_offsets.diff())

    @torch.no_grad()
    def add(self, embeddings: torch.Tensor, ids: Optional[torch.Tensor] = None) -> None:
        """File rows [n, embedding_dim], rounded to bf16 once, under their
        nearest centroids. ``ids`` are the item ids a search returns for them
        (default: the number of rows added before each)."""
        if not self.is_trained:
            raise RuntimeError("IVFFlatIndex.add: train() the index first")
        if embeddings.dim() != 2 or embeddings.shape[1] != self.embedding_dim:
            raise ValueError(f"IVFFlatIndex.add: expected [n, {self.embedding_dim}] embeddings")
        if embeddings.shape[0] == 0:
            return
        n0, n1 = self._n, self._n + embeddings.shape[0]
        dev = self.corpus.device
        rows = embeddings.to(device=dev, dtype=torch.bfloat16)
        new_lists = self._assign(rows, self.centroids, self.centroid_bias)
        self._row_list = torch.cat([self._stored_row_list(), new_lists])
        self._reserve(n1)
        self.corpus[n0:n1, : self.embedding_dim] = rows
        if self.metric == "l2":
            self.bias[n0:n1] = -0.5 * rows.float().square().sum(dim=1)
        self.ids[n0:n1] = (
            ids.to(device=dev, dtype=torch.int64).reshape(-1)
            if ids is not None
            else torch.arange(n0, n1, dtype=torch.int64, device=dev)
        )
        self._n = n1

    @torch.no_grad()
    def _regroup(self) -> None:
        """Bring the rows added since the last call into list order: a stable
        sort by list, so a list keeps insertion order."""
        if self._row_list is None:
            return
        n = self._n
        row_list = self._stored_row_list()
        order = torch.argsort(row_list, stable=True)
        for name in ("corpus", "bias", "ids"):
            buf = getattr(self, name)
            buf[:n] = buf[:n][order]
        counts = torch.bincount(row_list, minlength=self.nlist)
        self.list_offsets[1:] = torch.cumsum(counts, dim=0)
        self._row_list = None

    @torch.no_grad()
    def search(self, queries: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """(distances [B, k], ids [B, k]) among the rows of each query's
        ``nprobe`` best lists, as ``FlatIndex.search`` returns them. Where those
        lists hold fewer than k rows the tail is -inf (ip) / +inf (l2), id -1."""
        if not self.is_trained:
            raise RuntimeError("IVFFlatIndex.search: the index is not trained")
        if self._n == 0:
            raise RuntimeError("IVFFlatIndex.search: the index is empty")
        self._regroup()
        n = self._n
        l2 = self.metric == "l2"
        _, probes = ops.mips_topk(
            queries, self.centroids, self._nprobe, row_bias=self.centroid_bias if l2 else None
        )
        scores, rows = ops.ivf_topk(
            queries, self.corpus[:n], self.list_offsets, probes, k,
            row_bias=self.bias[:n] if l2 else None,
        )
        if l2:
            q_norm = queries.bfloat16().float().square().sum(dim=1, keepdim=True)
            scores = q_norm - 2.0 * scores
        return scores, torch.where(rows >= 0, self.ids[rows.clamp(min=0)], rows)

    def state_dict(self, *args, **kwargs):
        self._regroup()
        return super().state_dict(*args, **kwargs)

    # the row count, the trained flag and the buffers' sizes travel with the state dict
    def get_extra_state(self) -> Dict[str, Any]:
        return {"n": self._n, "trained": self.is_trained}

    def set_extra_state(self, state: Dict[str, Any]) -> None:
        self._n = int(state["n"])
        self.is_trained = bool(state["trained"])
        self._row_list = None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs) -> None:
        for name in self._BUFFERS:
            src = state_dict.get(prefix + name)
            if src is not None and src.shape != getattr(self, name).shape:
                setattr(self, name, getattr(self, name).new_zeros(src.shape))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)
