"""Op layer: CPU reference implementations + the gfx950 HIP extension.

Every op has two paths:
  * CPU: a plain-PyTorch reference implementation (used for CPU tests and as
    the numerics oracle for the HIP kernels).
  * GPU (``cuda`` device on ROCm): the hand-written CDNA4 HIP kernels from
    ``torchrec_amd/ops/csrc``.  On a GPU tensor the extension is REQUIRED —
    there is no silent eager fallback (a missing extension raises).

This is the MI355X-native replacement for the reference's external FBGEMM_GPU
op surface (reference call sites cited per-op below).
"""

from __future__ import annotations

import os
from typing import List, NamedTuple, Optional, Tuple, Union

import torch

_EXT = None
_EXT_ERR: Optional[str] = None


def _load_extension():
    """Load the in-tree HIP extension (torchrec_amd/ops/_hip_ops*.so)."""
    global _EXT, _EXT_ERR
    if _EXT is not None or _EXT_ERR is not None:
        return _EXT
    try:
        import importlib

        _EXT = importlib.import_module("torchrec_amd.ops._hip_ops")
    except Exception as e:  # noqa: BLE001
        _EXT_ERR = f"{type(e).__name__}: {e}"
        _EXT = None
    return _EXT


def hip_ops():
    """Return the HIP extension module; raise loudly if it is missing.

    Called on every GPU-tensor op so a GPU run can never silently fall back
    to eager PyTorch.
    """
    ext = _load_extension()
    if ext is None:
        raise RuntimeError(
            "torchrec_amd HIP extension (_hip_ops) is not built but a GPU "
            f"tensor op was requested. Build it with `python setup.py "
            f"build_ext --inplace` (PYTORCH_ROCM_ARCH=gfx950). Import error: {_EXT_ERR}"
        )
    return ext


def extension_available() -> bool:
    return _load_extension() is not None


# ------------------------------------------------------------------------
# lengths <-> offsets
# ------------------------------------------------------------------------


def complete_cumsum(lengths: torch.Tensor) -> torch.Tensor:
    """[0, cumsum(lengths)] of length N+1 (int64 in == int64 out).

    Semantics of the reference's ``asynchronous_complete_cumsum``
    (reference: torchrec/sparse/jagged_tensor.py:157).
    """
    if lengths.is_cuda:
        hip_ops()
        return torch.ops.trec_amd.complete_cumsum(lengths)
    out = torch.zeros(lengths.numel() + 1, dtype=lengths.dtype, device=lengths.device)
    torch.cumsum(lengths, dim=0, out=out[1:])
    return out


def offsets_to_lengths(offsets: torch.Tensor) -> torch.Tensor:
    return offsets[1:] - offsets[:-1]


def lengths_range(offsets: torch.Tensor) -> torch.Tensor:
    """For each segment i with length L_i emit [0, 1, ..., L_i-1] concatenated.

    Semantics of ``fbgemm.offsets_range`` (reference:
    torchrec/modules/feature_processor.py:57).
    """
    lengths = offsets_to_lengths(offsets)
    if offsets.is_cuda:
        hip_ops()
        return torch.ops.trec_amd.lengths_range(offsets)
    seq = torch.arange(int(offsets[-1]), device=offsets.device, dtype=offsets.dtype)
    starts = torch.repeat_interleave(offsets[:-1], lengths)
    return seq - starts


def expand_into_bag_ids(offsets: torch.Tensor, total: Optional[int] = None) -> torch.Tensor:
    """Position -> bag id (inverse of offsets). CPU + GPU (repeat_interleave)."""
    lengths = offsets_to_lengths(offsets)
    return torch.repeat_interleave(
        torch.arange(lengths.numel(), device=offsets.device, dtype=offsets.dtype), lengths
    )


# ------------------------------------------------------------------------
# KJT permute / split support
# ------------------------------------------------------------------------


def permute_2d_sparse_data(
    permute: torch.Tensor,
    lengths: torch.Tensor,  # [K, B]
    values: torch.Tensor,
    weights: Optional[torch.Tensor] = None,
    permuted_lengths_sum: Optional[int] = None,
) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Permute a feature-major KJT's (lengths, values[, weights]) by feature.

    ``permute[i] = j`` means output feature-row i is input feature-row j.
    Semantics of ``fbgemm.permute_2D_sparse_data`` (reference:
    torchrec/sparse/jagged_tensor.py:2913).
    Returns (permuted_lengths [K',B], permuted_values, permuted_weights).
    """
    if values.is_cuda:
        hip_ops()
        pl, pv, pw = torch.ops.trec_amd.permute_2d_sparse_data(
            permute,
            lengths,
            values,
            weights if weights is not None else torch.empty(0),
            -1 if permuted_lengths_sum is None else permuted_lengths_sum,
        )
        return pl, pv, (pw if weights is not None else None)
    K, B = lengths.shape
    offsets = complete_cumsum(lengths.reshape(-1))
    perm_lengths = lengths[permute]
    chunks = []
    wchunks = []
    for i in range(permute.numel()):
        j = int(permute[i])
        start = int(offsets[j * B])
        end = int(offsets[(j + 1) * B])
        chunks.append(values[start:end])
        if weights is not None:
            wchunks.append(weights[start:end])
    pv = torch.cat(chunks) if chunks else values.new_empty(0)
    pw = (torch.cat(wchunks) if wchunks else weights.new_empty(0)) if weights is not None else None
    return perm_lengths, pv, pw


def permute_1d_sparse_data(
    permute: torch.Tensor,
    lengths: torch.Tensor,  # [N]
    values: torch.Tensor,
    weights: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Permute variable-length segments (1-D lengths) by segment index.

    Semantics of ``fbgemm.permute_1D_sparse_data`` (reference:
    torchrec/sparse/jagged_tensor.py:3381).
    """
    lengths2d = lengths.view(-1, 1)
    pl, pv, pw = permute_2d_sparse_data(permute, lengths2d, values, weights)
    return pl.view(-1), pv, pw


def invert_permute(permute: torch.Tensor) -> torch.Tensor:
    """inverse[permute[i]] = i (reference: torchrec/distributed/dist_data.py:2068)."""
    inv = torch.empty_like(permute)
    inv[permute] = torch.arange(permute.numel(), device=permute.device, dtype=permute.dtype)
    return inv


# ------------------------------------------------------------------------
# jagged <-> dense
# ------------------------------------------------------------------------


def jagged_to_padded_dense(
    values: torch.Tensor,
    offsets: torch.Tensor,
    max_length: int,
    padding_value: float = 0.0,
) -> torch.Tensor:
    """[sum_L, D?] jagged -> [B, max_length, D?] padded dense.

    Semantics of ``fbgemm.jagged_to_padded_dense`` (reference:
    torchrec/sparse/jagged_tensor.py:1005).
    """
    two_d = values.dim() == 2
    vals2 = values if two_d else values.unsqueeze(1)
    if values.is_cuda:
        hip_ops()
        out = torch.ops.trec_amd.jagged_to_padded_dense(vals2, offsets, max_length, padding_value)
        return out if two_d else out.squeeze(-1)
    B = offsets.numel() - 1
    D = vals2.shape[1]
    out = torch.full((B, max_length, D), padding_value, dtype=values.dtype, device=values.device)
    for b in range(B):
        start, end = int(offsets[b]), int(offsets[b + 1])
        n = min(end - start, max_length)
        out[b, :n] = vals2[start : start + n]
    return out if two_d else out.squeeze(-1)


def dense_to_jagged(dense: torch.Tensor, offsets: torch.Tensor) -> torch.Tensor:
    """[B, max_length, D] dense -> [sum_L, D] jagged (inverse of padding)."""
    if dense.is_cuda:
        hip_ops()
        return torch.ops.trec_amd.dense_to_jagged(dense, offsets)
    B = offsets.numel() - 1
    chunks = []
    for b in range(B):
        n = int(offsets[b + 1]) - int(offsets[b])
        chunks.append(dense[b, :n])
    return torch.cat(chunks) if chunks else dense.new_empty((0, dense.shape[-1]))


# ------------------------------------------------------------------------
# segment ops
# ------------------------------------------------------------------------


def segment_sum_csr(batch_size: int, csr_seg: torch.Tensor, values: torch.Tensor) -> torch.Tensor:
    """Sum `values` over CSR segments of size `batch_size` groups.

    Semantics of ``fbgemm.segment_sum_csr`` (reference:
    torchrec/sparse/jagged_tensor.py:1346): csr_seg has S+1 entries; output[s]
    = sum(values[csr_seg[s]:csr_seg[s+1]]).
    """
    if values.is_cuda:
        hip_ops()
        return torch.ops.trec_amd.segment_sum_csr(csr_seg, values)
    out = values.new_empty(csr_seg.numel() - 1)
    for s in range(csr_seg.numel() - 1):
        out[s] = values[int(csr_seg[s]) : int(csr_seg[s + 1])].sum()
    return out


# ------------------------------------------------------------------------
# RW-sharding bucketize
# ------------------------------------------------------------------------


def block_bucketize_sparse_features(
    lengths: torch.Tensor,  # [F * B] feature-major
    indices: torch.Tensor,
    bucketize_pos: bool,
    sequence: bool,
    block_sizes: torch.Tensor,  # [F] rows per bucket-block for each feature
    num_buckets: int,
    weights: Optional[torch.Tensor] = None,
    total_num_blocks: Optional[torch.Tensor] = None,  # [F]; uniform blocks when set
    bag_feature_bounds: Optional[torch.Tensor] = None,  # [F+1] VBE bag->feature
) -> Tuple[
    torch.Tensor,
    torch.Tensor,
    Optional[torch.Tensor],
    Optional[torch.Tensor],
    Optional[torch.Tensor],
]:
    """Bucketize row ids into `num_buckets` contiguous row ranges per feature.

    Output layout is bucket-major: [bucket 0: all features/samples, bucket 1:
    ...], each bucket internally feature-major like the input. Returns
    (bucketized_lengths [num_buckets * F * B], bucketized_indices (local row
    ids), bucketized_weights, bucketized_pos, unbucketize_permute).

    Semantics of ``fbgemm.block_bucketize_sparse_features`` (reference:
    torchrec/distributed/embedding_sharding.py:315).
    """
    if indices.is_cuda:
        hip_ops()
        w = weights if weights is not None else torch.empty(0, device=indices.device)
        bb = (
            bag_feature_bounds
            if bag_feature_bounds is not None
            else torch.empty(0, dtype=torch.int64, device=indices.device)
        )
        bl, bi, bw, bp, up = torch.ops.trec_amd.block_bucketize_sparse_features(
            lengths, indices, block_sizes, num_buckets, bucketize_pos, sequence, w, bb
        )
        return (
            bl,
            bi,
            bw if weights is not None else None,
            bp if bucketize_pos else None,
            up if sequence else None,
        )
    FB = lengths.numel()
    F = block_sizes.numel()
    B = FB // F
    if bag_feature_bounds is not None:
        bounds = [int(x) for x in bag_feature_bounds]
        def _feat_of(bag: int) -> int:
            for fi in range(F):
                if bounds[fi] <= bag < bounds[fi + 1]:
                    return fi
            return F - 1
    else:
        def _feat_of(bag: int) -> int:
            return bag // B
    offsets = complete_cumsum(lengths)
    new_lengths = torch.zeros(num_buckets * FB, dtype=lengths.dtype)
    # bucket of each value
    bucket_of = torch.empty_like(indices)
    local_idx = torch.empty_like(indices)
    pos_list = torch.empty_like(indices) if bucketize_pos else None
    for bag in range(FB):
        f = _feat_of(bag)
        bs = int(block_sizes[f])
        start, end = int(offsets[bag]), int(offsets[bag + 1])
        for p in range(start, end):
            idx = int(indices[p])
            bkt = min(idx // bs, num_buckets - 1)
            bucket_of[p] = bkt
            local_idx[p] = idx - bkt * bs
            new_lengths[bkt * FB + bag] += 1
            if bucketize_pos:
                pos_list[p] = p - start
    new_offsets = complete_cumsum(new_lengths)
    new_indices = torch.empty_like(indices)
    new_weights = torch.empty_like(weights) if weights is not None else None
    new_pos = torch.empty_like(indices) if bucketize_pos else None
    unbucketize = torch.empty(indices.numel(), dtype=torch.int64) if sequence else None
    cursor = new_offsets[:-1].clone()
    for bag in range(FB):
        start, end = int(offsets[bag]), int(offsets[bag + 1])
        for p in range(start, end):
            bkt = int(bucket_of[p])
            slot = int(cursor[bkt * FB + bag])
            cursor[bkt * FB + bag] += 1
            new_indices[slot] = local_idx[p]
            if new_weights is not None:
                new_weights[slot] = weights[p]
            if bucketize_pos:
                new_pos[slot] = pos_list[p]
            if sequence:
                unbucketize[p] = slot
    return new_lengths, new_indices, new_weights, new_pos, unbucketize


# ------------------------------------------------------------------------
# pooled-embedding layout ops
# ------------------------------------------------------------------------


class _PermutePooledEmbs(torch.autograd.Function):
    """Differentiable column-group permute of [B, sum_D] pooled embeddings.

    Semantics of ``fbgemm.permute_pooled_embs_auto_grad`` (reference:
    torchrec/sparse/jagged_tensor.py:308).
    """

    @staticmethod
    def forward(ctx, values, in_offsets, out_offsets, order):  # type: ignore[override]
        ctx.save_for_backward(in_offsets, out_offsets, order)
        if values.is_cuda:
            hip_ops()
            return torch.ops.trec_amd.permute_pooled_embs(values, in_offsets, out_offsets, order)
        cols = []
        for i in range(order.numel()):
            g = int(order[i])
            cols.append(values[:, int(in_offsets[g]) : int(in_offsets[g + 1])])
        return torch.cat(cols, dim=1) if cols else values

    @staticmethod
    def backward(ctx, grad):  # type: ignore[override]
        in_offsets, out_offsets, order = ctx.saved_tensors
        inv = invert_permute(order)
        # output group j sits at out_offsets[j]; backward scatters back
        if grad.is_cuda:
            g = torch.ops.trec_amd.permute_pooled_embs(grad, out_offsets, in_offsets, inv)
        else:
            cols = []
            for i in range(inv.numel()):
                j = int(inv[i])
                cols.append(grad[:, int(out_offsets[j]) : int(out_offsets[j + 1])])
            g = torch.cat(cols, dim=1) if cols else grad
        return g, None, None, None


def permute_pooled_embs(
    values: torch.Tensor,
    group_dims: List[int],
    order: torch.Tensor,
) -> torch.Tensor:
    """Permute column groups of a [B, sum_D] tensor; differentiable."""
    device = values.device
    in_offsets = complete_cumsum(torch.tensor(group_dims, dtype=torch.int64)).to(device)
    out_dims = [group_dims[int(order[i])] for i in range(order.numel())]
    out_offsets = complete_cumsum(torch.tensor(out_dims, dtype=torch.int64)).to(device)
    return _PermutePooledEmbs.apply(values, in_offsets, out_offsets, order.to(device))


# ------------------------------------------------------------------------
# fused DLRM interaction (pairwise dot + triu + cat), CDNA4 kernel
# ------------------------------------------------------------------------

_PAIR_TABLES: dict = {}


def _pair_tables(F1: int, device: torch.device):
    key = (F1, device)
    if key not in _PAIR_TABLES:
        tri = torch.triu_indices(F1, F1, offset=1)
        P = tri.shape[1]
        # int16: the VALU kernel takes any F, and int8 wraps above row 127
        pi = tri[0].to(torch.int16)
        pj = tri[1].to(torch.int16)
        pair_col = torch.full((F1 * F1,), -1, dtype=torch.int32)
        for p in range(P):
            i, j = int(tri[0, p]), int(tri[1, p])
            pair_col[i * F1 + j] = p
            pair_col[j * F1 + i] = p
        _PAIR_TABLES[key] = (pi.to(device), pj.to(device), pair_col.to(device))
    return _PAIR_TABLES[key]


class _FusedInteraction(torch.autograd.Function):
    """out = [dense, triu(T @ T^T)] with T = [dense; sparse] — single kernel
    each way (csrc/interaction.hip); replaces cat+bmm+gather."""

    @staticmethod
    def forward(ctx, dense, sparse):  # type: ignore[override]
        F1 = sparse.shape[1] + 1
        pi, pj, pair_col = _pair_tables(F1, dense.device)
        d32 = dense.float()
        s32 = sparse.float()
        ctx.save_for_backward(d32, s32, pair_col)
        ctx.dtypes = (dense.dtype, sparse.dtype)
        return torch.ops.trec_amd.interaction_forward(d32, s32, pi, pj)

    @staticmethod
    def backward(ctx, grad_out):  # type: ignore[override]
        d32, s32, pair_col = ctx.saved_tensors
        dd, ds = torch.ops.trec_amd.interaction_backward(
            grad_out.float().contiguous(), d32, s32, pair_col
        )
        ddt, dst = ctx.dtypes
        return dd.to(ddt), ds.to(dst)


class _FusedInteractionMFMA(torch.autograd.Function):
    """MFMA (matrix-core) variant: per-sample Z = T @ T^T / dT = G @ T run on
    v_mfma_f32_16x16x32_bf16 tiles with fp32 accumulate
    (csrc/interaction_mfma.hip). Inputs round to bf16 inside the kernel —
    the standard autocast regime of the surrounding dense arch."""

    @staticmethod
    def forward(ctx, dense, sparse):  # type: ignore[override]
        F1 = sparse.shape[1] + 1
        pi, pj, pair_col = _pair_tables(F1, dense.device)
        if dense.dtype != sparse.dtype:
            dense = dense.to(sparse.dtype)
        ctx.save_for_backward(dense, sparse, pair_col)
        return torch.ops.trec_amd.interaction_mfma_forward(dense, sparse, pi, pj)

    @staticmethod
    def backward(ctx, grad_out):  # type: ignore[override]
        d, s, pair_col = ctx.saved_tensors
        dd, ds = torch.ops.trec_amd.interaction_mfma_backward(
            grad_out.to(d.dtype).contiguous(), d, s, pair_col
        )
        return dd, ds


def _mfma_interaction_ok(dense: torch.Tensor, sparse: torch.Tensor) -> bool:
    D = dense.shape[1]
    F1 = sparse.shape[1] + 1
    return (
        D % 32 == 0
        and 64 <= D <= 256
        and F1 <= 32
        and os.environ.get("TREC_INTERACTION_FP32") != "1"
    )


def fused_interaction(dense: torch.Tensor, sparse: torch.Tensor) -> torch.Tensor:
    """GPU: fused kernel (MFMA bf16 tiles where the shape allows, fp32 VALU
    otherwise or under TREC_INTERACTION_FP32=1); CPU callers should use the
    eager path."""
    hip_ops()
    if _mfma_interaction_ok(dense, sparse):
        return _FusedInteractionMFMA.apply(dense, sparse)
    return _FusedInteraction.apply(dense, sparse)


# ------------------------------------------------------------------------
# fused DCN-v2 low-rank cross stack (csrc/cross_mfma.hip)
# ------------------------------------------------------------------------


def lowrank_cross_shape_ok(n_features: int, rank: int) -> bool:
    """Shape rules of the fused cross kernels (bf16 operands assumed)."""
    return n_features > 0 and n_features % 32 == 0 and rank % 32 == 0 and 32 <= rank <= 512


def _cross_wgrad(g: torch.Tensor, x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(g^T @ x, colsum(g)) over the batch: the hipBLASLt bias-grad epilogue
    GEMM where the batch is a multiple of 8 rows and at least one k tile
    deep, torch.matmul + the col_sum kernel otherwise."""
    if g.shape[0] >= 64 and g.shape[0] % 8 == 0:
        return torch.ops.trec_amd.lt_wgrad_bgrad(g, x)
    return g.t() @ x, torch.ops.trec_amd.col_sum(g)


class _LowRankCross(torch.autograd.Function):
    """x_{l+1} = x_0 * (W_l (V_l x_l) + b_l) + x_l for the whole stack: one
    forward and one backward-data kernel per layer; the weight gradients are
    batch-deep GEMMs over the kernels' u = g * x_0 and dt = u W outputs."""

    @staticmethod
    def forward(ctx, x0, save_t, num_layers, *params):  # type: ignore[override]
        L = num_layers
        bf16 = torch.bfloat16
        Vs = [p.to(bf16) for p in params[:L]]
        Ws = [p.to(bf16) for p in params[L : 2 * L]]
        bs = [p.float() for p in params[2 * L :]]
        xs, ts = [x0], []
        for l in range(L):
            y, t = torch.ops.trec_amd.lowrank_cross_fwd(x0, xs[-1], Vs[l], Ws[l], bs[l], save_t)
            xs.append(y)
            ts.append(t)
        if save_t:
            ctx.save_for_backward(*xs[:L], *ts, *Vs, *Ws, *bs)
        ctx.num_layers = L
        ctx.param_dtypes = [p.dtype for p in params]
        return xs[-1]

    @staticmethod
    def backward(ctx, grad):  # type: ignore[override]
        L = ctx.num_layers
        saved = ctx.saved_tensors
        xs, ts = saved[:L], saved[L : 2 * L]
        Vs, Ws, bs = saved[2 * L : 3 * L], saved[3 * L : 4 * L], saved[4 * L :]
        x0 = xs[0]
        g = grad.to(torch.bfloat16).contiguous()
        dx0_acc = torch.zeros(x0.shape, dtype=torch.float32, device=x0.device)
        dV: List[Optional[torch.Tensor]] = [None] * L
        dW: List[Optional[torch.Tensor]] = [None] * L
        db: List[Optional[torch.Tensor]] = [None] * L
        for l in reversed(range(L)):
            g, u, dt = torch.ops.trec_amd.lowrank_cross_bwd(
                g, x0, xs[l], ts[l], Vs[l], Ws[l], bs[l], dx0_acc
            )
            dW[l], db[l] = _cross_wgrad(u, ts[l])
            dV[l], _ = _cross_wgrad(dt, xs[l])
        # layer 0's x_l is x_0: fold its dx_l into the fp32 sum, cast once
        dx0 = (dx0_acc + g.float()).to(x0.dtype)
        grads = [d.to(dt_) for d, dt_ in zip(dV + dW + db, ctx.param_dtypes)]
        return (dx0, None, None, *grads)


def lowrank_cross(
    x0: torch.Tensor,
    V_list: List[torch.Tensor],
    W_list: List[torch.Tensor],
    b_list: List[torch.Tensor],
) -> torch.Tensor:
    """DCN-v2 low-rank cross stack (reference: torchrec/modules/crossnet.py
    LowRankCrossNet): x_{l+1} = x_0 * (W_l (V_l x_l) + b_l) + x_l with V_l
    [r, N], W_l [N, r], b_l [N].

    GPU: bf16 x0, N % 32 == 0, r % 32 == 0, 32 <= r <= 512; fp32 parameters
    are cast to bf16 for the call (b is read as fp32) and get gradients in
    their own dtype. CPU: the plain recurrence."""
    if not x0.is_cuda:
        x_l = x0
        for V, W, b in zip(V_list, W_list, b_list):
            x_l_v = torch.nn.functional.linear(x_l, V)
            x_l_w = torch.nn.functional.linear(x_l_v, W)
            x_l = x0 * (x_l_w + b) + x_l
        return x_l
    hip_ops()
    L = len(V_list)
    if L == 0:
        return x0
    params = [*V_list, *W_list, *b_list]
    save_t = torch.is_grad_enabled() and (x0.requires_grad or any(p.requires_grad for p in params))
    return _LowRankCross.apply(x0.contiguous(), save_t, L, *params)


# ------------------------------------------------------------------------
# exhaustive top-k retrieval (csrc/mips_topk.hip)
# ------------------------------------------------------------------------

MIPS_TOPK_MAX_D = 256
MIPS_TOPK_MAX_K = 128


def mips_topk(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    k: int,
    row_bias: Optional[torch.Tensor] = None,
    splits: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Exact top-k of ``queries @ corpus.T (+ row_bias)`` per query.

    queries [B, D] fp32 or bf16 (rounded to bf16, RNE); corpus [N, Dp] bf16,
    contiguous, Dp = D rounded up to a multiple of 32 with zero pad columns;
    row_bias fp32 [N]. Returns (scores fp32 [B, k], ids int64 [B, k]) ordered
    by score descending, then id ascending; with N < k the tail is -inf / -1.
    ``splits`` forces the number of corpus splits on the GPU (0: from the
    shapes); it does not change the result. Scores must not be NaN: the GPU
    path drops a NaN score, the CPU sort would rank it first; +-inf are ordered.

    GPU: the fused score-and-select MFMA kernels, the score matrix is never
    materialised. CPU: an fp32 matmul of the bf16 values and a stable sort.
    """
    if queries.dim() != 2 or corpus.dim() != 2:
        raise ValueError("mips_topk: queries [B, D] and corpus [N, Dp] must be 2-D")
    D, (N, Dp) = queries.shape[1], corpus.shape
    if not 1 <= D <= MIPS_TOPK_MAX_D:
        raise ValueError(f"mips_topk: embedding width {D} is outside 1..{MIPS_TOPK_MAX_D}")
    if not 1 <= k <= MIPS_TOPK_MAX_K:
        raise ValueError(f"mips_topk: k = {k} is outside 1..{MIPS_TOPK_MAX_K}")
    if Dp % 32 != 0 or Dp != (D + 31) // 32 * 32:
        raise ValueError(
            f"mips_topk: corpus width {Dp} must be D = {D} rounded up to a multiple of 32"
        )
    if corpus.dtype != torch.bfloat16 or not corpus.is_contiguous():
        raise ValueError("mips_topk: corpus must be a contiguous bf16 tensor")
    if queries.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("mips_topk: queries must be fp32 or bf16")
    if row_bias is not None and (row_bias.shape != (N,) or row_bias.dtype != torch.float32):
        raise ValueError("mips_topk: row_bias must be an fp32 [N] tensor")
    if queries.is_cuda:
        hip_ops()
        return torch.ops.trec_amd.mips_topk(queries, corpus, row_bias, k, splits)
    scores = queries.bfloat16().float() @ corpus[:, :D].float().t()
    if row_bias is not None:
        scores = scores + row_bias
    top, ids = torch.sort(scores, dim=1, descending=True, stable=True)
    top, ids = top[:, :k], ids[:, :k]
    if N < k:
        pad = (queries.shape[0], k - N)
        top = torch.cat([top, top.new_full(pad, float("-inf"))], dim=1)
        ids = torch.cat([ids, ids.new_full(pad, -1)], dim=1)
    return top.contiguous(), ids.contiguous()


# ------------------------------------------------------------------------
# IVF-Flat fine stage: top-k restricted to probed lists (csrc/ivf_topk.hip)
# ------------------------------------------------------------------------

IVF_TOPK_MAX_PROBE = 128
IVF_TOPK_MAX_LISTS = 65536


def ivf_topk(
    queries: torch.Tensor,
    corpus: torch.Tensor,
    list_offsets: torch.Tensor,
    probes: torch.Tensor,
    k: int,
    row_bias: Optional[torch.Tensor] = None,
    splits: int = 0,
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Top-k of ``queries @ corpus.T (+ row_bias)`` per query among the rows of
    the lists it probes.

    queries, corpus, row_bias, k and the order of the result are those of
    ``mips_topk``. The corpus is stored list by list: list l is rows
    ``[list_offsets[l], list_offsets[l + 1])`` of it, list_offsets int64
    [nlist + 1], non-decreasing from 0 to N, empty lists allowed. probes int64
    [B, nprobe] names each query's lists; -1 is "no list", the other entries of
    a row must be distinct. Returns (scores fp32 [B, k], rows int64 [B, k]);
    where the probed lists hold fewer than k rows the tail is -inf / -1.
    ``splits`` forces the number of row ranges a list is cut into on the GPU
    (0: from the shapes); it does not change the result.

    GPU: a device-side plan turns the probes list-major, then each list is read
    once per 32 queries that probe it by the fused score-and-select MFMA
    kernel; no host synchronisation. CPU: the masked fp32 score matrix and a
    stable sort.
    """
    if queries.dim() != 2 or corpus.dim() != 2:
        raise ValueError("ivf_topk: queries [B, D] and corpus [N, Dp] must be 2-D")
    (B, D), (N, Dp) = queries.shape, corpus.shape
    if not 1 <= D <= MIPS_TOPK_MAX_D:
        raise ValueError(f"ivf_topk: embedding width {D} is outside 1..{MIPS_TOPK_MAX_D}")
    if not 1 <= k <= MIPS_TOPK_MAX_K:
        raise ValueError(f"ivf_topk: k = {k} is outside 1..{MIPS_TOPK_MAX_K}")
    if Dp % 32 != 0 or Dp != (D + 31) // 32 * 32:
        raise ValueError(
            f"ivf_topk: corpus width {Dp} must be D = {D} rounded up to a multiple of 32"
        )
    if corpus.dtype != torch.bfloat16 or not corpus.is_contiguous():
        raise ValueError("ivf_topk: corpus must be a contiguous bf16 tensor")
    if queries.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError("ivf_topk: queries must be fp32 or bf16")
    if row_bias is not None and (row_bias.shape != (N,) or row_bias.dtype != torch.float32):
        raise ValueError("ivf_topk: row_bias must be an fp32 [N] tensor")
    if (
        list_offsets.dim() != 1
        or list_offsets.dtype != torch.int64
        or not 1 <= list_offsets.numel() - 1 <= IVF_TOPK_MAX_LISTS
    ):
        raise ValueError(
            f"ivf_topk: list_offsets must be int64 [nlist + 1], nlist in 1..{IVF_TOPK_MAX_LISTS}"
        )
    if (
        probes.dim() != 2
        or probes.dtype != torch.int64
        or probes.shape[0] != B
        or not 1 <= probes.shape[1] <= IVF_TOPK_MAX_PROBE
    ):
        raise ValueError(
            f"ivf_topk: probes must be int64 [B, nprobe], nprobe in 1..{IVF_TOPK_MAX_PROBE}"
        )
    if queries.is_cuda:
        hip_ops()
        return torch.ops.trec_amd.ivf_topk(
            queries, corpus, list_offsets, probes, row_bias, k, splits
        )
    nlist = list_offsets.numel() - 1
    scores = queries.bfloat16().float() @ corpus[:, :D].float().t()
    if row_bias is not None:
        scores = scores + row_bias
    # list of every row (empty lists own none), then one extra column for -1
    row_list = torch.searchsorted(list_offsets[1:].contiguous(), torch.arange(N), right=True)
    probed = torch.zeros(B, nlist + 1, dtype=torch.bool)
    probed.scatter_(1, torch.where(probes < 0, nlist, probes), True)
    scores = scores.masked_fill(~probed[:, :nlist][:, row_list], float("-inf"))
    top, ids = torch.sort(scores, dim=1, descending=True, stable=True)
    top, ids = top[:, :k], ids[:, :k]
    if N < k:
        pad = (B, k - N)
        top = torch.cat([top, top.new_full(pad, float("-inf"))], dim=1)
        ids = torch.cat([ids, ids.new_full(pad, -1)], dim=1)
    ids = ids.masked_fill(top == float("-inf"), -1)
    return top.contiguous(), ids.contiguous()


class _FusedBceWithLogits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):  # type: ignore[override]
        labels_f = labels.float()
        ctx.save_for_backward(logits, labels_f)
        return torch.ops.trec_amd.bce_with_logits_fwd(logits, labels_f)

    @staticmethod
    def backward(ctx, grad_out):  # type: ignore[override]
        logits, labels_f = ctx.saved_tensors
        dx = torch.ops.trec_amd.bce_with_logits_bwd(
            logits, labels_f, grad_out.contiguous().float()
        )
        return dx, None


def fused_bce_with_logits(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean-reduced BCEWithLogits in two kernels (fwd deterministic two-level
    reduce; bwd one elementwise pass) — torch's nn.BCEWithLogitsLoss chain is
    ~12 launch-floor kernels inside a captured graph."""
    hip_ops()
    return _FusedBceWithLogits.apply(logits.contiguous(), labels)


def jagged_index_select_2d(
    values: torch.Tensor, lengths: torch.Tensor, indices: torch.Tensor
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Select (and possibly duplicate) jagged segments by segment index.

    Semantics of ``fbgemm.jagged_index_select_2d_forward_v2`` (reference:
    torchrec/modules/utils.py:427). Returns (selected_values,
    selected_lengths)."""
    pl, pv, _ = permute_1d_sparse_data(indices, lengths, values)
    return pv, pl


def jagged_unique_indices(
    hash_size_offsets: torch.Tensor,
    offsets: torch.Tensor,
    indices: torch.Tensor,
) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Dedup ids within hash-size buckets (reference fbgemm
    jagged_unique_indices, used for sequence input dedup at
    torchrec/distributed/embedding.py:1439).

    Returns (output_lengths, output_offsets, unique_indices, reverse_index):
    ids are linearized by their bucket, deduped (sorted), and every original
    position maps to its unique slot via ``reverse_index``."""
    n_buckets = hash_size_offsets.numel() - 1
    lengths = offsets[1:] - offsets[:-1]
    # bucket of each position (buckets delimit ranges of the lengths array)
    pos_bucket = torch.repeat_interleave(
        torch.arange(n_buckets, device=indices.device),
        (
            offsets[hash_size_offsets[1:].to(torch.int64)]
            - offsets[hash_size_offsets[:-1].to(torch.int64)]
        ),
    ) if n_buckets else torch.zeros_like(indices)
    lin = indices + pos_bucket * (int(indices.max()) + 1 if indices.numel() else 1)
    uniq, inverse = torch.unique(lin, sorted=True, return_inverse=True)
    u_bucket = torch.div(
        uniq, (int(indices.max()) + 1 if indices.numel() else 1), rounding_mode="floor"
    )
    out_lengths = torch.bincount(u_bucket, minlength=n_buckets)
    out_offsets = torch.zeros(n_buckets + 1, dtype=offsets.dtype, device=offsets.device)
    torch.cumsum(out_lengths, 0, out=out_offsets[1:])
    uniq_local = uniq - u_bucket * (int(indices.max()) + 1 if indices.numel() else 1)
    return out_lengths, out_offsets, uniq_local, inverse


def group_index_select_dim0(
    tensors: List[torch.Tensor], indices: List[torch.Tensor]
) -> List[torch.Tensor]:
    """Grouped row select (reference fbgemm group_index_select_dim0, used at
    torchrec/modules/embedding_modules.py:78)."""
    return [t.index_select(0, i.to(t.device)) for t, i in zip(tensors, indices)]


def batch_index_select_dim0(
    flat: torch.Tensor,
    indices: torch.Tensor,
    input_num_indices: List[int],
    input_rows: List[int],
    input_columns: List[int],
) -> torch.Tensor:
    """Batched row select over a flat buffer of stacked tables (reference
    fbgemm batch_index_select_dim0, torchrec/distributed/embeddingbag.py:411)."""
    outs = []
    row_off = 0
    idx_off = 0
    for n_idx, rows, cols in zip(input_num_indices, input_rows, input_columns):
        table = flat[row_off : row_off + rows * cols].view(rows, cols)
        idx = indices[idx_off : idx_off + n_idx]
        outs.append(table.index_select(0, idx).reshape(-1))
        row_off += rows * cols
        idx_off += n_idx
    return torch.cat(outs) if outs else flat.new_empty(0)


def expand_into_jagged_permute(
    permute: torch.Tensor,
    input_offsets: torch.Tensor,
    output_offsets: torch.Tensor,
    output_size: int,
) -> torch.Tensor:
    """Expand a segment-level permute into a position-level permute
    (reference fbgemm expand_into_jagged_permute, VBE output permute at
    torchrec/distributed/dist_data.py:340): output position j of segment i
    maps to input position input_offsets[permute[i]] + j."""
    n = permute.numel()
    out = torch.empty(output_size, dtype=torch.int64, device=permute.device)
    for i in range(n):
        o0, o1 = int(output_offsets[i]), int(output_offsets[i + 1])
        src = int(input_offsets[int(permute[i])])
        out[o0:o1] = torch.arange(src, src + (o1 - o0), device=permute.device)
    return out


def keyed_jagged_index_select_dim1(
    values: torch.Tensor,
    lengths: torch.Tensor,
    offsets: torch.Tensor,
    indices: torch.Tensor,
    batch_size: int,
    weights: Optional[torch.Tensor] = None,
) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
    """Select batch positions across every key of a feature-major KJT
    (semantics of ``fbgemm.keyed_jagged_index_select_dim1``, reference
    torchrec/sparse/jagged_tensor.py:531). ``lengths`` is [K*B]; the same
    ``indices`` (into the batch dim) apply to each key. Returns
    (values, lengths[, weights]) of the selected KJT."""
    K = lengths.numel() // batch_size
    sel = torch.cat(
        [indices + k * batch_size for k in range(K)]
    )
    pl, pv, pw = permute_1d_sparse_data(sel, lengths, values, weights)
    return pv, pl, pw


# ------------------------------------------------------------------------
# OCP microscaling wire codec for the quantized a2a (csrc/qcomm_codec.hip)
# ------------------------------------------------------------------------

# groups of 32 values per workgroup tile of the HIP kernels (kMxTileGroups)
QCOMM_MX_TILE_GROUPS = 256
_MX_FMT_IDS = {"mxfp8": 0, "mxfp4": 1}
_MX_COL_OFFS: dict = {}


def _mx_col_off(block_dims: List[int], device: torch.device) -> torch.Tensor:
    """Device int32 [n_blocks + 1] first column of every rank block."""
    key = (tuple(block_dims), device)
    if key not in _MX_COL_OFFS:
        offs = [0]
        for d in block_dims:
            assert d % 32 == 0, f"MX slab blocks need widths % 32 == 0, got {list(block_dims)}"
            offs.append(offs[-1] + d)
        _MX_COL_OFFS[key] = torch.tensor(offs, dtype=torch.int32).to(device)
    return _MX_COL_OFFS[key]


def _mx_no_table(device: torch.device) -> torch.Tensor:
    """Requires the extension; the empty column table selects flat mode."""
    assert hip_ops().qcomm_mx_tile_groups == QCOMM_MX_TILE_GROUPS
    return torch.empty(0, dtype=torch.int32, device=device)


def qcomm_mx_encode(
    x: torch.Tensor, fmt: str, block_dims: Optional[List[int]] = None
) -> torch.Tensor:
    """fp32 message -> int8 MXFP8 / MXFP4 wire (``fmt``: "mxfp8" | "mxfp4").

    Flat (``block_dims`` None): ``x`` is the message. Slab: ``x`` is a
    [B, sum(block_dims)] matrix and the message is the concatenation over r
    of its flattened [B, block_dims[r]] column block.
    """
    if block_dims is not None:
        assert x.dim() == 2 and x.shape[1] == sum(block_dims), (tuple(x.shape), block_dims)
    if x.is_cuda:
        no_table = _mx_no_table(x.device)
        x = x.float()
        if block_dims is None:
            return torch.ops.trec_amd.qcomm_mx_encode(x.reshape(-1), _MX_FMT_IDS[fmt], no_table, 0)
        return torch.ops.trec_amd.qcomm_mx_encode(
            x, _MX_FMT_IDS[fmt], _mx_col_off(block_dims, x.device), x.shape[0]
        )
    from torchrec_amd.distributed import qcomm_codecs as qc

    if block_dims is not None:
        x = qc._gather_pooled_blocks(x, block_dims)
    return qc.mx_encode_reference(x, fmt)


def qcomm_mx_decode(
    wire: torch.Tensor,
    numel: int,
    fmt: str,
    block_dims: Optional[List[int]] = None,
    B: Optional[int] = None,
    out: Optional[torch.Tensor] = None,
) -> torch.Tensor:
    """int8 wire -> fp32: the flat [numel] message, or with ``block_dims``
    and ``B`` the [B, sum(block_dims)] matrix whose column blocks it holds.
    ``out`` (contiguous fp32 of that shape) is overwritten when given."""
    if block_dims is not None:
        assert B is not None and numel == B * sum(block_dims), (numel, B, block_dims)
    shape = (numel,) if block_dims is None else (B, numel // max(B, 1))
    assert out is None or tuple(out.shape) == shape, (tuple(out.shape), shape)
    if wire.is_cuda:
        no_table = _mx_no_table(wire.device)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=wire.device)
        if block_dims is None:
            torch.ops.trec_amd.qcomm_mx_decode(wire, out, _MX_FMT_IDS[fmt], no_table, 0)
        else:
            torch.ops.trec_amd.qcomm_mx_decode(
                wire, out, _MX_FMT_IDS[fmt], _mx_col_off(block_dims, wire.device), B
            )
        return out
    from torchrec_amd.distributed import qcomm_codecs as qc

    res = qc.mx_decode_reference(wire, numel, fmt)
    if block_dims is not None:
        res = qc._paste_pooled_blocks(res, B, block_dims)
    return res if out is None else out.copy_(res)


# ------------------------------------------------------------------------
# MXFP8 linear layer for serving (csrc/mx_linear.hip)
# ------------------------------------------------------------------------

MX_LINEAR_K_STEP = 128  # codes are padded to a multiple of this many k
# widest workgroup column tile of the GEMM instantiations (kBigBN); checked
# against the extension's own value on every GPU call
MX_LINEAR_WIDEST_TILE = 128
_MX_OUT_DTYPES = {torch.float32: 0, torch.bfloat16: 1}
_MX_OUT_MXFP8 = 2  # the kernel's output-format code after the two dtypes
# weight element formats (the ids of _MX_FMT_IDS) and the k a code byte holds
_MX_WEIGHT_K_PER_BYTE = {"mxfp8": 1, "mxfp4": 2}


def _mx_weight_format(weight_format: str) -> str:
    if weight_format not in _MX_WEIGHT_K_PER_BYTE:
        raise ValueError(f"mx_linear: unknown weight_format {weight_format!r} ('mxfp8' | 'mxfp4')")
    return weight_format


class MxActivation(NamedTuple):
    """An activation of ``features`` columns handed from one ``mx_linear`` to
    the next in MXFP8, in the layout ``mx_linear_pack_weight`` gives a weight:
    ``codes`` uint8 [M, Kp] (Kp = features rounded up to 128), ``scales`` uint8
    [M, Kp / 32], groups of 32 consecutive features of a row, a ragged last
    group quantized as if padded with zeros, padding groups zero codes with
    scale byte 0, a group holding NaN or Inf zero codes with scale 0xFF."""

    codes: torch.Tensor
    scales: torch.Tensor
    features: int


def _mx_linear_ext() -> None:
    """Requires the extension and that its tiles are the ones stated here."""
    assert hip_ops().mx_linear_widest_tile == MX_LINEAR_WIDEST_TILE


def _mx_rows(t: torch.Tensor, width: int) -> torch.Tensor:
    """fp32 [R, width] with the rows zero-padded from t's width."""
    out = torch.zeros(t.shape[0], width, dtype=torch.float32, device=t.device)
    out[:, : t.shape[1]] = t.float()
    return out


def mx_linear_pack_weight(
    weight: torch.Tensor, weight_format: str = "mxfp8"
) -> Tuple[torch.Tensor, torch.Tensor]:
    """W [N, K] -> (codes uint8 [N, Kp], scales uint8 [N, Kp / 32]): MXFP8
    groups of 32 consecutive k of each row, Kp = K rounded up to 128, a
    ragged last group quantized as if padded with zeros, padding groups zero.
    ``weight_format="mxfp4"``: e2m1 codes uint8 [N, Kp / 2], element 2k in the
    low and 2k + 1 in the high nibble of byte k; scales as for MXFP8."""
    assert weight.dim() == 2 and weight.shape[0] >= 1 and weight.shape[1] >= 1, tuple(weight.shape)
    fmt = _mx_weight_format(weight_format)
    if weight.is_cuda:
        _mx_linear_ext()
        return torch.ops.trec_amd.mx_linear_pack_weight(weight.detach().float(), _MX_FMT_IDS[fmt])
    from torchrec_amd.distributed import qcomm_codecs as qc

    N, K = weight.shape
    Kp = -(-K // MX_LINEAR_K_STEP) * MX_LINEAR_K_STEP
    wire = qc.mx_encode_reference(_mx_rows(weight.detach(), Kp).reshape(-1), fmt)
    return _mx_split(wire, N, Kp, fmt)


def _mx_split(
    wire: torch.Tensor, rows: int, width: int, fmt: str = "mxfp8"
) -> Tuple[torch.Tensor, torch.Tensor]:
    """Reference wire of [rows, width] values -> (codes, scales [rows, width / 32]);
    codes are [rows, width] bytes for MXFP8 and [rows, width / 2] for MXFP4."""
    gb = 32 // _MX_WEIGHT_K_PER_BYTE[fmt]  # code bytes of a group, then its scale byte
    wire = wire.view(torch.uint8).reshape(rows, width // 32, gb + 1)
    codes = wire[:, :, :gb].reshape(rows, width // 32 * gb)
    return codes.contiguous(), wire[:, :, gb].contiguous()


def _mx_dequant(codes: torch.Tensor, scales: torch.Tensor, fmt: str = "mxfp8") -> torch.Tensor:
    """(codes, scales [R, W / 32]) -> fp32 [R, W] through the reference codec."""
    R, G = scales.shape
    wire = torch.cat([codes.reshape(R, G, -1), scales.reshape(R, G, 1)], dim=2)
    from torchrec_amd.distributed import qcomm_codecs as qc

    return qc.mx_decode_reference(wire.reshape(-1).view(torch.int8), R * G * 32, fmt).reshape(
        R, G * 32)


def mx_linear(
    x: Union[torch.Tensor, MxActivation],
    codes: torch.Tensor,
    scales: torch.Tensor,
    bias: Optional[torch.Tensor],
    in_features: int,
    relu: bool = False,
    output_dtype: torch.dtype = torch.float32,
    output_format: Optional[str] = None,
    weight_format: str = "mxfp8",
) -> Union[torch.Tensor, MxActivation]:
    """y = act(Qx(x) Qw(W)^T + b) with both operands in MXFP8 (groups of 32
    consecutive k per row), fp32 accumulation, bias and ReLU on the fp32 sum,
    one rounding to ``output_dtype`` (fp32 or bf16). ``x`` is [..., K] fp32 or
    bf16; ``codes`` / ``scales`` come from ``mx_linear_pack_weight``. With
    ``weight_format="mxfp4"`` they are that function's MXFP4 pair (W4A8: e2m1
    weights against e4m3 activations in the one MFMA); x, the result and an
    ``MxActivation`` on either side are the same as for MXFP8 weights.

    ``x`` may instead be the ``MxActivation`` an earlier call returned: its
    codes and scales are the operand as they stand and nothing is quantized.
    ``output_format="mxfp8"`` returns one: the rounding is then the MXFP8
    quantization of groups of 32 output columns, and ``output_dtype`` is not
    used. The pair is 2-D; leading dimensions are the caller's.

    GPU: the block-scaled MFMA kernel. CPU: the same contract in plain
    PyTorch (reference quantize / dequantize, fp32 matmul)."""
    assert output_dtype in _MX_OUT_DTYPES, f"mx_linear: output_dtype {output_dtype}"
    assert output_format in (None, "mxfp8"), f"mx_linear: output_format {output_format!r}"
    fmt = _mx_weight_format(weight_format)
    K = in_features
    N, Kp = codes.shape[0], -(-K // MX_LINEAR_K_STEP) * MX_LINEAR_K_STEP
    assert codes.shape[1] * _MX_WEIGHT_K_PER_BYTE[fmt] == Kp, (tuple(codes.shape), K, fmt)
    mx_in, mx_out = isinstance(x, MxActivation), output_format == "mxfp8"
    if mx_in:
        assert x.features == K and x.codes.dim() == 2 and x.codes.shape[1] == Kp, (
            x.features, tuple(x.codes.shape), K)
        lead, x2 = x.codes.shape[:1], x.codes
    else:
        assert x.shape[-1] == K, (tuple(x.shape), K)
        lead = x.shape[:-1]
        x2 = x.reshape(-1, K)
        assert not mx_out or x.dim() == 2, "mx_linear: an MXFP8 result is 2-D, flatten x first"
    if x2.is_cuda:
        _mx_linear_ext()
        if not (mx_in or mx_out):
            y = torch.ops.trec_amd.mx_linear_fwd(
                x2, codes, scales, bias, K, relu, _MX_OUT_DTYPES[output_dtype], _MX_FMT_IDS[fmt]
            )
            return y.reshape(*lead, N)
        out = torch.ops.trec_amd.mx_linear_fwd_act(
            x2, x.scales if mx_in else None, codes, scales, bias, K, relu,
            _MX_OUT_MXFP8 if mx_out else _MX_OUT_DTYPES[output_dtype], _MX_FMT_IDS[fmt],
        )
        return MxActivation(out[0], out[1], N) if mx_out else out[0]
    from torchrec_amd.distributed import qcomm_codecs as qc

    if mx_in:
        xq = _mx_dequant(x.codes, x.scales)
    else:
        xq = qc.mx_decode_reference(
            qc.mx_encode_reference(_mx_rows(x2, Kp).reshape(-1), "mxfp8"), x2.shape[0] * Kp, "mxfp8"
        ).reshape(-1, Kp)
    y = xq @ _mx_dequant(codes, scales, fmt).t()
    if bias is not None:
        y = y + bias.float()
    if relu:
        y = torch.relu(y)
    if mx_out:
        Np = -(-N // MX_LINEAR_K_STEP) * MX_LINEAR_K_STEP
        wire = qc.mx_encode_reference(_mx_rows(y, Np).reshape(-1), "mxfp8")
        return MxActivation(*_mx_split(wire, y.shape[0], Np), N)
    return y.to(output_dtype).reshape(*lead, N)
