"""Quantized (rowwise INT8 / INT4 / INT2 / FP8) inference embedding modules.

Reference parity: torchrec/quant/embedding_modules.py
(quant EmbeddingBagCollection :346 with from_float / quantize_state_dict
:217; EmbeddingCollection :748) — backed by the CDNA4 quantized TBE kernels
(ops/csrc/quant_tbe.hip) instead of FBGEMM IntNBit.

Packed row, for bits in {8, 4, 2}: ``[codes: D*bits/8 B][fp16 scale]
[fp16 bias][zero padding]``, stride rounded up to 16 B. Element ``e`` sits in
byte ``e*bits // 8`` at bit ``(e*bits) % 8``, low bits first. ``w = q * scale
+ bias``. The width is a per-table choice (``EmbeddingBagConfig.data_type``);
a module whose tables are all INT8 runs exactly the INT8 kernels.

FP8 row (``DataType.FP8``): ``[e4m3fn codes: D bytes][fp16 scale][2 zero
bytes][zero padding]``, stride ``round_up(D + 4, 16)`` (the INT8 stride),
``D % 4 == 0``. The codes are OCP ``e4m3fn`` (``torch.float8_e4m3fn``), which
gfx950 converts natively, not MI300's ``e4m3fnuz``. There is no bias: e4m3 is
signed. With ``amax = max|x|`` over the row, ``scale_h`` is the smallest fp16
``>= amax / 448`` (round up: ``h = fp16_rne(v)``, and the next fp16 up if
``float(h) < v``), so ``|x| / scale_h <= 448`` and nothing saturates;
``amax == 0`` gives ``scale_h = 0`` and all codes 0. ``code =
e4m3fn_rne(clamp(x / scale, -448, 448))`` with ``scale = float(scale_h)``,
the stored value; the NaN codes 0x7f / 0xff are never produced. ``w =
decode(code) * scale`` in fp32. Inputs are assumed finite with ``amax <=
448 * 65504`` (the scale must fit fp16). The error is relative, at most 2^-4
of each element (2^-10 * scale in e4m3's subnormal range), where INT8's is
absolute.
"""

from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from torchrec_amd import ops
from torchrec_amd.modules.embedding_configs import (
    DATA_TYPE_NUM_BITS,
    DataType,
    EmbeddingBagConfig,
    EmbeddingConfig,
    PoolingType,
)
from torchrec_amd.modules.embedding_modules import (
    EmbeddingBagCollection as FloatEBC,
    EmbeddingCollection as FloatEC,
)
from torchrec_amd.sparse.jagged_tensor import JaggedTensor, KeyedJaggedTensor, KeyedTensor

_QUANT_DATA_TYPES = (DataType.INT8, DataType.INT4, DataType.INT2, DataType.FP8)
# Per-table format code, the values of the ``weight_bits`` tensor handed to the
# n-bit ops: 8 / 4 / 2 are the integer widths; FP8 rows are 8 bits wide too, so
# they carry a code of their own whose low byte is still the width
# (quant_tbe.hip: kFormatFp8).
FP8_FORMAT_CODE = 0x108
# output columns one lane of the n-bit kernels owns, by format code (quant_tbe.hip: CodeUnit)
_LANE_COLS = {8: 4, 4: 8, 2: 8, FP8_FORMAT_CODE: 4}
# output_dtype -> the ops' code (the training TBE's: ops/tbe.py)
_OUT_DTYPE_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
_FP8_MAX = 448.0  # largest finite e4m3fn


def _format_code(data_type: DataType) -> int:
    return FP8_FORMAT_CODE if data_type is DataType.FP8 else DATA_TYPE_NUM_BITS[data_type]


def quant_data_type(data_type: object) -> DataType:
    """The quantized format a table is served at: INT8/INT4/INT2/FP8 (given as
    a DataType or its name) are honoured, anything else means INT8."""
    for dt in _QUANT_DATA_TYPES:
        if data_type is dt or data_type == dt.name:
            return dt
    return DataType.INT8


def int8_row_stride(D: int) -> int:
    return ((D + 4 + 15) // 16) * 16


def _check_nbit_dim(D: int, bits: int) -> None:
    """``bits`` is a format code: 8, 4, 2 or FP8_FORMAT_CODE."""
    if bits == FP8_FORMAT_CODE:
        if D <= 0 or D % 4 != 0:
            raise ValueError(
                f"embedding_dim {D} cannot be packed as FP8: D must be a multiple of 4 "
                f"(a row is a whole number of 32-bit code words)"
            )
        return
    if bits not in (8, 4, 2):
        raise ValueError(f"quantized rows are 8, 4 or 2 bits wide, got {bits}")
    if D <= 0 or (D * bits) % 32 != 0:
        raise ValueError(
            f"embedding_dim {D} cannot be packed at {bits} bits: D*bits must be a "
            f"multiple of 32 (D % {32 // bits} == 0)"
        )


def nbit_row_stride(D: int, bits: int) -> int:
    """Bytes per packed row: codes + fp16 scale + fp16 bias, rounded up to 16."""
    _check_nbit_dim(D, bits)
    return ((D * bits // 8 + 4 + 15) // 16) * 16


def quantize_rowwise_int8(weights: torch.Tensor) -> torch.Tensor:
    """fp32 [R, D] -> packed int8 rows [R, stride] (CPU ref / HIP kernel)."""
    if weights.is_cuda:
        ops.hip_ops()
        return torch.ops.trec_amd.quantize_rowwise_int8(weights)
    R, D = weights.shape
    stride = int8_row_stride(D)
    out = torch.zeros(R, stride, dtype=torch.uint8)
    mn = weights.min(dim=1).values
    mx = weights.max(dim=1).values
    scale = (mx - mn) / 255.0
    inv = torch.where(scale > 0, 1.0 / scale, torch.zeros_like(scale))
    q = ((weights - mn.unsqueeze(1)) * inv.unsqueeze(1) + 0.5).clamp(0, 255).floor()
    out[:, :D] = q.to(torch.uint8)
    sb = torch.stack([scale.half(), mn.half()], dim=1)  # [R, 2] fp16
    out[:, D : D + 4] = sb.view(torch.uint8).reshape(R, 4)
    return out


def dequantize_rowwise_int8(packed: torch.Tensor, D: int) -> torch.Tensor:
    """Packed rows -> fp32 [R, D] using the STORED fp16 scale/bias."""
    R = packed.shape[0]
    q = packed[:, :D].float()
    # a copy: at an odd D the scale sits at an odd byte, which cannot be viewed as fp16
    sb = packed[:, D : D + 4].contiguous().view(torch.float16)
    scale = sb[:, 0].float()
    bias = sb[:, 1].float()
    return q * scale.unsqueeze(1) + bias.unsqueeze(1)


def quantize_rowwise_nbit(weights: torch.Tensor, bits: int) -> torch.Tensor:
    """fp32 [R, D] -> packed ``bits``-wide rows [R, stride] (CPU ref / HIP kernel).

    INT4/INT2 codes are taken against the STORED fp16 scale and bias, so an
    interior value is off by at most half a stored step. ``bits == 8`` is the
    INT8 quantiser, unchanged."""
    R, D = weights.shape
    stride = nbit_row_stride(D, bits)
    if bits == 8:
        return quantize_rowwise_int8(weights)
    if weights.is_cuda:
        ops.hip_ops()
        return torch.ops.trec_amd.quantize_rowwise_nbit(weights, bits)
    levels = (1 << bits) - 1
    code_bytes = D * bits // 8
    mn = weights.min(dim=1).values
    mx = weights.max(dim=1).values
    scale_h = ((mx - mn) / float(levels)).half()
    bias_h = mn.half()
    scale = scale_h.float().unsqueeze(1)
    bias = bias_h.float().unsqueeze(1)
    q = torch.floor((weights - bias) / scale + 0.5).clamp(0, levels)
    q = torch.where(scale == 0, torch.zeros_like(q), q).to(torch.uint8)
    per_byte = 8 // bits
    shifts = torch.arange(per_byte, dtype=torch.uint8) * bits
    codes = (q.reshape(R, code_bytes, per_byte) << shifts).sum(dim=2).to(torch.uint8)
    out = torch.zeros(R, stride, dtype=torch.uint8)
    out[:, :code_bytes] = codes
    sb = torch.stack([scale_h, bias_h], dim=1)  # [R, 2] fp16
    out[:, code_bytes : code_bytes + 4] = sb.view(torch.uint8).reshape(R, 4)
    return out


def unpack_codes_nbit(packed: torch.Tensor, D: int, bits: int) -> torch.Tensor:
    """Packed rows -> the integer codes, uint8 [R, D]."""
    _check_nbit_dim(D, bits)
    R = packed.shape[0]
    code_bytes = D * bits // 8
    per_byte = 8 // bits
    shifts = torch.arange(per_byte, dtype=torch.uint8, device=packed.device) * bits
    codes = (packed[:, :code_bytes].unsqueeze(2) >> shifts) & ((1 << bits) - 1)
    return codes.reshape(R, D)


def dequantize_rowwise_nbit(packed: torch.Tensor, D: int, bits: int) -> torch.Tensor:
    """Packed ``bits``-wide rows -> fp32 [R, D] using the stored fp16 scale/bias."""
    R = packed.shape[0]
    code_bytes = D * bits // 8
    q = unpack_codes_nbit(packed, D, bits).float()
    sb = packed[:, code_bytes : code_bytes + 4].reshape(R, 2, 2).view(torch.float16)
    sb = sb.reshape(R, 2)
    scale = sb[:, 0].float()
    bias = sb[:, 1].float()
    return q * scale.unsqueeze(1) + bias.unsqueeze(1)


def fp8_row_stride(D: int) -> int:
    """Bytes per packed FP8 row: D codes + fp16 scale + 2 reserved bytes,
    rounded up to 16 (the INT8 stride)."""
    _check_nbit_dim(D, FP8_FORMAT_CODE)
    return int8_row_stride(D)


def _fp16_round_up(v: torch.Tensor) -> torch.Tensor:
    """Smallest fp16 >= v for finite fp32 v >= 0: round to nearest, then step
    up once where that fell short (the HIP kernel does the same)."""
    h = v.half()
    short = h.float() < v
    return (h.view(torch.int16) + short.to(torch.int16)).view(torch.float16)


def quantize_rowwise_fp8(weights: torch.Tensor) -> torch.Tensor:
    """fp32 [R, D] -> packed FP8 rows [R, stride] (CPU ref / HIP kernel); the
    format and its assumptions are in the module docstring."""
    R, D = weights.shape
    stride = fp8_row_stride(D)
    if weights.is_cuda:
        ops.hip_ops()
        return torch.ops.trec_amd.quantize_rowwise_fp8(weights)
    w = weights.float()
    scale_h = _fp16_round_up(w.abs().amax(dim=1) / _FP8_MAX)
    scale = scale_h.float().unsqueeze(1)
    r = (w / scale).clamp(-_FP8_MAX, _FP8_MAX)
    r = torch.where(scale == 0, torch.zeros_like(r), r)
    out = torch.zeros(R, stride, dtype=torch.uint8)
    out[:, :D] = r.to(torch.float8_e4m3fn).view(torch.uint8)
    out[:, D : D + 2] = scale_h.view(torch.uint8).reshape(R, 2)
    return out


def dequantize_rowwise_fp8(packed: torch.Tensor, D: int) -> torch.Tensor:
    """Packed FP8 rows -> fp32 [R, D]: decode(code) * the stored fp16 scale."""
    R = packed.shape[0]
    codes = packed[:, :D].contiguous().view(torch.float8_e4m3fn).float()
    scale = packed[:, D : D + 2].contiguous().view(torch.float16).float()
    return codes * scale.reshape(R, 1)


class QuantTableBatchedEmbeddingBags(nn.Module):
    """Inference-only quantized TBE (pooled). Flat packed buffer, per-table byte
    offsets and per-table format (``weight_dtypes``: INT8/INT4/INT2/FP8, None =
    all INT8). GPU path = tbe_forward_pooled_int8 when every table is INT8, else
    tbe_forward_pooled_nbit (one launch for mixed formats); CPU path = dequant
    reference. ``output_dtype`` (fp32 / bf16 / fp16) is the dtype of every
    lookup's result: the arithmetic is fp32 and the value is rounded once.

    ``bounds_check`` / ``index_remapping`` (checking; off by default). With
    checking on, every lookup first runs ``quant_tbe_remap_indices`` (one HIP
    launch, no host read, capturable in a graph) over its ids and hands the
    result, a new int64 tensor, to the unchanged lookup op; the caller's ids
    are never written. An id outside ``[0, logical rows)`` of its table is
    dropped and counted (``out_of_range_counts()``); it is NOT clamped, which
    would serve another item's embedding. ``index_remapping[t]`` (int32/int64
    ``[logical_rows]``, values in ``[-1, rows)``) serves a pruned table:
    ``specs[t][1]`` stays the physical row count, the logical id space is
    ``len(index_remapping[t])``, and an id mapped to -1 is dropped without
    being counted. A remap on any table turns checking on. A dropped id
    contributes zero to a pooled lookup (MEAN still divides by the full bag
    length, the reference's semantics for pruned ids) and is a zero row of a
    sequence lookup. Per-sample weights are assumed finite: a dropped id is
    ``weight * 0``, and ``NaN * 0`` is NaN.

    Layout with checking on: each table is ``[one all-zero row][rows...]`` and
    the table's byte offset points past the zero row, so the lookup kernels
    (signed 64-bit ``id * stride``) read id -1 as zero bytes, which dequantise
    to 0 in every format. ``qweights`` is ``sum(stride_t)`` bytes larger than
    an unchecked module's, ``packed_table(i)`` is still the ``[rows, stride]``
    view without the zero row, and no zero row is ever written. A checked and
    an unchecked module do not exchange ``state_dict``s (the buffer sizes
    differ, and a pruned module also carries ``index_remap``). A module built
    without checking has the byte layout, ``state_dict``, launches and results
    it had before these arguments existed."""

    def __init__(
        self,
        specs: List[Tuple[str, int, int]],  # (name, rows, dim)
        feature_table_map: Optional[List[int]] = None,
        pooling: PoolingType = PoolingType.SUM,
        device: Optional[torch.device] = None,
        location: str = "device",  # "device" (HBM) | "managed" (pinned host, QUANT_UVM)
        weight_dtypes: Optional[List[DataType]] = None,
        output_dtype: torch.dtype = torch.float32,
        bounds_check: bool = False,
        index_remapping: Optional[List[Optional[torch.Tensor]]] = None,
    ) -> None:
        super().__init__()
        if output_dtype not in _OUT_DTYPE_CODE:
            raise ValueError(
                f"output_dtype must be torch.float32, torch.bfloat16 or torch.float16, "
                f"got {output_dtype}"
            )
        self.output_dtype = output_dtype
        self._out_dtype_code = _OUT_DTYPE_CODE[output_dtype]
        device = device or torch.device("cpu")
        self._uvm = location == "managed" and device.type == "cuda"
        qdevice = torch.device("cpu") if self._uvm else device
        self._specs = specs
        T = len(specs)
        if weight_dtypes is None:
            weight_dtypes = [DataType.INT8] * T
        if len(weight_dtypes) != T:
            raise ValueError(f"weight_dtypes has {len(weight_dtypes)} entries for {T} tables")
        for dt in weight_dtypes:
            if dt not in _QUANT_DATA_TYPES:
                raise ValueError(f"quantized tables are INT8, INT4, INT2 or FP8, got {dt}")
        self._weight_dtypes = list(weight_dtypes)
        self._bits = [DATA_TYPE_NUM_BITS[dt] for dt in weight_dtypes]
        # what the n-bit ops switch on: the width, or FP8_FORMAT_CODE
        self._formats = [_format_code(dt) for dt in weight_dtypes]
        self._all_int8 = all(dt is DataType.INT8 for dt in weight_dtypes)
        if not self._all_int8:
            for (name, _, dim), b in zip(specs, self._formats):
                try:
                    _check_nbit_dim(dim, b)
                except ValueError as e:
                    raise ValueError(f"table {name}: {e}") from None
        self._feature_table_map = feature_table_map or list(range(T))
        F = len(self._feature_table_map)
        self._num_features = F
        self.pooling = pooling
        remaps = self._check_index_remapping(specs, index_remapping)
        self._checked = bool(bounds_check) or any(r is not None for r in remaps)
        self._has_remap = any(r is not None for r in remaps)
        self._logical_rows = [
            rows if r is None else r.numel() for (_, rows, _), r in zip(specs, remaps)
        ]
        # table_starts[t] is where table t's rows begin; with checking on an
        # all-zero row sits in front of them (row -1 of the table)
        table_starts = []
        end = 0
        for (_, rows, dim), b in zip(specs, self._formats):
            stride = self._stride(dim, b)
            start = end + (stride if self._checked else 0)
            table_starts.append(start)
            end = start + rows * stride
        byte_offsets = table_starts + [end]
        dims = [s[2] for s in specs]
        feat_dims = [dims[t] for t in self._feature_table_map]
        d_out = [0]
        for d in feat_dims:
            d_out.append(d_out[-1] + d)
        self._total_D = d_out[-1]
        self._max_D = max(dims) if dims else 0
        # widest row in lane units, what the n-bit launch is sized by: a lane
        # owns 4 columns of an INT8 or FP8 row and 8 of an INT4 or INT2 row
        self._max_units = max(
            (d // _LANE_COLS[b] for d, b in zip(dims, self._formats)), default=0
        )
        qw = torch.zeros(byte_offsets[-1], dtype=torch.uint8, device=qdevice)
        if getattr(self, "_uvm", False):
            qw = qw.pin_memory()
        self.register_buffer("qweights", qw)
        reg = lambda n, t: self.register_buffer(n, t.to(device), persistent=False)
        reg("_table_byte_offsets", torch.tensor(byte_offsets[:-1], dtype=torch.int64))
        reg("_dims_t", torch.tensor(dims, dtype=torch.int32))
        reg("_weight_bits_t", torch.tensor(self._formats, dtype=torch.int32))
        reg("_feat_table_t", torch.tensor(self._feature_table_map, dtype=torch.int32))
        reg("_d_out_offsets", torch.tensor(d_out, dtype=torch.int64))
        reg("_empty_f", torch.empty(0, dtype=torch.float32))
        if self._checked:
            remap_offsets, flat, n = [], [], 0
            for r in remaps:
                remap_offsets.append(-1 if r is None else n)
                if r is not None:
                    flat.append(r.to(torch.int32).cpu())
                    n += r.numel()
            reg("_logical_rows_t", torch.tensor(self._logical_rows, dtype=torch.int64))
            reg("_remap_offsets_t", torch.tensor(remap_offsets, dtype=torch.int64))
            reg("_table_ids_t", torch.arange(T, dtype=torch.int32))
            reg("_oob_counts", torch.zeros(T, dtype=torch.int64))
            if self._has_remap:
                # part of the served model: persistent, and registered only
                # here, so the state_dict of a module without a remap is the
                # one it always had
                self.register_buffer("index_remap", torch.cat(flat).to(device))
            else:
                reg("_empty_i32", torch.empty(0, dtype=torch.int32))

    @staticmethod
    def _check_index_remapping(
        specs: List[Tuple[str, int, int]],
        index_remapping: Optional[List[Optional[torch.Tensor]]],
    ) -> List[Optional[torch.Tensor]]:
        """Host-side validation at construction: one entry per table, each
        None or an int32/int64 [logical_rows] tensor with values in [-1, rows)."""
        if index_remapping is None:
            return [None] * len(specs)
        if len(index_remapping) != len(specs):
            raise ValueError(
                f"index_remapping has {len(index_remapping)} entries for {len(specs)} tables"
            )
        out: List[Optional[torch.Tensor]] = []
        for (name, rows, _), r in zip(specs, index_remapping):
            if r is None:
                out.append(None)
                continue
            if not isinstance(r, torch.Tensor) or r.dtype not in (torch.int32, torch.int64):
                raise ValueError(
                    f"table {name}: index_remapping must be an int32 or int64 tensor, got "
                    f"{getattr(r, 'dtype', type(r))}"
                )
            if r.dim() != 1:
                raise ValueError(
                    f"table {name}: index_remapping must be 1-D [logical_rows], got "
                    f"{tuple(r.shape)}"
                )
            r = r.detach().cpu()
            if r.numel() and (int(r.min()) < -1 or int(r.max()) >= rows):
                raise ValueError(
                    f"table {name}: index_remapping values must lie in [-1, {rows}) "
                    f"(rows = the table's physical row count), got [{int(r.min())}, "
                    f"{int(r.max())}]"
                )
            out.append(r)
        return out

    def _remap(self) -> torch.Tensor:
        return self.index_remap if self._has_remap else self._empty_i32

    def _remap_indices(
        self, indices: torch.Tensor, seg_offsets: torch.Tensor, seg_stride: int,
        feat_table: torch.Tensor,
    ) -> torch.Tensor:
        """GPU: logical ids -> physical rows, -1 for a dropped id (a new tensor)."""
        if indices.numel() == 0:
            return indices
        return torch.ops.trec_amd.quant_tbe_remap_indices(
            indices,
            seg_offsets,
            seg_stride,
            feat_table,
            self._logical_rows_t,
            self._remap_offsets_t,
            self._remap(),
            self._oob_counts,
        )

    def _map_ids_cpu(self, t: int, idx: torch.Tensor) -> torch.Tensor:
        """CPU: the same mapping for ids of table ``t``, in torch."""
        idx = idx.to(torch.int64)
        ok = (idx >= 0) & (idx < self._logical_rows[t])
        self._oob_counts[t] += int((~ok).sum())
        ro = int(self._remap_offsets_t[t])
        if ro >= 0:
            seg = self.index_remap[ro : ro + self._logical_rows[t]].to(torch.int64)
            mapped = seg[torch.where(ok, idx, torch.zeros_like(idx))]
        else:
            mapped = idx
        return torch.where(ok, mapped, torch.full_like(idx, -1))

    def _cpu_lookup_table(self, t: int) -> torch.Tensor:
        """fp32 table for the CPU reference; with checking on a zero row is
        appended, which is where id -1 (a dropped id) indexes."""
        w = self.dequantized_table(t)
        if self._checked:
            w = torch.cat([w, w.new_zeros(1, w.shape[1])])
        return w

    def out_of_range_counts(self) -> torch.Tensor:
        """Cumulative int64 [T]: ids outside ``[0, logical rows)`` seen per
        table by lookups (and by ``update_rows`` of a pruned module) since
        construction or the last reset. Pruned ids are not counted. The
        tensor lives on the device and reading it here syncs nothing."""
        if not self._checked:
            raise RuntimeError("this module was built without bounds_check / index_remapping")
        return self._oob_counts

    def reset_out_of_range_counts(self) -> None:
        self.out_of_range_counts().zero_()

    @staticmethod
    def _stride(dim: int, bits: int) -> int:
        # ``bits`` is a format code. INT8 keeps its own stride rule (no dim
        # check: CPU lookups of odd dims keep working as before)
        if bits == FP8_FORMAT_CODE:
            return fp8_row_stride(dim)
        return int8_row_stride(dim) if bits == 8 else nbit_row_stride(dim, bits)

    def load_float_table(self, i: int, weights: torch.Tensor) -> None:
        name, rows, dim = self._specs[i]
        if self._checked and tuple(weights.shape) != (rows, dim):
            # a longer table would run into the next table's zero row
            raise ValueError(
                f"table {name} holds [{rows}, {dim}] rows, got {tuple(weights.shape)}"
            )
        packed = self._quantize_rows(i, weights.to(self.qweights.device).float())
        start = int(self._table_byte_offsets[i])
        self.qweights[start : start + packed.numel()].copy_(packed.reshape(-1))

    def packed_table(self, i: int) -> torch.Tensor:
        name, rows, dim = self._specs[i]
        start = int(self._table_byte_offsets[i])
        stride = self._stride(dim, self._formats[i])
        return self.qweights[start : start + rows * stride].view(rows, stride)

    def _code_bytes(self, i: int) -> int:
        return self._specs[i][2] * self._bits[i] // 8

    def _quantize_rows(self, i: int, w: torch.Tensor) -> torch.Tensor:
        """fp32 [n, dim] -> packed rows in table ``i``'s format (its own quantiser)."""
        if self._formats[i] == FP8_FORMAT_CODE:
            return quantize_rowwise_fp8(w)
        if self._bits[i] == 8:
            return quantize_rowwise_int8(w)
        return quantize_rowwise_nbit(w, self._bits[i])

    def _update_meta(
        self, counts: Tuple[int, ...], windows: Tuple[Tuple[int, int], ...]
    ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """(row_lo, row_hi, upd_offsets, val_offsets) on the device, built from
        shapes alone and cached, so a repeated update of the same shape
        uploads nothing (and can be captured in a graph after one warm-up)."""
        dev = self._dims_t.device
        key = (counts, windows, dev)
        cache = self.__dict__.setdefault("_update_meta_cache", {})
        meta = cache.get(key)
        if meta is None:
            upd, val = [0], []
            v = 0
            for n, (_, _, dim) in zip(counts, self._specs):
                upd.append(upd[-1] + n)
                val.append(v)
                v += n * dim
            i64 = lambda xs: torch.tensor(xs, dtype=torch.int64).to(dev)
            meta = (
                i64([w[0] for w in windows]),
                i64([w[1] for w in windows]),
                i64(upd),
                i64(val),
            )
            if len(cache) >= 64:
                cache.clear()
            cache[key] = meta
        return meta

    @torch.no_grad()
    def update_rows(
        self,
        updates: Dict[int, Tuple[torch.Tensor, torch.Tensor]],
        row_windows: Optional[List[Tuple[int, int]]] = None,
    ) -> torch.Tensor:
        """Requantise rows of the served tables in place from float rows.

        ``updates[t] = (ids [n], rows [n, dim])`` for table index ``t``; rows
        of any float dtype are converted to fp32. ``row_windows[t] = (lo, hi)``
        (default ``(0, rows)``) is the range of ids this module holds for
        table ``t``: an entry with id ``r`` is applied only if ``lo <= r <
        hi``, to local row ``r - lo``, and every other entry is dropped (on
        the device, with no host sync). ``(0, rows)`` bounds-checks an
        unsharded table; a shard passes its own global row range, so every
        rank takes the same full delta and keeps its rows. An id whose local
        row lies past the table is dropped as well. Returns int64 [T]: the
        number of entries applied per table.

        Contract (GPU: ``quant_tbe_update_rows``, one HIP kernel, one wave per
        entry, current stream, pinned-host ``location="managed"`` tables
        included; CPU: the CPU quantisers):

        * the first ``code_bytes + 4`` bytes of an applied row are exactly
          what the table's own quantiser (``quantize_rowwise_int8`` for INT8,
          any ``D``; ``quantize_rowwise_nbit`` for INT4/INT2;
          ``quantize_rowwise_fp8`` for FP8) writes for that fp32 row;
        * no other byte of ``qweights`` changes: not the row's padding, not
          its neighbours, not another table;
        * ids within one table's segment must be unique (the model tracker's
          ``UniqueRows`` are); duplicates with different values are undefined
          on the GPU;
        * the update is ordered against lookups on the same stream only. A
          lookup running concurrently on another stream may see a row whose
          codes and scale come from different versions: serialising the
          streams is the caller's job.

        On a module built with checking the zero rows are never written:
        every window is clamped to ``0 <= lo`` and ``hi <= lo + rows``. On a
        module with an ``index_remapping`` the ids are LOGICAL ids: they go
        through ``quant_tbe_remap_indices`` first (the segments are the
        tables), an entry for a pruned or out-of-range id is dropped and not
        counted as applied, out-of-range ones add to
        ``out_of_range_counts()``, and the windows apply to the physical rows.

        Shapes are validated on the host; id values are not (that would need
        a host sync). Nothing here reads a device value on the host, so an
        update whose shapes were seen once before can be captured in a graph.
        """
        T = len(self._specs)
        for t in updates:
            if not isinstance(t, int) or not 0 <= t < T:
                raise IndexError(f"update_rows: table index {t!r} is not in [0, {T})")
        if row_windows is None:
            row_windows = [(0, rows) for _, rows, _ in self._specs]
        if len(row_windows) != T:
            raise ValueError(f"row_windows has {len(row_windows)} entries for {T} tables")
        windows = tuple((int(lo), int(hi)) for lo, hi in row_windows)
        if self._checked:
            windows = tuple(
                (max(lo, 0), min(hi, max(lo, 0) + rows))
                for (lo, hi), (_, rows, _) in zip(windows, self._specs)
            )
        on_gpu = self.qweights.is_cuda or self._uvm
        dev = self._dims_t.device if on_gpu else self.qweights.device
        ids_l: List[torch.Tensor] = []
        rows_l: List[torch.Tensor] = []
        counts: List[int] = []
        for t, (name, _, dim) in enumerate(self._specs):
            if t not in updates:
                counts.append(0)
                continue
            ids, rows = updates[t]
            if ids.dim() != 1 or tuple(rows.shape) != (ids.numel(), dim):
                raise ValueError(
                    f"update_rows: table {name} takes ids [n] and rows [n, {dim}], got "
                    f"{tuple(ids.shape)} and {tuple(rows.shape)}"
                )
            if not rows.is_floating_point():
                raise ValueError(f"update_rows: table {name}: rows must be a float tensor")
            counts.append(ids.numel())
            ids_l.append(ids.to(device=dev, dtype=torch.int64))
            rows_l.append(rows.to(device=dev, dtype=torch.float32))
        if on_gpu:
            ops.hip_ops()
            row_lo, row_hi, upd_offsets, val_offsets = self._update_meta(tuple(counts), windows)
            if ids_l:
                upd_rows = torch.cat(ids_l) if len(ids_l) > 1 else ids_l[0].contiguous()
                values = (
                    torch.cat([r.reshape(-1) for r in rows_l])
                    if len(rows_l) > 1
                    else rows_l[0].contiguous().reshape(-1)
                )
            else:
                upd_rows = torch.empty(0, dtype=torch.int64, device=dev)
                values = torch.empty(0, dtype=torch.float32, device=dev)
            if self._has_remap:
                upd_rows = self._remap_indices(upd_rows, upd_offsets, 1, self._table_ids_t)
            return torch.ops.trec_amd.quant_tbe_update_rows(
                self.qweights,
                self._table_byte_offsets,
                self._dims_t,
                self._weight_bits_t,
                row_lo,
                row_hi,
                upd_offsets,
                upd_rows,
                values,
                val_offsets,
            )
        # CPU: the same contract with the CPU quantisers
        applied = torch.zeros(T, dtype=torch.int64)
        k = 0
        for t, n in enumerate(counts):
            if t not in updates:
                continue
            ids, rows = ids_l[k], rows_l[k]
            k += 1
            lo, hi = windows[t]
            if self._has_remap:
                ids = self._map_ids_cpu(t, ids)
            local = ids - lo
            keep = (ids >= lo) & (ids < hi) & (local < self._specs[t][1])
            applied[t] = int(keep.sum())
            if applied[t] == 0:
                continue
            nb = self._code_bytes(t) + 4
            packed = self._quantize_rows(t, rows[keep])
            self.packed_table(t)[local[keep], :nb] = packed[:, :nb]
        return applied

    def dequantized_table(self, i: int) -> torch.Tensor:
        """fp32 [rows, dim] of table ``i`` from its packed bytes."""
        name, rows, dim = self._specs[i]
        if self._formats[i] == FP8_FORMAT_CODE:
            return dequantize_rowwise_fp8(self.packed_table(i), dim)
        if self._bits[i] == 8:
            return dequantize_rowwise_int8(self.packed_table(i), dim)
        return dequantize_rowwise_nbit(self.packed_table(i), dim, self._bits[i])

    @torch.no_grad()
    def forward(
        self,
        indices: torch.Tensor,
        offsets: torch.Tensor,
        per_sample_weights: Optional[torch.Tensor] = None,
    ) -> torch.Tensor:
        B = (offsets.numel() - 1) // self._num_features
        if self.qweights.is_cuda or (self.qweights.is_pinned() and indices.is_cuda):
            ops.hip_ops()
            if self._checked:
                indices = self._remap_indices(indices, offsets, max(B, 1), self._feat_table_t)
            if not self._all_int8:
                return torch.ops.trec_amd.tbe_forward_pooled_nbit(
                    self.qweights,
                    self._table_byte_offsets,
                    self._dims_t,
                    self._weight_bits_t,
                    self._feat_table_t,
                    self._d_out_offsets,
                    indices,
                    offsets,
                    per_sample_weights if per_sample_weights is not None else self._empty_f,
                    B,
                    self._total_D,
                    self._max_units,
                    self.pooling == PoolingType.MEAN,
                    self._out_dtype_code,
                )
            return torch.ops.trec_amd.tbe_forward_pooled_int8(
                self.qweights,
                self._table_byte_offsets,
                self._dims_t,
                self._feat_table_t,
                self._d_out_offsets,
                indices,
                offsets,
                per_sample_weights if per_sample_weights is not None else self._empty_f,
                B,
                self._total_D,
                self._max_D,
                self.pooling == PoolingType.MEAN,
                self._out_dtype_code,
            )
        # CPU reference
        outs = []
        for f, t in enumerate(self._feature_table_map):
            w = self._cpu_lookup_table(t)
            off = offsets[f * B : (f + 1) * B + 1] - offsets[f * B]
            idx = indices[int(offsets[f * B]) : int(offsets[(f + 1) * B])]
            if self._checked:
                idx = self._map_ids_cpu(t, idx)
                idx = torch.where(idx < 0, torch.full_like(idx, w.shape[0] - 1), idx)
            pw = (
                per_sample_weights[int(offsets[f * B]) : int(offsets[(f + 1) * B])]
                if per_sample_weights is not None
                else None
            )
            mean = self.pooling == PoolingType.MEAN
            if mean and pw is not None:
                # embedding_bag has no weighted mean; the kernels compute the
                # weighted sum over the bag length
                pooled = torch.nn.functional.embedding_bag(
                    idx, w, off, mode="sum", per_sample_weights=pw, include_last_offset=True
                )
                n = (off[1:] - off[:-1]).clamp(min=1).to(pooled.dtype)
                outs.append(pooled / n.unsqueeze(1))
                continue
            outs.append(
                torch.nn.functional.embedding_bag(
                    idx,
                    w,
                    off,
                    mode="mean" if mean else "sum",
                    per_sample_weights=pw,
                    include_last_offset=True,
                )
            )
        return self.to_output_dtype(torch.cat(outs, dim=1))

    def to_output_dtype(self, x: torch.Tensor) -> torch.Tensor:
        """The one rounding of an fp32 CPU-reference result to ``output_dtype``."""
        return x if x.dtype == self.output_dtype else x.to(self.output_dtype)

    @torch.no_grad()
    def forward_sequence(
        self, indices: torch.Tensor, feat_val_offsets: torch.Tensor, dim: int
    ) -> torch.Tensor:
        """GPU per-row lookup [N, dim]: tbe_forward_seq_int8 when every table is
        INT8, else tbe_forward_seq_nbit. ``feat_val_offsets`` is [F+1]. A
        module whose tables are on the CPU answers from the dequantised tables."""
        if not (self.qweights.is_cuda or (self.qweights.is_pinned() and indices.is_cuda)):
            return self.to_output_dtype(self._sequence_rows_cpu(indices, feat_val_offsets, dim))
        ops.hip_ops()
        if self._checked:
            indices = self._remap_indices(indices, feat_val_offsets, 1, self._feat_table_t)
        if not self._all_int8:
            return torch.ops.trec_amd.tbe_forward_seq_nbit(
                self.qweights,
                self._table_byte_offsets,
                self._dims_t,
                self._weight_bits_t,
                self._feat_table_t,
                feat_val_offsets,
                indices,
                dim,
                self._max_units,
                self._out_dtype_code,
            )
        return torch.ops.trec_amd.tbe_forward_seq_int8(
            self.qweights,
            self._table_byte_offsets,
            self._dims_t,
            self._feat_table_t,
            feat_val_offsets,
            indices,
            dim,
            self._max_D,
            self._out_dtype_code,
        )


    def _sequence_rows_cpu(
        self, indices: torch.Tensor, feat_val_offsets: torch.Tensor, dim: int
    ) -> torch.Tensor:
        """CPU reference of the sequence lookup, fp32 [N, dim]."""
        fvo = feat_val_offsets.tolist()
        rows_l = []
        for f, t in enumerate(self._feature_table_map):
            idx = indices[fvo[f] : fvo[f + 1]]
            if idx.numel() == 0:
                continue
            if self._checked:
                idx = self._map_ids_cpu(t, idx)  # -1 indexes the appended zero row
            rows_l.append(self._cpu_lookup_table(t)[idx])
        return torch.cat(rows_l, dim=0) if rows_l else torch.empty(0, dim)


def delta_ids_rows(name: str, entry: object) -> Tuple[torch.Tensor, torch.Tensor]:
    """One table's entry of a model delta, a ``UniqueRows`` (model tracker) or
    an ``(ids, rows)`` pair, as ``(ids, rows)``."""
    if isinstance(entry, (tuple, list)):
        ids, rows = entry
    else:
        ids, rows = entry.ids, entry.rows
    if rows is None:
        raise ValueError(
            f"table {name}: the delta carries ids but no rows. Track with "
            f"UpdateMode.FIRST or UpdateMode.LAST: UpdateMode.NONE records ids only"
        )
    return ids, rows


def check_delta_tables(delta: Dict[str, object], served: List[str], module: str) -> None:
    unknown = [n for n in delta if n not in served]
    if unknown:
        raise KeyError(f"{module} serves no table named {unknown}; it serves {list(served)}")


def update_tbe_from_delta(
    tbe: QuantTableBatchedEmbeddingBags,
    delta: Dict[str, object],
    row_windows: Optional[List[Tuple[int, int]]] = None,
) -> Dict[str, torch.Tensor]:
    """Apply the entries of ``delta`` whose table ``tbe`` holds (the others are
    not its business); returns table name -> applied count (int64 scalar)."""
    updates = {
        i: delta_ids_rows(name, delta[name])
        for i, (name, _, _) in enumerate(tbe._specs)
        if name in delta
    }
    if not updates:
        return {}
    applied = tbe.update_rows(updates, row_windows)
    return {tbe._specs[i][0]: applied[i] for i in updates}


def _resolve_weight_dtype(
    name: str,
    weight_dtype: DataType,
    per_table_weight_dtype: Optional[Dict[str, DataType]],
) -> DataType:
    dt = (per_table_weight_dtype or {}).get(name, weight_dtype)
    if dt not in _QUANT_DATA_TYPES:
        raise ValueError(
            f"table {name}: quantized tables are INT8, INT4, INT2 or FP8, got {dt}"
        )
    return dt


def _remap_physical_rows(name: str, remap: object, logical: Optional[int]) -> int:
    """The physical row count a table's remap addresses, ``max + 1``, after
    the checks that need no table: an int32/int64 [logical] tensor, no value
    below -1."""
    if not isinstance(remap, torch.Tensor) or remap.dtype not in (torch.int32, torch.int64):
        raise ValueError(
            f"table {name}: index_remapping must be an int32 or int64 tensor, got "
            f"{getattr(remap, 'dtype', type(remap))}"
        )
    if remap.dim() != 1 or (logical is not None and remap.numel() != logical):
        raise ValueError(
            f"table {name}: index_remapping must have one entry per logical id "
            f"([{logical}]), got {tuple(remap.shape)}"
        )
    if remap.numel() == 0:
        return 0
    if int(remap.min()) < -1:
        raise ValueError(
            f"table {name}: index_remapping values must be -1 (pruned) or a physical "
            f"row, got {int(remap.min())}"
        )
    return int(remap.max()) + 1


def _tbe_pruning_args(
    tables: List[object], index_remapping: Optional[Dict[str, torch.Tensor]], module: str
) -> Tuple[List[Tuple[str, int, int]], Optional[List[Optional[torch.Tensor]]]]:
    """(specs with PHYSICAL row counts, per-table remaps or None) for the TBE
    behind a quant EBC / EC. ``num_embeddings`` is the logical id space, so a
    remap has that many entries; ``num_embeddings_post_pruning``, where set,
    must be the remap's physical row count."""
    index_remapping = index_remapping or {}
    unknown = [n for n in index_remapping if n not in [t.name for t in tables]]
    if unknown:
        raise KeyError(f"index_remapping names {unknown}, which {module} does not serve")
    specs, remaps = [], []
    for t in tables:
        r = index_remapping.get(t.name)
        post = getattr(t, "num_embeddings_post_pruning", None)
        if r is None:
            if post is not None and post != t.num_embeddings:
                raise ValueError(
                    f"table {t.name}: num_embeddings_post_pruning={post} of "
                    f"{t.num_embeddings} rows needs an index_remapping"
                )
            rows = t.num_embeddings
        else:
            rows = _remap_physical_rows(t.name, r, t.num_embeddings)
            if post is not None and post != rows:
                raise ValueError(
                    f"table {t.name}: num_embeddings_post_pruning={post} but its "
                    f"index_remapping addresses {rows} physical rows"
                )
            if post is not None:
                rows = post
        specs.append((t.name, rows, t.embedding_dim))
        remaps.append(r)
    return specs, (remaps if any(r is not None for r in remaps) else None)


def _float_rows_for_remap(name: str, weight: torch.Tensor, remap: torch.Tensor) -> torch.Tensor:
    """The physical rows of a pruned table from its float table. A float table
    with ``len(remap)`` rows is logical: physical row ``j`` is the float row
    of the one id mapped to ``j``. One with the physical row count is taken
    as it is (many ids may share a row: the in-training pruning case)."""
    rows = _remap_physical_rows(name, remap, None)
    n = weight.shape[0]
    if n == remap.numel():
        r = remap.to(torch.int64).cpu()
        kept = (r >= 0).nonzero().flatten()
        per_row = torch.bincount(r[kept], minlength=rows)
        if bool((per_row != 1).any()):
            j = int((per_row != 1).nonzero()[0])
            raise ValueError(
                f"table {name}: the float table is logical ({n} rows), so every physical "
                f"row needs exactly one id, but row {j} has {int(per_row[j])}"
            )
        src = torch.empty(rows, dtype=torch.int64)
        src[r[kept]] = kept
        return weight[src.to(weight.device)]
    if n == rows:
        return weight
    raise ValueError(
        f"table {name}: the float table has {n} rows, neither the remap's logical "
        f"{remap.numel()} nor its physical {rows}"
    )


def _quant_configs_for_remap(tables: List[object], index_remapping: Dict[str, torch.Tensor]):
    """from_float: a remapped table's config gets the logical id space and the
    physical row count of its remap."""
    out = []
    for t in tables:
        r = index_remapping.get(t.name)
        if r is not None:
            rows = _remap_physical_rows(t.name, r, None)
            post = getattr(t, "num_embeddings_post_pruning", None)
            if post is not None and post != rows:
                raise ValueError(
                    f"table {t.name}: num_embeddings_post_pruning={post} but its "
                    f"index_remapping addresses {rows} physical rows"
                )
            t = dataclasses.replace(
                t,
                num_embeddings=r.numel(),
                num_embeddings_post_pruning=_remap_physical_rows(t.name, r, None),
            )
        out.append(t)
    return out


class EmbeddingBagCollection(nn.Module):
    """Quantized EBC (reference quant/embedding_modules.py:346). Each table is
    served at its config's ``data_type`` when that is INT8/INT4/INT2/FP8, else INT8.

    ``bounds_check`` and ``index_remapping`` (table name -> int32/int64
    ``[num_embeddings]`` tensor of physical rows, -1 = pruned) are
    ``QuantTableBatchedEmbeddingBags``'s arguments by table name:
    ``num_embeddings`` stays the logical id space and
    ``num_embeddings_post_pruning``, where set, must be the remap's physical
    row count (``max + 1``)."""

    def __init__(
        self,
        tables: List[EmbeddingBagConfig],
        is_weighted: bool = False,
        device: Optional[torch.device] = None,
        output_dtype: torch.dtype = torch.float32,
        bounds_check: bool = False,
        index_remapping: Optional[Dict[str, torch.Tensor]] = None,
    ) -> None:
        super().__init__()
        self._embedding_bag_configs = tables
        self._is_weighted = is_weighted
        self._output_dtype = output_dtype
        self._feature_names = [f for t in tables for f in t.feature_names]
        self._lengths_per_embedding = [t.embedding_dim for t in tables for _ in t.feature_names]
        poolings = {t.pooling for t in tables}
        assert len(poolings) <= 1, "uniform pooling per quant EBC group"
        specs, remaps = _tbe_pruning_args(tables, index_remapping, "this quant EBC")
        self._tbe = QuantTableBatchedEmbeddingBags(
            specs,
            feature_table_map=[i for i, t in enumerate(tables) for _ in t.feature_names],
            pooling=next(iter(poolings)) if poolings else PoolingType.SUM,
            device=device,
            weight_dtypes=[quant_data_type(t.data_type) for t in tables],
            output_dtype=output_dtype,
            bounds_check=bounds_check,
            index_remapping=remaps,
        )

    @classmethod
    def from_float(
        cls,
        module: FloatEBC,
        output_dtype: torch.dtype = torch.float32,
        weight_dtype: DataType = DataType.INT8,
        per_table_weight_dtype: Optional[Dict[str, DataType]] = None,
        bounds_check: bool = False,
        index_remapping: Optional[Dict[str, torch.Tensor]] = None,
    ):
        """``index_remapping`` may name tables of other modules (they are
        ignored here). A named table's float rows are its logical rows, gathered
        through the remap, or already its physical rows: the row count decides
        (``_float_rows_for_remap``)."""
        tables = module.embedding_bag_configs()
        device = next(module.parameters()).device if any(True for _ in module.parameters()) else torch.device("cpu")
        own = {t.name for t in tables}
        index_remapping = {n: r for n, r in (index_remapping or {}).items() if n in own}
        qtables = [
            EmbeddingBagConfig(
                num_embeddings=t.num_embeddings,
                embedding_dim=t.embedding_dim,
                name=t.name,
                feature_names=list(t.feature_names),
                pooling=t.pooling,
                data_type=_resolve_weight_dtype(t.name, weight_dtype, per_table_weight_dtype),
                num_embeddings_post_pruning=t.num_embeddings_post_pruning,
            )
            for t in tables
        ]
        weights = []
        for t in tables:
            w = module.embedding_bags[t.name].weight.detach()
            if t.name in index_remapping:
                w = _float_rows_for_remap(t.name, w, index_remapping[t.name])
            weights.append(w)
        q = cls(
            tables=_quant_configs_for_remap(qtables, index_remapping),
            is_weighted=module.is_weighted(),
            device=device,
            output_dtype=output_dtype,
            bounds_check=bounds_check,
            index_remapping=index_remapping or None,
        )
        for i, w in enumerate(weights):
            q._tbe.load_float_table(i, w)
        return q

    def embedding_bag_configs(self) -> List[EmbeddingBagConfig]:
        return self._embedding_bag_configs

    def is_weighted(self) -> bool:
        return self._is_weighted

    def output_dtype(self) -> torch.dtype:
        return self._output_dtype

    def update_embeddings(self, delta: Dict[str, object]) -> Dict[str, torch.Tensor]:
        """Requantise the rows of ``delta`` (table name -> the model tracker's
        ``UniqueRows`` or ``(ids, rows)``) in place; ids outside ``[0, rows)``
        are dropped. Returns table name -> applied count. The contract is
        ``QuantTableBatchedEmbeddingBags.update_rows``'s."""
        check_delta_tables(delta, [t.name for t in self._embedding_bag_configs], "this quant EBC")
        return update_tbe_from_delta(self._tbe, delta)

    def forward(self, features: KeyedJaggedTensor) -> KeyedTensor:
        if features.keys() != self._feature_names:
            order = [features.keys().index(f) for f in self._feature_names]
            features = features.permute(order)
        values = self._tbe(
            features.values(),
            features.offsets(),
            features.weights_or_none() if self._is_weighted else None,
        )
        return KeyedTensor(
            keys=self._feature_names,
            values=values,
            length_per_key=self._lengths_per_embedding,
        )


class EmbeddingCollection(nn.Module):
    """Quantized sequence EC (reference quant/embedding_modules.py:748). Each
    table is served at its config's ``data_type`` when that is
    INT8/INT4/INT2/FP8, else INT8."""

    def __init__(
        self,
        tables: List[EmbeddingConfig],
        device: Optional[torch.device] = None,
        output_dtype: torch.dtype = torch.float32,
        bounds_check: bool = False,
        index_remapping: Optional[Dict[str, torch.Tensor]] = None,
    ) -> None:
        super().__init__()
        self._embedding_configs = tables
        self._output_dtype = output_dtype
        self._feature_names = [f for t in tables for f in t.feature_names]
        dims = {t.embedding_dim for t in tables}
        assert len(dims) <= 1
        self._dim = next(iter(dims)) if dims else 0
        specs, remaps = _tbe_pruning_args(tables, index_remapping, "this quant EC")
        self._tbe = QuantTableBatchedEmbeddingBags(
            specs,
            feature_table_map=[i for i, t in enumerate(tables) for _ in t.feature_names],
            device=device,
            weight_dtypes=[quant_data_type(t.data_type) for t in tables],
            output_dtype=output_dtype,
            bounds_check=bounds_check,
            index_remapping=remaps,
        )

    @classmethod
    def from_float(
        cls,
        module: FloatEC,
        output_dtype: torch.dtype = torch.float32,
        weight_dtype: DataType = DataType.INT8,
        per_table_weight_dtype: Optional[Dict[str, DataType]] = None,
        bounds_check: bool = False,
        index_remapping: Optional[Dict[str, torch.Tensor]] = None,
    ):
        """``bounds_check`` / ``index_remapping``: as the quant EBC's ``from_float``."""
        tables = [
            dataclasses.replace(
                t,
                feature_names=list(t.feature_names),
                data_type=_resolve_weight_dtype(t.name, weight_dtype, per_table_weight_dtype),
            )
            for t in module.embedding_configs()
        ]
        own = {t.name for t in tables}
        index_remapping = {n: r for n, r in (index_remapping or {}).items() if n in own}
        weights = []
        for t in tables:
            w = module.embeddings[t.name].weight.detach()
            if t.name in index_remapping:
                w = _float_rows_for_remap(t.name, w, index_remapping[t.name])
            weights.append(w)
        q = cls(
            tables=_quant_configs_for_remap(tables, index_remapping),
            output_dtype=output_dtype,
            bounds_check=bounds_check,
            index_remapping=index_remapping or None,
        )
        for i, w in enumerate(weights):
            q._tbe.load_float_table(i, w)
        return q

    def embedding_configs(self) -> List[EmbeddingConfig]:
        return self._embedding_configs

    def output_dtype(self) -> torch.dtype:
        return self._output_dtype

    def update_embeddings(self, delta: Dict[str, object]) -> Dict[str, torch.Tensor]:
        """Requantise the rows of ``delta`` (table name -> the model tracker's
        ``UniqueRows`` or ``(ids, rows)``) in place; ids outside ``[0, rows)``
        are dropped. Returns table name -> applied count. The contract is
        ``QuantTableBatchedEmbeddingBags.update_rows``'s."""
        check_delta_tables(delta, [t.name for t in self._embedding_configs], "this quant EC")
        return update_tbe_from_delta(self._tbe, delta)

    @torch.no_grad()
    def forward(self, features: KeyedJaggedTensor) -> Dict[str, JaggedTensor]:
        if features.keys() != self._feature_names:
            order = [features.keys().index(f) for f in self._feature_names]
            features = features.permute(order)
        tbe = self._tbe
        F = tbe._num_features
        B = features.stride()
        offsets = features.offsets()
        if tbe.qweights.is_cuda or (
            tbe.qweights.is_pinned() and features.values().is_cuda
        ):
            feat_val_offsets = offsets[:: B][: F + 1].contiguous()
            rows = tbe.forward_sequence(features.values(), feat_val_offsets, self._dim)
        else:
            rows_l = []
            for f, t in enumerate(tbe._feature_table_map):
                w = tbe._cpu_lookup_table(t)
                idx = features.values()[int(offsets[f * B]) : int(offsets[(f + 1) * B])]
                if tbe._checked:
                    idx = tbe._map_ids_cpu(t, idx)  # -1 indexes the appended zero row
                rows_l.append(w[idx])
            rows = torch.cat(rows_l, dim=0) if rows_l else torch.empty(0, self._dim)
            rows = tbe.to_output_dtype(rows)
        out: Dict[str, JaggedTensor] = {}
        opk = features.offset_per_key()
        lengths = features.lengths()
        for i, f in enumerate(self._feature_names):
            out[f] = JaggedTensor(
                values=rows[opk[i] : opk[i + 1]],
                lengths=lengths[i * B : (i + 1) * B],
            )
        return out
