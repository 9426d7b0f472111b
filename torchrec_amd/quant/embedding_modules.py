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
    lookup's result: the arithmetic is fp32 and the value is rounded once."""

    def __init__(
        self,
        specs: List[Tuple[str, int, int]],  # (name, rows, dim)
        feature_table_map: Optional[List[int]] = None,
        pooling: PoolingType = PoolingType.SUM,
        device: Optional[torch.device] = None,
        location: str = "device",  # "device" (HBM) | "managed" (pinned host, QUANT_UVM)
        weight_dtypes: Optional[List[DataType]] = None,
        output_dtype: torch.dtype = torch.float32,
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
        byte_offsets = [0]
        for (_, rows, dim), b in zip(specs, self._formats):
            byte_offsets.append(byte_offsets[-1] + rows * self._stride(dim, b))
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

    @staticmethod
    def _stride(dim: int, bits: int) -> int:
        # ``bits`` is a format code. INT8 keeps its own stride rule (no dim
        # check: CPU lookups of odd dims keep working as before)
        if bits == FP8_FORMAT_CODE:
            return fp8_row_stride(dim)
        return int8_row_stride(dim) if bits == 8 else nbit_row_stride(dim, bits)

    def load_float_table(self, i: int, weights: torch.Tensor) -> None:
        name, rows, dim = self._specs[i]
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
            w = self.dequantized_table(t)
            off = offsets[f * B : (f + 1) * B + 1] - offsets[f * B]
            idx = indices[int(offsets[f * B]) : int(offsets[(f + 1) * B])]
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
        INT8, else tbe_forward_seq_nbit. ``feat_val_offsets`` is [F+1]."""
        ops.hip_ops()
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


class EmbeddingBagCollection(nn.Module):
    """Quantized EBC (reference quant/embedding_modules.py:346). Each table is
    served at its config's ``data_type`` when that is INT8/INT4/INT2/FP8, else INT8."""

    def __init__(
        self,
        tables: List[EmbeddingBagConfig],
        is_weighted: bool = False,
        device: Optional[torch.device] = None,
        output_dtype: torch.dtype = torch.float32,
    ) -> None:
        super().__init__()
        self._embedding_bag_configs = tables
        self._is_weighted = is_weighted
        self._output_dtype = output_dtype
        self._feature_names = [f for t in tables for f in t.feature_names]
        self._lengths_per_embedding = [t.embedding_dim for t in tables for _ in t.feature_names]
        poolings = {t.pooling for t in tables}
        assert len(poolings) <= 1, "uniform pooling per quant EBC group"
        self._tbe = QuantTableBatchedEmbeddingBags(
            [(t.name, t.num_embeddings, t.embedding_dim) for t in tables],
            feature_table_map=[i for i, t in enumerate(tables) for _ in t.feature_names],
            pooling=next(iter(poolings)) if poolings else PoolingType.SUM,
            device=device,
            weight_dtypes=[quant_data_type(t.data_type) for t in tables],
            output_dtype=output_dtype,
        )

    @classmethod
    def from_float(
        cls,
        module: FloatEBC,
        output_dtype: torch.dtype = torch.float32,
        weight_dtype: DataType = DataType.INT8,
        per_table_weight_dtype: Optional[Dict[str, DataType]] = None,
    ):
        tables = module.embedding_bag_configs()
        device = next(module.parameters()).device if any(True for _ in module.parameters()) else torch.device("cpu")
        q = cls(
            tables=[
                EmbeddingBagConfig(
                    num_embeddings=t.num_embeddings,
                    embedding_dim=t.embedding_dim,
                    name=t.name,
                    feature_names=list(t.feature_names),
                    pooling=t.pooling,
                    data_type=_resolve_weight_dtype(
                        t.name, weight_dtype, per_table_weight_dtype
                    ),
                )
                for t in tables
            ],
            is_weighted=module.is_weighted(),
            device=device,
            output_dtype=output_dtype,
        )
        for i, t in enumerate(tables):
            q._tbe.load_float_table(i, module.embedding_bags[t.name].weight.detach())
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
    ) -> None:
        super().__init__()
        self._embedding_configs = tables
        self._output_dtype = output_dtype
        self._feature_names = [f for t in tables for f in t.feature_names]
        dims = {t.embedding_dim for t in tables}
        assert len(dims) <= 1
        self._dim = next(iter(dims)) if dims else 0
        self._tbe = QuantTableBatchedEmbeddingBags(
            [(t.name, t.num_embeddings, t.embedding_dim) for t in tables],
            feature_table_map=[i for i, t in enumerate(tables) for _ in t.feature_names],
            device=device,
            weight_dtypes=[quant_data_type(t.data_type) for t in tables],
            output_dtype=output_dtype,
        )

    @classmethod
    def from_float(
        cls,
        module: FloatEC,
        output_dtype: torch.dtype = torch.float32,
        weight_dtype: DataType = DataType.INT8,
        per_table_weight_dtype: Optional[Dict[str, DataType]] = None,
    ):
        tables = [
            dataclasses.replace(
                t,
                feature_names=list(t.feature_names),
                data_type=_resolve_weight_dtype(t.name, weight_dtype, per_table_weight_dtype),
            )
            for t in module.embedding_configs()
        ]
        q = cls(tables=tables, output_dtype=output_dtype)
        for i, t in enumerate(tables):
            q._tbe.load_float_table(i, module.embeddings[t.name].weight.detach())
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
                w = tbe.dequantized_table(t)
                idx = features.values()[int(offsets[f * B]) : int(offsets[(f + 1) * B])]
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
