"""Quantized-communication codecs for pooled/sequence collectives.

Reference parity: torchrec/distributed/fbgemm_qcomm_codec.py (QCommsConfig
:55, precisions FP32/FP16/BF16/FP8/INT8 :31-50) and the QuantizedCommCodec
protocol (torchrec/distributed/types.py:233). The codec plugs into
comm_ops.alltoall_pooled / reduce-scatter via the ``codec`` argument.
"""

from __future__ import annotations

from dataclasses import dataclass
from enum import Enum, unique
from typing import Optional

import torch


@unique
class CommType(Enum):
    FP32 = "fp32"
    FP16 = "fp16"
    BF16 = "bf16"
    FP8 = "fp8"
    INT8 = "int8"
    MX4 = "mx4"
    MXFP8 = "mxfp8"  # OCP MX: 32 x e4m3fn + one E8M0 scale byte per group
    MXFP4 = "mxfp4"  # OCP MX: 32 x e2m1 (two per byte) + one E8M0 scale byte


# ---------------------------------------------------------------------------
# OCP microscaling wire (MXFP8 / MXFP4): plain-PyTorch reference.
#
# This is the numerics oracle of ops/csrc/qcomm_codec.hip and the path CPU
# (gloo) tensors take. Groups of 32 consecutive fp32 values share one
# power-of-two scale 2^E; the wire is interleaved per group, codes first and
# the scale byte (E + 127) last, so a split at any group boundary is
# self-contained: encode(cat(a, b)) == cat(encode(a), encode(b)).
# ---------------------------------------------------------------------------

MX_GROUP = 32
# fmt -> (elem_max, emax, mantissa bits of elem_max, code bytes per group)
_MX_FORMATS = {
    "mxfp8": (448.0, 8, 0x600000, 32),  # 448 = 1.75 * 2^8
    "mxfp4": (6.0, 2, 0x400000, 16),  # 6 = 1.5 * 2^2
}
_E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def mx_group_bytes(fmt: str) -> int:
    return _MX_FORMATS[fmt][3] + 1


def _pow2(e: torch.Tensor) -> torch.Tensor:
    """2^e in fp32 for integer e in [-127, 127], built from the bits (2^-127
    is the subnormal 0x00400000)."""
    e = e.to(torch.int32)
    bits = torch.where(e > -127, (e + 127) << 23, torch.full_like(e, 0x00400000))
    return bits.view(torch.float32)


def _e2m1_codes(a: torch.Tensor) -> torch.Tensor:
    """Magnitude code (0..7) of a in [0, 6], round to nearest even. The grid
    step is .5 below 2, 1 below 4 and 2 above, and torch.round sends halves
    to the even multiple, which on every binade is the even mantissa: the
    midpoints .25 .75 1.25 1.75 2.5 3.5 5 go to 0 1 1 2 2 4 4."""
    q = torch.where(
        a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2)
    )
    return torch.where(q < 2, q * 2, torch.where(q < 4, q + 2, q / 2 + 4)).to(torch.uint8)


def mx_encode_reference(t: torch.Tensor, fmt: str) -> torch.Tensor:
    """Flat fp32 message -> int8 wire of numel / 32 groups."""
    elem_max, emax, mant_max, _ = _MX_FORMATS[fmt]
    assert t.numel() % MX_GROUP == 0, "MX wire needs numel % 32 == 0"
    v = t.reshape(-1, MX_GROUP).float()
    bits = v.contiguous().view(torch.int32)
    # amax from the |x| bit patterns: NaN and Inf sort above every finite value
    amax_bits = (bits & 0x7FFFFFFF).amax(dim=1)
    exp = amax_bits >> 23  # a subnormal amax has exp 0, i.e. exponent -127
    nonfinite = exp == 255
    zero = amax_bits == 0
    # E0 = exp - 127 - emax puts amax * 2^-E0 in [2^emax, 2^(emax+1)); it is
    # above elem_max exactly when amax's mantissa is above elem_max's
    E = exp - 127 - emax + ((amax_bits & 0x7FFFFF) > mant_max).to(torch.int32)
    E = E.clamp(-127, 127)
    scaled = (v * _pow2(-E).unsqueeze(1)).clamp(-elem_max, elem_max)
    sign = ((bits >> 31) & 1).to(torch.uint8)
    if fmt == "mxfp8":
        mag = torch.nan_to_num(scaled).to(torch.float8_e4m3fn).view(torch.uint8) & 0x7F
        codes = mag | (sign << 7)
    else:
        nib = _e2m1_codes(torch.nan_to_num(scaled).abs()) | (sign << 3)
        codes = nib[:, 0::2] | (nib[:, 1::2] << 4)
    codes = torch.where((nonfinite | zero).unsqueeze(1), torch.zeros_like(codes), codes)
    scale = torch.where(nonfinite, 255, torch.where(zero, 0, E + 127)).to(torch.uint8)
    return torch.cat([codes, scale.unsqueeze(1)], dim=1).reshape(-1).view(torch.int8)


def mx_decode_reference(wire: torch.Tensor, numel: int, fmt: str) -> torch.Tensor:
    """int8 wire -> flat fp32 message; code * 2^E is exact in fp32."""
    code_bytes = _MX_FORMATS[fmt][3]
    b = wire.view(torch.uint8).reshape(numel // MX_GROUP, code_bytes + 1)
    codes, scale = b[:, :code_bytes], b[:, code_bytes].to(torch.int32)
    if fmt == "mxfp8":
        vals = codes.contiguous().view(torch.float8_e4m3fn).to(torch.float32)
    else:
        nib = torch.stack([codes & 0xF, codes >> 4], dim=-1).reshape(-1, MX_GROUP)
        lut = torch.tensor(_E2M1_VALUES, dtype=torch.float32, device=wire.device)
        vals = lut[(nib & 7).long()] * (1.0 - 2.0 * (nib >> 3).to(torch.float32))
    out = vals * _pow2(scale.clamp(max=254) - 127).unsqueeze(1)
    nan = torch.full_like(out, float("nan"))
    return torch.where((scale == 255).unsqueeze(1), nan, out).reshape(-1)


def _gather_pooled_blocks(mat: torch.Tensor, dim_sum_per_rank) -> torch.Tensor:
    """[B, sum_D] -> flat message: each rank's column block, flattened."""
    parts, off = [], 0
    for d in dim_sum_per_rank:
        parts.append(mat[:, off : off + d].reshape(-1))
        off += d
    return torch.cat(parts)


def _paste_pooled_blocks(flat: torch.Tensor, B: int, dim_sum_per_rank) -> torch.Tensor:
    """Flat message -> [B, sum_D]: rank r's B * d_r values are its block."""
    blocks, off = [], 0
    for d in dim_sum_per_rank:
        blocks.append(flat[off : off + B * d].view(B, d))
        off += B * d
    return torch.cat(blocks, dim=1)


class QuantizedCommCodec:
    """encode/decode a flat fp32 tensor for the wire (reference types.py:233)."""

    def __init__(self, comm_precision: CommType) -> None:
        self._precision = comm_precision
        self._wire_dtype = {
            CommType.FP32: torch.float32,
            CommType.FP16: torch.float16,
            CommType.BF16: torch.bfloat16,
            CommType.FP8: torch.float8_e4m3fn,  # OCP e4m3 (gfx950-native)
            CommType.INT8: torch.int8,
            CommType.MX4: torch.int8,
            CommType.MXFP8: torch.int8,
            CommType.MXFP4: torch.int8,
        }[comm_precision]
        self._mx = comm_precision in (CommType.MXFP8, CommType.MXFP4)

    @property
    def precision(self) -> CommType:
        return self._precision

    @property
    def group_size(self) -> int:
        """Pooled a2a block widths must be a multiple of this (1: no limit)."""
        return MX_GROUP if self._mx else 1

    MX4_GROUP = 32  # values per shared exponent (OCP MX spec)

    def encoded_numel(self, numel: int) -> int:
        if self._precision == CommType.INT8:
            return numel + 4  # + packed fp32 scale
        if self._precision == CommType.MX4:
            assert numel % self.MX4_GROUP == 0, (
                "MX4 wire needs numel % 32 == 0 (use dims that are multiples "
                "of 32 so a2a block splits stay group-aligned)"
            )
            # 32 nibbles -> 16 bytes + 1 shared-exponent byte per group
            return (numel // self.MX4_GROUP) * (self.MX4_GROUP // 2 + 1)
        if self._mx:
            assert numel % MX_GROUP == 0, (
                f"{self._precision.value} wire needs numel % 32 == 0 (use dims that are "
                "multiples of 32 so a2a block splits stay group-aligned)"
            )
            return (numel // MX_GROUP) * mx_group_bytes(self._precision.value)
        return numel

    def encode(self, t: torch.Tensor) -> torch.Tensor:
        if self._precision == CommType.FP32:
            return t
        if self._precision == CommType.INT8:
            # symmetric per-message scale packed into 4 trailing int8 bytes
            scale = (t.abs().max().clamp(min=1e-8) / 127.0).reshape(1)
            q = (t / scale).round().clamp(-127, 127).to(torch.int8)
            return torch.cat([q, scale.view(torch.int8)])
        if self._precision == CommType.FP8:
            # OCP e4m3 payload on an int8 wire (RCCL dtype support)
            return t.to(self._wire_dtype).view(torch.int8)
        if self._precision == CommType.MX4:
            return self._encode_mx4(t)
        if self._mx:
            from torchrec_amd import ops

            return ops.qcomm_mx_encode(t, self._precision.value)
        return t.to(self._wire_dtype)

    def _encode_mx4(self, t: torch.Tensor) -> torch.Tensor:
        """OCP MX4-style: groups of 32 share a power-of-two exponent byte;
        each value is a signed 4-bit scaled integer (1 sign + 3 magnitude)."""
        G = self.MX4_GROUP
        v = t.reshape(-1, G).float()
        amax = v.abs().amax(dim=1).clamp(min=1e-30)
        # shared exponent: scale so the max maps to 7
        exp = torch.ceil(torch.log2(amax / 7.0))
        exp = exp.clamp(-127, 127)
        scale = torch.pow(2.0, exp).unsqueeze(1)
        q = (v / scale).round().clamp(-7, 7).to(torch.int8)  # [-7, 7]
        # pack two nibbles per byte (offset-8 so the nibble is unsigned)
        u = (q + 8).to(torch.uint8).reshape(-1, G // 2, 2)
        packed = (u[..., 0] | (u[..., 1] << 4)).reshape(-1, G // 2)
        exp_b = (exp.to(torch.int8) .view(-1, 1)).view(torch.uint8)
        return torch.cat([packed, exp_b], dim=1).reshape(-1).view(torch.int8)

    def decode(self, t: torch.Tensor, numel: int) -> torch.Tensor:
        if self._precision == CommType.FP32:
            return t
        if self._precision == CommType.INT8:
            scale = t[-4:].view(torch.float32)
            return t[:-4].to(torch.float32) * scale
        if self._precision == CommType.FP8:
            return t.view(torch.float8_e4m3fn).to(torch.float32)
        if self._precision == CommType.MX4:
            return self._decode_mx4(t, numel)
        if self._mx:
            from torchrec_amd import ops

            return ops.qcomm_mx_decode(t, numel, self._precision.value)
        return t.to(torch.float32)

    # -- pooled a2a: the message is the concatenation over ranks r of the
    # [B, d_r] column block of one [B, sum_D] matrix -------------------------

    def encode_pooled_blocks(self, mat: torch.Tensor, dim_sum_per_rank) -> torch.Tensor:
        """[B, sum_D] -> wire of the rank-block-major message. MXFP8 / MXFP4
        gather the blocks inside the encode kernel; the others slice,
        flatten and concatenate, then encode."""
        if self._mx:
            from torchrec_amd import ops

            return ops.qcomm_mx_encode(mat, self._precision.value, block_dims=dim_sum_per_rank)
        return self.encode(_gather_pooled_blocks(mat, dim_sum_per_rank))

    def decode_pooled_blocks(self, wire: torch.Tensor, B: int, dim_sum_per_rank) -> torch.Tensor:
        """Inverse of encode_pooled_blocks: wire -> [B, sum_D]."""
        numel = B * sum(dim_sum_per_rank)
        if self._mx:
            from torchrec_amd import ops

            return ops.qcomm_mx_decode(
                wire, numel, self._precision.value, block_dims=dim_sum_per_rank, B=B
            )
        return _paste_pooled_blocks(self.decode(wire, numel), B, dim_sum_per_rank)

    def _decode_mx4(self, t: torch.Tensor, numel: int) -> torch.Tensor:
        G = self.MX4_GROUP
        rows = numel // G
        b = t.view(torch.uint8).reshape(rows, G // 2 + 1)
        packed = b[:, : G // 2]
        exp = b[:, G // 2].view(torch.int8).to(torch.float32)
        lo = (packed & 0xF).to(torch.int16) - 8
        hi = (packed >> 4).to(torch.int16) - 8
        q = torch.stack([lo, hi], dim=-1).reshape(rows, G).to(torch.float32)
        return (q * torch.pow(2.0, exp).unsqueeze(1)).reshape(-1)


@dataclass
class QCommsConfig:
    """Reference parity: fbgemm_qcomm_codec.py:55."""

    forward_precision: CommType = CommType.FP32
    backward_precision: CommType = CommType.FP32


def get_qcomm_codecs(config: Optional[QCommsConfig]):
    if config is None:
        return None, None
    fwd = (
        QuantizedCommCodec(config.forward_precision)
        if config.forward_precision != CommType.FP32
        else None
    )
    bwd = (
        QuantizedCommCodec(config.backward_precision)
        if config.backward_precision != CommType.FP32
        else None
    )
    return fwd, bwd
