"""MXFP8 dense layers for serving: the quantized forms of ``modules.mlp``'s
Perceptron / MLP (the reference's ``quantize_dense`` only casts to fp16).

A layer holds its weight as MXFP8 codes and E8M0 scale bytes (groups of 32
consecutive input features per output row, ``ops.mx_linear_pack_weight``) and
runs ``ops.mx_linear``: the activations are quantized the same way inside the
GEMM kernel, products and sums are fp32, and bias and ReLU ride the kernel's
epilogue. With ``activation_format="mxfp8"`` the layers of a ``QuantMLP`` hand
each other the quantized activation itself (``ops.MxActivation``), so a layer
quantizes its result once in its epilogue and the next one reads codes.
``weight_format="mxfp4"`` stores the weight as e2m1 codes instead (two k per
byte, the same scale bytes): half the weight bytes, activations still MXFP8.
Inference only."""

from __future__ import annotations

from typing import Callable, Optional, Union

import torch
import torch.nn as nn

from torchrec_amd import ops
from torchrec_amd.modules.mlp import MLP, Perceptron

_OUTPUT_DTYPES = (torch.float32, torch.bfloat16)


class QuantPerceptron(nn.Module):
    """``activation(mx_linear(x))``. ReLU (``torch.relu`` / ``nn.ReLU``) and
    identity ride the kernel; any other activation is applied by torch to the
    kernel's un-activated output.

    ``activation_format="mxfp8"`` makes the layer return an
    ``ops.MxActivation`` (2-D input only) for a following ``QuantPerceptron``
    instead of an ``output_dtype`` tensor, where its activation rides the
    kernel; with any other activation it returns the tensor as before. Its
    input may be either form whatever the keyword says."""

    def __init__(
        self,
        in_size: int,
        codes: torch.Tensor,
        scales: torch.Tensor,
        bias: Optional[torch.Tensor],
        activation: Union[Callable[[torch.Tensor], torch.Tensor], nn.Module] = torch.relu,
        output_dtype: torch.dtype = torch.float32,
        activation_format: Optional[str] = None,
        weight_format: str = "mxfp8",
    ) -> None:
        super().__init__()
        assert weight_format in ("mxfp8", "mxfp4"), f"unknown weight_format {weight_format!r}"
        assert output_dtype in _OUTPUT_DTYPES, f"output_dtype must be fp32 or bf16, got {output_dtype}"
        assert activation_format in (None, "mxfp8"), f"unknown activation_format {activation_format!r}"
        self._in_size = in_size
        self._out_size = codes.shape[0]
        self._output_dtype = output_dtype
        self._weight_format = weight_format
        self._activation_fn = activation
        self._relu = activation is torch.relu or isinstance(activation, nn.ReLU)
        self._identity = activation is None or isinstance(activation, nn.Identity)
        self._output_format = activation_format if self._relu or self._identity else None
        self.register_buffer("codes", codes)
        self.register_buffer("scales", scales)
        self.register_buffer("bias", bias)

    @classmethod
    def from_float(
        cls,
        module: Perceptron,
        output_dtype: torch.dtype = torch.float32,
        activation_format: Optional[str] = None,
        weight_format: str = "mxfp8",
    ) -> "QuantPerceptron":
        linear = module._linear
        codes, scales = ops.mx_linear_pack_weight(linear.weight, weight_format)
        bias = None if linear.bias is None else linear.bias.detach().float().clone()
        return cls(module._in_size, codes, scales, bias, module._activation_fn, output_dtype,
                   activation_format, weight_format)

    def forward(
        self, input: Union[torch.Tensor, ops.MxActivation]
    ) -> Union[torch.Tensor, ops.MxActivation]:
        if (torch.is_grad_enabled() and not isinstance(input, ops.MxActivation)
                and input.requires_grad):
            raise RuntimeError("QuantPerceptron is inference-only: its input requires grad")
        y = ops.mx_linear(
            input, self.codes, self.scales, self.bias, self._in_size,
            relu=self._relu, output_dtype=self._output_dtype, output_format=self._output_format,
            weight_format=self._weight_format,
        )
        return y if self._relu or self._identity else self._activation_fn(y)


class QuantMLP(nn.Module):
    """Stack of QuantPerceptrons. Every layer, the intermediate ones too,
    emits ``output_dtype``, unless ``result_dtype`` names another dtype for
    the last layer (what ``quantize_dense`` uses to hand the stack's result
    to float neighbours in their own dtype while the layers between stay
    bf16).

    ``activation_format="mxfp8"``: every layer but the last whose activation
    rides the kernel hands its successor an ``ops.MxActivation`` instead; a
    layer with another activation emits ``output_dtype`` and its successor
    quantizes in-kernel as before. Input and result stay float tensors."""

    def __init__(self, layers: nn.Sequential, in_size: int, out_size: int) -> None:
        super().__init__()
        self._mlp = layers
        self._in_size = in_size
        self._out_size = out_size

    @classmethod
    def from_float(
        cls,
        module: MLP,
        output_dtype: torch.dtype = torch.float32,
        result_dtype: Optional[torch.dtype] = None,
        activation_format: Optional[str] = None,
        weight_format: str = "mxfp8",
    ) -> "QuantMLP":
        last = len(module._mlp) - 1
        layers = nn.Sequential(
            *[
                QuantPerceptron.from_float(
                    p,
                    output_dtype=(result_dtype or output_dtype) if i == last else output_dtype,
                    activation_format=None if i == last else activation_format,
                    weight_format=weight_format,
                )
                for i, p in enumerate(module._mlp)
            ]
        )
        return cls(layers, module._in_size, module._out_size)

    def forward(self, input: torch.Tensor) -> torch.Tensor:
        if torch.is_grad_enabled() and input.requires_grad:
            raise RuntimeError("QuantMLP is inference-only: its input requires grad")
        # the MXFP8 pair between two layers is 2-D
        y = self._mlp(input.reshape(-1, input.shape[-1]))
        return y.reshape(*input.shape[:-1], y.shape[-1])
