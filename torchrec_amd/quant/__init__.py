"""Quantized (INT8/INT4/INT2/FP8) inference modules (reference: torchrec/quant/__init__.py)."""

from torchrec_amd.quant.embedding_modules import (  # noqa: F401
    EmbeddingBagCollection,
    EmbeddingCollection,
    QuantTableBatchedEmbeddingBags,
    dequantize_rowwise_fp8,
    dequantize_rowwise_nbit,
    fp8_row_stride,
    nbit_row_stride,
    quantize_rowwise_fp8,
    quantize_rowwise_nbit,
)
