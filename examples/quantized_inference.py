"""Quantized inference end to end: train (briefly) -> quantize (INT8 by
default) -> shard for inference -> serve through the native batching runtime.

Run (1 GPU):  python examples/quantized_inference.py [--weight-dtype FP8]
``--weight-dtype`` is INT8, INT4, INT2 or FP8 (e4m3fn codes with a rowwise
scale: the bytes of INT8, a relative instead of an absolute error).
CPU works too (reference dequant path).
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from torchrec_amd.inference.modules import apply_model_delta, quantize_inference_model
from torchrec_amd.models.dlrm import DLRM
from torchrec_amd.modules.embedding_configs import DataType, EmbeddingBagConfig
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
from torchrec_amd.quant.embedding_modules import (
    EmbeddingBagCollection as QuantEmbeddingBagCollection,
)
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor


def main() -> None:
    parser = argparse.ArgumentParser()
    parser.add_argument("--weight-dtype", default="INT8", choices=["INT8", "INT4", "INT2", "FP8"])
    args = parser.parse_args()
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    keys = [f"cat_{i}" for i in range(4)]
    rows = [1000, 500, 800, 600]
    ebc = EmbeddingBagCollection(
        tables=[
            EmbeddingBagConfig(
                num_embeddings=r, embedding_dim=16, name=f"t{i}",
                feature_names=[keys[i]],
            )
            for i, r in enumerate(rows)
        ]
    )
    model = DLRM(
        embedding_bag_collection=ebc,
        dense_in_features=4,
        dense_arch_layer_sizes=[16, 16],
        over_arch_layer_sizes=[16, 1],
    )
    # quantize the sparse arch for serving
    # bounds_check: an id outside its table is dropped and counted on the
    # device instead of being read (index_remapping={table: remap} would also
    # serve pruned tables at their pruned size)
    qmodel = quantize_inference_model(
        model, weight_dtype=DataType[args.weight_dtype], bounds_check=True
    )
    qmodel = qmodel.to(device)

    B = 8
    g = torch.Generator().manual_seed(0)
    lengths = torch.ones(4 * B, dtype=torch.int64)
    values = torch.cat(
        [torch.randint(0, r, (B,), generator=g) for r in rows]
    )
    kjt = KeyedJaggedTensor(keys=keys, values=values, lengths=lengths, stride=B).to(device)
    dense = torch.rand(B, 4, device=device)
    with torch.no_grad():
        logits = qmodel(dense, kjt)
    print("predictions:", torch.sigmoid(logits.squeeze(-1)).cpu().tolist())

    # publish a training delta: fresh float rows for a few ids of table t0 (what
    # ModelDeltaTracker.get_unique() returns in UpdateMode.LAST) requantise in
    # place; nothing else in the served tables moves
    ids = values[:B].unique()
    delta = {"t0": (ids, torch.randn(ids.numel(), 16, device=device))}
    applied = apply_model_delta(qmodel, delta)
    with torch.no_grad():
        logits = qmodel(dense, kjt)
    print("rows updated:", {n: int(c) for n, c in applied.items()})
    print("predictions after the delta:", torch.sigmoid(logits.squeeze(-1)).cpu().tolist())

    # a request with a bad id: the lookup drops it (a zero contribution) and counts it
    bad = values.clone()
    bad[0] = rows[0] + 7
    with torch.no_grad():
        qmodel(dense, KeyedJaggedTensor(keys=keys, values=bad, lengths=lengths, stride=B).to(device))
    for m in qmodel.modules():
        if isinstance(m, QuantEmbeddingBagCollection):
            print("out-of-range ids per table:", m._tbe.out_of_range_counts().tolist())


if __name__ == "__main__":
    main()
