"""activation_format="mxfp8": the layers of a QuantMLP hand each other the
MXFP8 pair. The emitted codes are those the next layer's own quantizer makes
of the fp32 result, so every module returns exactly what it returns without
the keyword."""

import pytest
import torch

from tests.test_quant_dense import _batch, _dlrm
from torchrec_amd import ops
from torchrec_amd.inference.modules import quantize_inference_model
from torchrec_amd.modules.mlp import MLP
from torchrec_amd.quant.mlp import QuantMLP

DEVICES = ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)]


@pytest.mark.parametrize("middle", [torch.relu, torch.sigmoid])
@pytest.mark.parametrize("device", DEVICES)
def test_quant_mlp_handoff_equals_default(device, middle):
    torch.manual_seed(0)
    mlp = MLP(13, [40, 33, 5]).to(device)
    mlp._mlp[1]._activation_fn = middle
    plain, handoff = QuantMLP.from_float(mlp), QuantMLP.from_float(mlp, activation_format="mxfp8")
    # a layer hands the pair on only where its activation rides the kernel, never the last
    assert [p._output_format for p in handoff._mlp] == [
        "mxfp8", "mxfp8" if middle is torch.relu else None, None]
    with torch.inference_mode():
        first = handoff._mlp[0](torch.randn(19, 13, device=device))
        assert isinstance(first, ops.MxActivation) and first.codes.shape == (19, 128)
        for shape in [(19, 13), (2, 19, 13)]:
            x = torch.randn(*shape, device=device)
            y = handoff(x)
            assert y.shape == (*shape[:-1], 5) and torch.equal(y, plain(x))


@pytest.mark.parametrize("device", DEVICES)
def test_quantize_inference_model_dense_activation_format(device):
    with pytest.raises(ValueError):
        quantize_inference_model(_dlrm(), dense_format="mxfp8", dense_activation_format="mxfp4")
    plain = quantize_inference_model(_dlrm().to(device), dense_format="mxfp8")
    handoff = quantize_inference_model(_dlrm().to(device), dense_format="mxfp8",
                                       dense_activation_format="mxfp8")
    assert handoff.dense_arch.model._mlp[0]._output_format == "mxfp8"
    dense, kjt = _batch()
    with torch.inference_mode():
        assert torch.equal(handoff(dense.to(device), kjt.to(device)),
                           plain(dense.to(device), kjt.to(device)))
