"""MXFP8 dense modules (quant/mlp.py) and the quantize_dense build step."""

import pytest
import torch

from torchrec_amd import ops
from torchrec_amd.inference.modules import quantize_dense, quantize_inference_model
from torchrec_amd.models.dlrm import DLRM
from torchrec_amd.modules.embedding_configs import EmbeddingBagConfig
from torchrec_amd.modules.embedding_modules import EmbeddingBagCollection
from torchrec_amd.modules.mlp import MLP, Perceptron
from torchrec_amd.quant.embedding_modules import EmbeddingBagCollection as QuantEBC
from torchrec_amd.quant.mlp import QuantMLP, QuantPerceptron
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

KEYS, ROWS, B = ["a", "b"], [50, 30], 6


def _dlrm():
    torch.manual_seed(0)
    ebc = EmbeddingBagCollection(tables=[
        EmbeddingBagConfig(num_embeddings=r, embedding_dim=16, name=f"t{i}", feature_names=[k])
        for i, (k, r) in enumerate(zip(KEYS, ROWS))
    ])
    return DLRM(ebc, dense_in_features=13, dense_arch_layer_sizes=[24, 16],
                over_arch_layer_sizes=[40, 20, 1])


def _batch():
    g = torch.Generator().manual_seed(1)
    values = torch.cat([torch.randint(0, r, (B,), generator=g) for r in ROWS])
    kjt = KeyedJaggedTensor(keys=KEYS, values=values,
                            lengths=torch.ones(2 * B, dtype=torch.int64), stride=B)
    return torch.randn(B, 13, generator=g), kjt


def _kinds(model, *types):
    return [n for n, m in model.named_modules() if isinstance(m, types)]


def _chain(q, x, relu, dtype):
    for p in q._mlp:
        x = ops.mx_linear(x, p.codes, p.scales, p.bias, p._in_size, relu=relu, output_dtype=dtype)
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_quant_mlp_is_the_op_chain(dtype):
    torch.manual_seed(0)
    x = torch.randn(33, 479, device="cuda")
    relu_q = QuantMLP.from_float(MLP(479, [96, 40, 1]).cuda(), output_dtype=dtype)
    sig_q = QuantMLP.from_float(MLP(479, [96, 40, 1], bias=False, activation="sigmoid").cuda(),
                                output_dtype=dtype)
    assert sig_q._mlp[0].bias is None
    with torch.inference_mode():
        y = relu_q(x)
        assert y.dtype == dtype and torch.equal(y, _chain(relu_q, x, True, dtype))
        h = x
        for p in sig_q._mlp:
            h = torch.sigmoid(
                ops.mx_linear(h, p.codes, p.scales, p.bias, p._in_size, output_dtype=dtype))
        assert torch.equal(sig_q(x), h)


def test_quantize_dense_swaps_mlps_only():
    model = _dlrm()
    with pytest.raises(ValueError):
        quantize_dense(model, weight_format="fp16")
    assert not _kinds(model, QuantMLP, QuantPerceptron)
    assert quantize_dense(model, skip={"over_arch.model.0"}) is model
    assert isinstance(model.dense_arch.model, QuantMLP)
    assert isinstance(model.over_arch.model[0], MLP)
    quantize_dense(model)
    assert not _kinds(model, MLP, Perceptron) and len(_kinds(model, QuantPerceptron)) == 4
    assert isinstance(model.sparse_arch.embedding_bag_collection, EmbeddingBagCollection)
    # a lone Perceptron is swapped too
    holder = torch.nn.Sequential(Perceptron(13, 8))
    assert isinstance(quantize_dense(holder)[0], QuantPerceptron)


def test_quantize_inference_model_dense_format():
    plain = quantize_inference_model(_dlrm())
    assert _kinds(plain, QuantEBC) and not _kinds(plain, QuantMLP, QuantPerceptron)
    assert len(_kinds(plain, MLP)) == 2
    both = quantize_inference_model(_dlrm(), dense_format="mxfp8")
    assert _kinds(both, QuantEBC) and len(_kinds(both, QuantMLP)) == 2 and not _kinds(both, MLP)
    dense, kjt = _batch()
    with torch.inference_mode():
        want = both.over_arch(both.inter_arch(
            _chain(both.dense_arch.model, dense, True, torch.float32), both.sparse_arch(kjt)))
        assert torch.equal(both(dense, kjt), want)


@pytest.mark.parametrize("via_inference_model", [False, True])
def test_bf16_dense_runs_on_dlrm(via_inference_model):
    """bf16 stays inside a swapped MLP; its result is fp32 for the float neighbours,
    and the embeddings' output_dtype is not the dense one."""
    dense, kjt = _batch()
    if via_inference_model:
        with pytest.raises(ValueError):
            quantize_inference_model(_dlrm(), dense_format="mxfp8", dense_output_dtype=torch.float16)
        model = quantize_inference_model(_dlrm(), output_dtype=torch.bfloat16, dense_format="mxfp8")
        assert {p._output_dtype for p in model.modules() if isinstance(p, QuantPerceptron)} == {
            torch.float32}
        model = quantize_inference_model(_dlrm(), output_dtype=torch.bfloat16,
                                         dense_format="mxfp8", dense_output_dtype=torch.bfloat16)
    else:
        model = quantize_dense(_dlrm(), output_dtype=torch.bfloat16)
    assert [p._output_dtype for p in model.over_arch.model[0]._mlp] == [torch.bfloat16,
                                                                       torch.float32]
    with torch.inference_mode():
        assert model.dense_arch(dense).dtype == torch.float32
        out = model(dense, kjt)
    assert out.dtype == torch.float32 and out.shape == (B, 1) and out.isfinite().all()


def test_state_dict_round_trip_and_inference_only():
    a = quantize_dense(_dlrm())
    torch.manual_seed(5)
    b = quantize_dense(DLRM(a.sparse_arch.embedding_bag_collection, 13, [24, 16], [40, 20, 1]))
    dense, kjt = _batch()
    with torch.inference_mode():
        assert not torch.equal(a(dense, kjt), b(dense, kjt))
        b.load_state_dict(a.state_dict())
        assert torch.equal(a(dense, kjt), b(dense, kjt))
    sd = a.dense_arch.state_dict()
    assert sd["model._mlp.0.codes"].shape == (24, 128) and sd["model._mlp.0.scales"].shape == (24, 4)
    with pytest.raises(RuntimeError):
        a.dense_arch(dense.requires_grad_(True))
