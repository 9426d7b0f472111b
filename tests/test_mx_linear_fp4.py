"""ops.mx_linear with MXFP4 weights (W4A8, mx_linear.hip) against float64.

Inputs, oracle and bound are tests/test_mx_linear.py's with wq =
decode4(encode4(W)), the plain-PyTorch MXFP4 codec; xq stays MXFP8. Measured
worst error / unwidened bound on the MI355X over seeds 0-2 (fp32 output, no
activation): (1, 32, 16) 0.01, (5, 13, 24) 15.95, (33, 160, 1) 0.32,
(130, 479, 80) 0.39 (bf16 x: 0.39), (64, 1024, 129) 0.09, (1030, 300, 2050)
1.22. The smallest power of two that covers 15.95 twice is 32, at most 64, so
WIDEN stays 64. A wrong nibble order or lane mapping is thousands of times out.
"""

import functools

import pytest
import torch

from tests.test_mx_linear import H, N_STAR, U, WIDEN, _case as _case8, _draw
from tests.test_quant_dense import _batch, _dlrm, _kinds
from torchrec_amd import ops
from torchrec_amd.distributed import qcomm_codecs as qc
from torchrec_amd.inference.modules import quantize_dense, quantize_inference_model
from torchrec_amd.modules.mlp import MLP, Perceptron
from torchrec_amd.quant.mlp import QuantMLP

SHAPES = [(1, 32, 16), (5, 13, 24), (33, 160, 1), (130, 479, 80), (64, 1024, N_STAR),
          (1030, 300, 2050)]
F4 = dict(weight_format="mxfp4")


def _quant(t, fmt, width=None):
    """(float64 decode(encode(t)), wire) of the rows zero-padded to whole groups or ``width``."""
    p = torch.zeros(t.shape[0], width or -(-t.shape[1] // 32) * 32)
    p[:, : t.shape[1]] = t.float()
    wire = qc.mx_encode_reference(p.reshape(-1), fmt)
    return qc.mx_decode_reference(wire, p.numel(), fmt).reshape(p.shape).double(), wire


@functools.lru_cache(maxsize=None)
def _case(M, K, N, x_bf16=False, bias=True, seed=0):
    """CPU (x, W, b, s, acc): s = xq wq^T + b before the activation, acc unwidened."""
    x, W, b, _, _ = _case8(M, K, N, x_bf16, bias, seed)
    xq, wq = _quant(x, "mxfp8")[0], _quant(W, "mxfp4")[0]
    b64 = b.double() if bias else torch.zeros(N, dtype=torch.float64)
    return x, W, b, xq @ wq.T + b64, 2 * (K + 1) * U * (xq.abs() @ wq.abs().T + b64.abs())


def _ratio(case, device, relu, dtype, W=None):
    """Error / bound per element of ops.mx_linear on ``device`` (W: a variant of the case's)."""
    x, W0, b, s, acc = case
    codes, scales = ops.mx_linear_pack_weight((W0 if W is None else W).to(device), **F4)
    got = ops.mx_linear(x.to(device), codes, scales, None if b is None else b.to(device),
                        W0.shape[1], relu=relu, output_dtype=dtype, **F4)
    assert got.dtype == dtype and got.shape == s.shape
    ref = s.clamp_min(0) if relu else s
    acc = acc * (WIDEN if device == "cuda" else 1)
    bound = acc if dtype == torch.float32 else acc + H * (ref.abs() + acc)
    ratio = (got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)
    print(f"y{tuple(s.shape)} K={W0.shape[1]}: worst error/bound = {ratio.max().item():.3f}")
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("case", [(*s, False, True) for s in SHAPES]
                         + [(130, 479, 80, True, True), (130, 479, 80, False, False)])
def test_fp4_gpu(case, relu, dtype):  # the last two: bf16 input, no bias
    assert _ratio(_case(*case), "cuda", relu, dtype).max().item() <= 1.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,K,N", [(5, 13, 24), (130, 479, 80)])
def test_fp4_cpu(M, K, N, dtype):
    assert _ratio(_case(M, K, N), "cpu", True, dtype).max().item() <= 1.0


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(24, 13), (80, 479), (17, 1024)])
def test_fp4_pack_weight_matches_reference(N, K):
    W = _draw(torch.Generator().manual_seed(N + K), N, K, K ** -0.5, 2)
    G, Kp = -(-K // 32), -(-K // 128) * 128
    wire = _quant(W, "mxfp4")[1].view(torch.uint8).reshape(N, G, 17)
    codes, scales = (t.cpu() for t in ops.mx_linear_pack_weight(W.cuda(), **F4))
    assert codes.shape == (N, Kp // 2) and scales.shape == (N, Kp // 32)
    assert torch.equal(codes[:, : G * 16], wire[:, :, :16].reshape(N, G * 16))
    assert torch.equal(scales[:, :G], wire[:, :, 16])
    assert not codes[:, G * 16 :].any() and not scales[:, G:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("M,K,Hd,N", [(5, 13, 24, 33), (130, 479, 80, 129)])
def test_fp4_handoff(M, K, Hd, N):
    gen = torch.Generator().manual_seed(M + K + Hd + N)
    x, b1 = _draw(gen, M, K, 1.0, 6).cuda(), (torch.randn(Hd, generator=gen) / 8).cuda()
    W1, W2 = _draw(gen, Hd, K, K ** -0.5, 2).cuda(), _draw(gen, N, Hd, Hd ** -0.5, 2).cuda()
    (c1, s1), (c2, s2) = (ops.mx_linear_pack_weight(w, **F4) for w in (W1, W2))
    Hp = -(-Hd // 128) * 128
    pair = ops.mx_linear(x, c1, s1, b1, K, relu=True, output_format="mxfp8", **F4)
    hq, wire = _quant(ops.mx_linear(x, c1, s1, b1, K, relu=True, **F4).cpu(), "mxfp8", Hp)
    wire = wire.view(torch.uint8).reshape(M, Hp // 32, 33)
    assert pair.features == Hd and torch.equal(pair.codes.cpu(), wire[:, :, :32].reshape(M, Hp))
    assert torch.equal(pair.scales.cpu(), wire[:, :, 32])
    got = ops.mx_linear(pair, c2, s2, None, Hd, **F4)
    assert torch.equal(got, ops.mx_linear(hq[:, :Hd].float().cuda(), c2, s2, None, Hd, **F4))


@pytest.mark.gpu
def test_fp4_inf_in_w_marks_the_output_column():
    case = _case(33, 160, 24)
    W = case[1].clone()
    W[7, 40] = float("inf")
    ratio = _ratio(case, "cuda", False, torch.float32, W=W)
    assert ratio[:, 7].isnan().all() and ratio[:, torch.arange(24) != 7].max().item() <= 1.0


@pytest.mark.gpu
def test_fp4_graph_replay_equals_eager():
    x, W, b, _, _ = (t.cuda() for t in _case(130, 479, 80))
    codes, scales = ops.mx_linear_pack_weight(W, **F4)
    eager = ops.mx_linear(x, codes, scales, b, 479, relu=True, **F4)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.mx_linear(x, codes, scales, b, 479, relu=True, **F4)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


def test_fp4_quantize_dense_and_inference_model():
    with pytest.raises(ValueError):
        quantize_dense(_dlrm(), weight_format="fp6")
    model = quantize_dense(_dlrm(), weight_format="mxfp4")
    assert not _kinds(model, MLP, Perceptron) and len(_kinds(model, QuantMLP)) == 2
    sd = model.dense_arch.state_dict()
    assert sd["model._mlp.0.codes"].shape == (24, 64) and sd["model._mlp.0.scales"].shape == (24, 4)
    dense, kjt = _batch()
    plain = quantize_inference_model(_dlrm(), dense_format="mxfp4")
    act = quantize_inference_model(_dlrm(), dense_format="mxfp4", dense_activation_format="mxfp8")
    with torch.inference_mode():
        out = plain(dense, kjt)
        assert torch.equal(out, act(dense, kjt))
        out8 = quantize_inference_model(_dlrm(), dense_format="mxfp8")(dense, kjt)
    assert out.isfinite().all() and not torch.equal(out, out8)
