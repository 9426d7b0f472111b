"""MXFP8 activations handed from one ops.mx_linear to the next (mx_linear.hip).

A chain K -> H -> N: the producer (x W1^T + b1, ReLU on or off) emits an
ops.MxActivation, the consumer (ReLU the other way round) reads it.
  1. The emitted pair equals, byte for byte, the reference codec applied to
     the fp32 result of the existing float path on the same device, rows
     zero-padded to Hp; all padding is zero.
  2. The consumer against float64 on the decoded pair hq: ref = act(hq wq^T +
     b2), bound 2 (H + 1) u (|hq| |wq|^T + |b2|), widened by
     tests/test_mx_linear.py's WIDEN on the GPU, plus its bf16 term.
  3. The consumer fed the pair equals the float-in path fed hq bit for bit.
Inputs are test_mx_linear.py's draw: per-group exponents, one zeroed group.
"""

import functools

import pytest
import torch

from tests.test_mx_linear import H as H16, U, WIDEN, _draw
from torchrec_amd import ops
from torchrec_amd.distributed import qcomm_codecs as qc

# (M, K, H, N): H below a group with three padding groups; ragged everything;
# one column in H's second group, two row tiles, N = 1; ragged H inside the
# first 128, N past the widest tile; eight K steps on the consumer; producer
# on the 64 x 128 tile
SHAPES = [(1, 32, 16, 16), (5, 13, 24, 33), (33, 160, 33, 1), (130, 479, 80, 129),
          (64, 300, 1024, 129), (1030, 300, 2050, 16)]


@functools.lru_cache(maxsize=None)
def _case(M, K, Hd, N):
    gen = torch.Generator().manual_seed(M * 7919 + K * 263 + Hd * 31 + N)
    x = _draw(gen, M, K, 1.0, 6)
    W1, W2 = _draw(gen, Hd, K, K ** -0.5, 2), _draw(gen, N, Hd, Hd ** -0.5, 2)
    return x, W1, torch.randn(Hd, generator=gen) / 8, W2, torch.randn(N, generator=gen) / 8


def _encode_rows(h, width):
    """Reference (codes, scales) of the rows of fp32 ``h`` zero-padded to ``width``."""
    p = torch.zeros(h.shape[0], width)
    p[:, : h.shape[1]] = h
    wire = qc.mx_encode_reference(p.reshape(-1), "mxfp8").view(torch.uint8)
    wire = wire.reshape(h.shape[0], width // 32, 33)
    return wire[:, :, :32].reshape(h.shape[0], width), wire[:, :, 32]


def _decode64(codes, scales, width):
    wire = torch.cat([codes.reshape(codes.shape[0], -1, 32), scales.unsqueeze(2)], dim=2)
    flat = qc.mx_decode_reference(wire.reshape(-1).view(torch.int8), codes.numel(), "mxfp8")
    return flat.reshape(codes.shape)[:, :width].double()


def _check(shape, relu, device):
    M, K, Hd, N = shape
    x, W1, b1, W2, b2 = (t.to(device) for t in _case(*shape))
    (c1, s1), (c2, s2) = ops.mx_linear_pack_weight(W1), ops.mx_linear_pack_weight(W2)
    Hp = -(-Hd // 128) * 128

    # 1. producer
    pair = ops.mx_linear(x, c1, s1, b1, K, relu=relu, output_format="mxfp8")
    h32 = ops.mx_linear(x, c1, s1, b1, K, relu=relu, output_dtype=torch.float32)
    codes, scales = pair.codes.cpu(), pair.scales.cpu()
    assert pair.features == Hd and codes.shape == (M, Hp) and scales.shape == (M, Hp // 32)
    want_codes, want_scales = _encode_rows(h32.cpu(), Hp)
    assert torch.equal(codes, want_codes) and torch.equal(scales, want_scales)
    assert not codes[:, Hd:].any() and not scales[:, -(-Hd // 32):].any()

    hq, wq = _decode64(codes, scales, Hd), _decode64(c2.cpu(), s2.cpu(), Hd)
    s = hq @ wq.T + b2.double().cpu()
    ref = s if relu else s.clamp_min(0)
    acc = 2 * (Hd + 1) * U * (hq.abs() @ wq.abs().T + b2.double().cpu().abs())
    acc = acc * (WIDEN if device == "cuda" else 1)
    for dtype in (torch.float32, torch.bfloat16):
        got = ops.mx_linear(pair, c2, s2, b2, Hd, relu=not relu, output_dtype=dtype)
        assert got.dtype == dtype and got.shape == (M, N)
        # 2. float64 oracle
        bound = acc if dtype == torch.float32 else acc + H16 * (ref.abs() + acc)
        ratio = ((got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()
        print(f"{shape} relu={relu} {dtype}: worst error/bound = {ratio:.3f}")
        assert ratio <= 1.0, f"error is {ratio:.2f}x the bound"
        # 3. the float-in path on the decoded activation
        same = ops.mx_linear(hq.float().to(device), c2, s2, b2, Hd, relu=not relu,
                             output_dtype=dtype)
        assert torch.equal(got, same)


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_handoff_gpu(shape, relu):
    _check(shape, relu, "cuda")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", SHAPES[:2])
def test_handoff_cpu(shape, relu):
    _check(shape, relu, "cpu")


@pytest.mark.gpu
def test_inf_in_x_marks_the_producer_row():
    M, K, Hd, _ = shape = SHAPES[2]
    x, W1, b1, _, _ = (t.cuda() for t in _case(*shape))
    x = x.clone()
    x[7, 40] = float("inf")
    c1, s1 = ops.mx_linear_pack_weight(W1)
    pair = ops.mx_linear(x, c1, s1, b1, K, relu=True, output_format="mxfp8")
    live = -(-Hd // 32)
    assert (pair.scales[7, :live] == 0xFF).all() and not pair.scales[7, live:].any()
    assert not pair.codes[7].any()
    want = _encode_rows(ops.mx_linear(x, c1, s1, b1, K, relu=True).cpu(), pair.codes.shape[1])
    assert torch.equal(pair.codes.cpu(), want[0]) and torch.equal(pair.scales.cpu(), want[1])


@pytest.mark.gpu
def test_handoff_graph_replay_equals_eager():
    M, K, Hd, N = shape = SHAPES[3]
    x, W1, b1, W2, b2 = (t.cuda() for t in _case(*shape))
    (c1, s1), (c2, s2) = ops.mx_linear_pack_weight(W1), ops.mx_linear_pack_weight(W2)

    def chain():
        pair = ops.mx_linear(x, c1, s1, b1, K, relu=True, output_format="mxfp8")
        return pair, ops.mx_linear(pair, c2, s2, b2, Hd)

    eager_pair, eager = chain()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pair, out = chain()
    for _ in range(3):
        for t in (pair.codes, pair.scales, out):
            t.fill_(1)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(pair.codes, eager_pair.codes)
        assert torch.equal(pair.scales, eager_pair.scales) and torch.equal(out, eager)
