"""ops.mx_linear / mx_linear_pack_weight (mx_linear.hip) against float64.

Oracle: xq = decode(encode(x)), wq = decode(encode(W)) with the plain-PyTorch
MXFP8 codec on rows zero-padded to whole groups, ref = act(xq wq^T + b) in
float64. Codes and scales are exact, so only the fp32 accumulation separates
the kernel from ref: with u = 2^-24, h = 2^-8,
    acc   = 2 (K + 1) u (|xq| |wq|^T + |b|)        fp32 output
    bound = acc + h (|ref| + acc)                  bf16 output
One wrong code, scale byte or lane mapping is orders of magnitude outside:
32 consecutive k per lane, the CK headers' reading of the MFMA's layout, is
6000x to 100000x the bound wherever the four scales of a row differ.

The CPU path (an fp32 matmul) is held to acc as it stands. For the kernel acc
is widened by WIDEN = 64. The scaled MFMA does not sum its 128 products
as an fp32 chain: against this oracle the kernel's error is up to about
1300 u (|xq| |wq|^T), whatever K is, already for a single MFMA on 13
products, presumably because the products are aligned to the largest of them
in a fixed window and cut below it. Measured worst error / unwidened bound
over seeds 0-2 on the MI355X (fp32 output, no activation): (1, 32, 16) 2.81,
(5, 13, 24) 16.11, (33, 160, 1) 1.36, (130, 479, 80) 0.74 (bf16 x: 0.74),
(64, 1024, 129) 0.16, (1030, 300, 2050) 2.10. The smallest power of two that
covers 16.11 with a factor-two margin is 64. Integer inputs whose products
need no alignment come out exact.

x is randn * 2^e with e drawn per 32-group from [-6, 6], W randn / sqrt(K)
with e in [-2, 2], one whole group of each zeroed, b randn / 8.
"""

import functools

import pytest
import torch

from torchrec_amd import ops
from torchrec_amd.distributed import qcomm_codecs as qc

H, U = 2.0 ** -8, 2.0 ** -24
WIDEN = 64
N_STAR = ops.MX_LINEAR_WIDEST_TILE + 1
# the last shape is the one the host routes to the 64 x 128 tile (17 x 17
# workgroups, three K steps); all others take the 16 x 32 tile
SHAPES = [(1, 32, 16), (5, 13, 24), (33, 160, 1), (130, 479, 80), (64, 1024, N_STAR),
          (1030, 300, 2050)]
DTYPES = [torch.float32, torch.bfloat16]


def _draw(gen, rows, K, scale, emax):
    G = -(-K // 32)
    v = torch.randn(rows, G, 32, generator=gen) * scale
    v = v * torch.exp2(torch.randint(-emax, emax + 1, (rows, G, 1), generator=gen).float())
    if rows * G > 1:  # the one-tile case's x is a single group: zeroing it would void the check
        v[rows // 2, G // 2] = 0.0
    return v.reshape(rows, G * 32)[:, :K].contiguous()


@functools.lru_cache(maxsize=None)
def _case(M, K, N, x_bf16=False, bias=True, seed=0):
    """CPU (x, W, b, s, acc): s = xq wq^T + b before the activation, acc unwidened."""
    def quant(t):  # float64 decode(encode(t)) of the rows, zero-padded to whole groups
        p = torch.zeros(t.shape[0], -(-K // 32) * 32)
        p[:, :K] = t.float()
        wire = qc.mx_encode_reference(p.reshape(-1), "mxfp8")
        return qc.mx_decode_reference(wire, p.numel(), "mxfp8").reshape(p.shape).double()

    gen = torch.Generator().manual_seed(seed * 1000003 + M * 7919 + K * 263 + N)
    x = _draw(gen, M, K, 1.0, 6)
    x = x.bfloat16() if x_bf16 else x
    W = _draw(gen, N, K, K ** -0.5, 2)
    b = torch.randn(N, generator=gen) / 8 if bias else None
    xq, wq = quant(x), quant(W)
    b64 = b.double() if bias else torch.zeros(N, dtype=torch.float64)
    s = xq @ wq.T + b64
    acc = 2 * (K + 1) * U * (xq.abs() @ wq.abs().T + b64.abs())
    return x, W, b, s, acc


def _check(case, device, relu, dtype):
    """Run ops.mx_linear on ``device`` and hold it to the bound: acc as derived
    for the CPU path's fp32 matmul, widened by WIDEN for the MFMA."""
    x, W, b, s, acc = case
    codes, scales = ops.mx_linear_pack_weight(W.to(device))
    bd = None if b is None else b.to(device)
    got = ops.mx_linear(x.to(device), codes, scales, bd, W.shape[1], relu=relu, output_dtype=dtype)
    assert got.dtype == dtype and got.shape == s.shape
    ref = s.clamp_min(0) if relu else s
    acc = acc * (WIDEN if device == "cuda" else 1)
    bound = acc if dtype == torch.float32 else acc + H * (ref.abs() + acc)
    ratio = ((got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"y{tuple(s.shape)} K={W.shape[1]}: worst error/bound = {ratio:.3f}")
    assert ratio <= 1.0, f"error is {ratio:.2f}x the bound"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("M,K,N", SHAPES)
def test_mx_linear_gpu(M, K, N, relu, dtype):
    _check(_case(M, K, N), "cuda", relu, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("bias", [True, False])
def test_mx_linear_gpu_bf16_input(bias, dtype):
    _check(_case(130, 479, 80, x_bf16=True, bias=bias), "cuda", True, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K,N", [(5, 13, 24), (130, 479, 80)])
def test_mx_linear_cpu(M, K, N, dtype):
    _check(_case(M, K, N), "cpu", True, dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("N,K", [(24, 13), (80, 479), (17, 1024)])
def test_pack_weight_matches_reference(N, K):
    W = _draw(torch.Generator().manual_seed(N + K), N, K, K ** -0.5, 2)
    G, Kp = -(-K // 32), -(-K // 128) * 128
    p = torch.zeros(N, G * 32)
    p[:, :K] = W
    wire = qc.mx_encode_reference(p.reshape(-1), "mxfp8").view(torch.uint8).reshape(N, G, 33)
    codes, scales = (t.cpu() for t in ops.mx_linear_pack_weight(W.cuda()))
    assert codes.shape == (N, Kp) and scales.shape == (N, Kp // 32)
    assert torch.equal(codes[:, : G * 32], wire[:, :, :32].reshape(N, G * 32))
    assert torch.equal(scales[:, :G], wire[:, :, 32])
    assert not codes[:, G * 32 :].any() and not scales[:, G:].any()


@pytest.mark.gpu
def test_graph_replay_equals_eager():
    x, W, b, _, _ = _case(130, 479, 80)
    codes, scales = ops.mx_linear_pack_weight(W.cuda())
    xd, bd = x.cuda(), b.cuda()
    eager = ops.mx_linear(xd, codes, scales, bd, 479, relu=True)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.mx_linear(xd, codes, scales, bd, 479, relu=True)
    for _ in range(3):
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)
