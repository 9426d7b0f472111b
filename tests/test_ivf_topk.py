"""IVF-Flat retrieval (ivf_topk.hip, IVFFlatIndex) against a float64 oracle:
scores of the bf16-rounded inputs plus bias, every row outside the query's
probed lists masked to -inf, stable sort by (score desc, row asc), first k,
-inf entries as (-inf, -1).

The exact cases draw integers in [-8, 8] (tests/test_mips_topk.py: fp32 is
exact in any order, ties are dense), so the kernel must equal the oracle bit
for bit. They share one list layout, lengths 0, 1, 63, 64, 65, 200, 700, 0, 16
(N = 1109): empty lists in front and inside, one under / on / over the 64-row
step, past one unrolled triple of steps (192), several triples (uneven when
split in three). The 70 queries' probes, from three columns on: the 700-row
list by every query but the last (69: two full tiles and one of 5), the 65-row
list by exactly 33 (a second tile with one live query), the 1-row list by
query 40 alone, the 16-row list by nobody, -1 entries in many rows, and the
last query probes only the two empty lists.
"""

import pytest
import torch

from tests.test_lowrank_cross import _draw
from tests.test_mips_topk import _adversarial, _check_real, _ints, oracle
from torchrec_amd import ops
from torchrec_amd.modules import IVFFlatIndex

LENGTHS = [0, 1, 63, 64, 65, 200, 700, 0, 16]
OFFSETS = torch.tensor([0] + LENGTHS).cumsum(0)
B, N = 70, sum(LENGTHS)
# (D, k, nprobe, splits, l2 bias)
EXACT = [
    (8, 1, 1, 1, False), (8, 10, 3, 3, False), (8, 128, 8, 1, False), (8, 100, 3, 3, True),
    (96, 10, 3, 1, False), (96, 100, 8, 3, True), (96, 1, 8, 3, False), (96, 128, 1, 1, False),
    (256, 10, 1, 3, False), (256, 128, 3, 1, False), (256, 100, 8, 1, False),
    (256, 10, 8, 3, False),
]


def _probes(nprobe):
    mid = [5, 2, 3]  # the 200-, 63- and 64-row lists
    rows = []
    for b in range(B - 1):
        c1 = 4 if b < 33 else mid[b % 3]
        c2 = 1 if b == 40 else -1 if b % 5 == 0 else mid[(b + (b >= 33)) % 3]
        rows.append([6, c1, c2, 7 if b % 2 == 0 else -1, 0 if b % 4 == 1 else -1,
                     mid[(b + 2) % 3], -1, -1])
    rows.append([0, 7, -1, -1, -1, -1, -1, -1])
    return torch.tensor(rows)[:, :nprobe].contiguous()


def ivf_oracle(q, corpus, bias, offsets, probes, k):
    """float64 (scores, rows) of the top-k restricted to the probed lists."""
    s = oracle(q, corpus, bias, 1)[2]
    row_list = torch.searchsorted(offsets[1:].contiguous(), torch.arange(corpus.shape[0]),
                                  right=True)
    allowed = (probes[:, :, None] == row_list[None, None, :]).any(dim=1)
    s = s.masked_fill(~allowed, float("-inf"))
    top, rows = torch.sort(s, dim=1, descending=True, stable=True)
    top, rows = top[:, :k], rows[:, :k]
    return top, rows.masked_fill(top == float("-inf"), -1)


def _equals_oracle(q, corpus, bias, offsets, probes, k, splits, device):
    ref_s, ref_i = ivf_oracle(q, corpus, bias, offsets, probes, k)
    for qd in (q.to(device), q.bfloat16().to(device)):  # both query dtypes
        s, i = ops.ivf_topk(qd, corpus.to(device), offsets.to(device), probes.to(device), k,
                            None if bias is None else bias.to(device), splits)
        assert s.dtype == torch.float32 and i.dtype == torch.int64
        assert torch.equal(i.cpu(), ref_i) and torch.equal(s.cpu().double(), ref_s)


@pytest.mark.gpu
@pytest.mark.parametrize("D,k,nprobe,splits,l2", EXACT)
def test_exact(D, k, nprobe, splits, l2):
    ops.hip_ops()
    _equals_oracle(*_ints(B, N, D, l2), OFFSETS, _probes(nprobe), k, splits, "cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("splits", [1, 4])
def test_overflow_order(splits):
    """Ascending scores: every step beats the running threshold, so the
    candidate buffers overflow at every step."""
    ops.hip_ops()
    q, c = _adversarial("ascending")
    offsets, probes = torch.tensor([0, 4096]), torch.zeros(3, 1, dtype=torch.int64)
    _equals_oracle(q, c, None, offsets, probes, 100, splits, "cuda")
    rows = ops.ivf_topk(q.cuda(), c.cuda(), offsets.cuda(), probes.cuda(), 100, None, splits)[1]
    assert torch.equal(rows.cpu(), torch.arange(4095, 3995, -1).expand(3, -1))


@pytest.mark.gpu
def test_graph_replay():
    ops.hip_ops()
    q, c, _ = _ints(B, N, 96, False)
    args = (q.cuda(), c.cuda(), OFFSETS.cuda(), _probes(8).cuda(), 10)
    eager = ops.ivf_topk(*args)
    ops.ivf_topk(*args)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.ivf_topk(*args)
    for _ in range(3):
        out[0].zero_()
        out[1].zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out[0], eager[0]) and torch.equal(out[1], eager[1])


@pytest.mark.parametrize("case", [EXACT[1], EXACT[5]])
def test_cpu_path_equals_oracle(case):
    D, k, nprobe, _, l2 = case
    _equals_oracle(*_ints(B, N, D, l2), OFFSETS, _probes(nprobe), k, 0, "cpu")


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda", marks=pytest.mark.gpu)])
def test_ivf_index(device, metric):
    n, D, nlist, k = 2000, 24, 16, 10
    gen = torch.Generator().manual_seed(11)
    q, c = _draw(gen, 17, D).float(), _draw(gen, n, D, scale=D ** -0.5).float()
    ext = torch.arange(n) * 3 + 7
    index = IVFFlatIndex(D, nlist, nprobe=nlist, metric=metric, device=torch.device(device))
    with pytest.raises(RuntimeError, match="train"):
        index.search(q, k)
    with pytest.raises(RuntimeError, match="train"):
        index.add(c)
    index.train(c)
    index.add(c[:700], ext[:700])
    index.add(c[700:], ext[700:])
    assert len(index) == n and index.is_trained
    with pytest.raises(ValueError, match="nprobe"):
        index.nprobe = nlist + 1
    qd = q.to(device)
    l2 = metric == "l2"

    def search(nprobe):
        """index.search, checked to be coarse stage + ivf_topk + id map +
        distance conversion of the index's own buffers; returns the probes and
        the kernel-side (scores, storage rows)."""
        index.nprobe = nprobe
        dist, ids = index.search(qd, k)
        probes = ops.mips_topk(qd, index.centroids, nprobe, index.centroid_bias if l2 else None)[1]
        s, rows = ops.ivf_topk(qd, index.corpus[:n], index.list_offsets, probes, k,
                               index.bias[:n] if l2 else None)
        assert torch.equal(ids, index.ids[rows])
        assert torch.equal(dist, qd.bfloat16().float().square().sum(1, keepdim=True) - 2 * s
                           if l2 else s)
        return probes.cpu(), s.cpu(), rows.cpu()

    # every list probed: the search is exhaustive, and no row was lost or
    # duplicated on the way into the lists
    _, s, rows = search(nlist)
    corpus, offsets = index.corpus[:n].cpu(), index.list_offsets.cpu()
    bias = index.bias[:n].cpu() if l2 else None
    assert offsets[0] == 0 and offsets[-1] == n and (offsets.diff() >= 0).all()
    assert torch.equal(corpus[:, :D], c.bfloat16()[(index.ids[:n].cpu() - 7) // 3])
    assert torch.equal(index.ids[:n].cpu().sort().values, ext)
    _check_real(q, corpus, bias, k, s, rows)

    # two lists probed: the oracle restricted to the lists the coarse stage picks
    probes, s, rows = search(2)
    ref_s, ref_rows = ivf_oracle(q, corpus, bias, offsets, probes, k)
    if device == "cpu":
        assert torch.equal(rows, ref_rows)
    for b in range(q.shape[0]):  # the real-valued criterion inside each query's lists
        sub = torch.cat([torch.arange(offsets[p], offsets[p + 1]) for p in probes[b].sort().values])
        _check_real(q[b:b + 1], corpus[sub], None if bias is None else bias[sub], k,
                    s[b:b + 1], torch.searchsorted(sub, rows[b:b + 1]))

    clone = IVFFlatIndex(D, nlist, nprobe=2, metric=metric, device=torch.device(device))
    clone.load_state_dict(index.state_dict())
    assert len(clone) == n and clone.is_trained
    assert all(torch.equal(a, b) for a, b in zip(clone.search(qd, k), index.search(qd, k)))
