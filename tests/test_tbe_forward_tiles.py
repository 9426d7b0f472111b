"""Pooled TBE forward: tiles of consecutive bags, coalesced offsets / indices
rounds and row flights (torchrec_amd/ops/csrc/tbe.hip).

Two yardsticks, both exact:

* a float64 gather-and-sum on dyadic inputs (weights = integers in [-8, 8] / 8,
  psw in {0.5, 1, 2}). Every partial sum is then exact in fp32 and the result
  is exact in the output type, whatever the order of the adds; the test checks
  that claim on the CPU before it trusts it. A 16-bit output keeps 8 (bf16)
  significant bits, so those cases shrink the weight magnitude until
  max bag length x magnitude x psw range fits in them.
* the previous kernel's outputs on arbitrary real weights, recorded bit for
  bit under tests/golden/tbe_forward_tiles by tests/tbe_forward_tiles_cases.py.
  They pin the order of the adds, which exact sums cannot see.

An over-read cannot fault here: the index, offset, psw and cache_loc views sit
inside larger buffers whose other entries are valid and point at a poison row
(4096.0) or a poison weight (64.0), so an over-read that is accumulated shows
as a wrong sum.
"""

import os

import numpy as np
import pytest
import torch

from tests import tbe_forward_tiles_cases as C

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "tbe_forward_tiles")


def _lens(seed, n, menu=C.LENGTHS):
    return C.mixed_lengths(np.random.default_rng(seed), n, menu)


def _mag16(lengths, psw, odtype):
    """Largest integer weight magnitude (in eighths) whose sums a 16-bit
    output still holds exactly: terms are multiples of 1/16 (psw 0.5) of at
    most mag / 8 * 2, so |sum| * 16 <= len * mag * 4 must stay below 2^8."""
    if odtype == "fp32":
        return 8
    per_term = 4 if psw else 1
    mag = 255 // (max(1, int(np.max(lengths))) * per_term)
    return min(8, mag)


def _exact_case(seed, dims, ft, B, lengths, **kw):
    mag = _mag16(lengths, kw.get("psw", False), kw.get("odtype", "fp32"))
    assert mag >= 1, "bag too long for an exact 16-bit sum: shorten the menu"
    return C.make_case(seed, dims, ft, B, lengths, mag=mag, **kw)


def _expected_exact(case):
    """float64 oracle, after checking on the CPU that it is legitimate: the
    fp32 sequential sum equals it, and the output type holds it."""
    exp = C.oracle64(case)
    seq = C.sequential32(case)
    assert np.array_equal(seq.astype(np.float64), exp), "inputs are not exactly summable"
    t = torch.from_numpy(exp)
    held = t.to(C.TORCH_DT[case["odtype"]]).to(torch.float64)
    assert torch.equal(held, t), "sum exceeds the output type's significant bits"
    return t


def _check_exact(case, embed=False):
    exp = _expected_exact(case)
    out = C.run_forward(case, "cuda", embed=embed)
    assert out.dtype == C.TORCH_DT[case["odtype"]]
    bad = (out.to(torch.float64) != exp).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} wrong elements, first at {bad[0].tolist()}"


# ---------------------------------------------------------------------------
# CPU: the oracle checks itself, and notices what it is meant to notice
# ---------------------------------------------------------------------------


def _cpu_case(**kw):
    B = 9
    return _exact_case(5, [4, 128], [0, 1, 1], B, _lens(5, 3 * B), **kw)


@pytest.mark.parametrize("psw", [False, True])
@pytest.mark.parametrize("mean", [False, True])
def test_oracle_sequential_fp32_equals_float64(psw, mean):
    menu = C.LENGTHS_POW2 if mean else C.LENGTHS
    case = _exact_case(6, [4, 64, 128], [0, 1, 2, 1], 9, _lens(6, 36, menu), psw=psw, mean=mean)
    _expected_exact(case)


@pytest.mark.parametrize("odtype", ["bf16", "fp16"])
def test_oracle_16bit_cap_holds(odtype):
    case = _exact_case(7, [64, 128], [0, 1, 1], 9, _lens(7, 27, [0, 1, 3, 4, 5, 31, 32, 33]),
                       psw=True, odtype=odtype)
    _expected_exact(case)


@pytest.mark.parametrize("mutant", ["drop_last", "neighbour", "no_psw"])
def test_oracle_catches_mutants(mutant):
    case = _cpu_case(psw=True)
    exp = C.oracle64(case)
    assert not np.array_equal(C.oracle64(case, mutant=mutant), exp)


def test_16bit_cap_rejects_long_bags():
    with pytest.raises(AssertionError):
        _exact_case(8, [64], [0], 1, np.asarray([70]), psw=True, odtype="bf16")


# ---------------------------------------------------------------------------
# GPU, exact sums
# ---------------------------------------------------------------------------

DIM_PAIRS = [(4, 128), (64, 128), (4, 64)]  # 32, 32 and 16 lanes per slot


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 31, 32, 33, 80])
@pytest.mark.parametrize("dims", DIM_PAIRS)
@pytest.mark.parametrize("psw", [False, True])
def test_sum_mixed_lengths(B, dims, psw):
    """F = 3 over 2 tables; fewer bags than a tile, ragged last tile, feature
    boundary mid-wave; all lengths of the menu mixed inside the tiles."""
    case = _exact_case(100 + B, list(dims), [0, 1, 0], B, _lens(B, 3 * B), psw=psw)
    _check_exact(case)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 31, 32, 33, 80])
@pytest.mark.parametrize("dims", DIM_PAIRS)
@pytest.mark.parametrize("psw", [False, True])
def test_mean_pow2_lengths(B, dims, psw):
    case = _exact_case(
        200 + B, list(dims), [0, 1, 1], B, _lens(B, 3 * B, C.LENGTHS_POW2), psw=psw, mean=True
    )
    _check_exact(case)


@pytest.mark.gpu
def test_mean_non_pow2_length():
    """fl32(sum) * fl32(1 / len), computed the same way in numpy float32."""
    B = 33
    case = C.make_case(9, [64, 128], [0, 1, 0], B, _lens(9, 3 * B), psw=True, mean=True)
    summed = dict(case, mean=False)
    _expected_exact(summed)  # the sums themselves are exact
    exp = C.sequential32(case)
    out = C.run_forward(case, "cuda")
    assert np.array_equal(out.numpy().view(np.int32), exp.view(np.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 256, 512, 1024, 2048])
@pytest.mark.parametrize("psw,mean", [(False, False), (True, True)])
def test_wide_rows(D, psw, mean):
    """CHUNKS 2 / 4 / 8 at 64 lanes per slot; D = 64 alone is 16 lanes."""
    B = 33
    menu = C.LENGTHS_POW2 if mean else C.LENGTHS
    case = _exact_case(300 + D, [D], [0, 0], B, _lens(D, 2 * B, menu), psw=psw, mean=mean)
    _check_exact(case)


@pytest.mark.gpu
@pytest.mark.parametrize("tdtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("odtype", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("psw", [False, True])
def test_dtype_cross(tdtype, odtype, psw):
    B = 33
    menu = [0, 1, 3, 4, 5, 31, 32, 33] if psw else C.LENGTHS
    case = _exact_case(
        400, [64, 128], [0, 1, 1], B, _lens(4, 3 * B, menu), tdtype=tdtype, odtype=odtype, psw=psw
    )
    _check_exact(case)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["one_tile", "whole_batch"])
def test_empty_tiles(which):
    """A tile whose bags are all empty stores zeros and reads no index."""
    B = 80
    lengths = _lens(10, 3 * B)
    if which == "whole_batch":
        lengths[:] = 0
    else:
        lengths[32:64] = 0  # feature 0, second tile of 32; covers two tiles of 16
    case = _exact_case(500, [64, 128], [0, 1, 1], B, lengths, psw=True)
    _check_exact(case, embed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("tdtype", ["fp32", "bf16"])
@pytest.mark.parametrize("dims", [(4, 128), (512,)])
def test_cached_hits_and_misses_share_a_flight(tdtype, dims):
    B = 33
    ft = [0, 1, 1] if len(dims) == 2 else [0, 0]
    case = _exact_case(
        600, list(dims), ft, B, _lens(11, len(ft) * B), tdtype=tdtype, psw=True, cached=True
    )
    loc = case["cache_loc"]
    runs = np.lib.stride_tricks.sliding_window_view(loc >= 0, 4)
    assert (runs.any(axis=1) & ~runs.all(axis=1)).any()
    _check_exact(case, embed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", DIM_PAIRS + [(512,)])
@pytest.mark.parametrize("mean", [False, True])
def test_views_into_larger_buffers(dims, mean):
    """Every over-read neighbour is a valid index of the poison row, a valid
    offset or a poison weight: accumulated, it is a wrong sum, never a fault."""
    B = 33
    ft = [0, 1, 0] if len(dims) == 2 else [0, 0]
    menu = C.LENGTHS_POW2 if mean else C.LENGTHS
    case = _exact_case(
        700, list(dims), ft, B, _lens(12, len(ft) * B, menu), psw=True, mean=mean
    )
    _check_exact(case, embed=True)


@pytest.mark.gpu
@pytest.mark.parametrize("dims", DIM_PAIRS + [(256,)])
def test_one_block_walks_many_tiles(dims, monkeypatch):
    """Grid cap of one block: each slot takes several tiles in turn, so the
    state carried from one tile to the next must start clean."""
    B = 80
    ft = [0, 1, 0, 1, 1, 0] if len(dims) == 2 else [0] * 6
    case = _exact_case(800, list(dims), ft, B, _lens(13, len(ft) * B), psw=True, cached=True)
    monkeypatch.setenv("TREC_FWD_GRID_CAP", "1")  # read on every call
    _check_exact(case, embed=True)


# ---------------------------------------------------------------------------
# GPU, parent pins
# ---------------------------------------------------------------------------


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(C.pin_cases()))
@pytest.mark.parametrize("embed", [False, True])
def test_bit_equal_to_previous_kernel(name, embed):
    case, out_bits = C.load_pin(os.path.join(GOLDEN, name + ".npz"))
    out = C.run_forward(case, "cuda", embed=embed)
    assert np.array_equal(C._bits(out), out_bits)

