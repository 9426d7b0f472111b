"""FP8 (e4m3fn) rowwise-scaled rows on the quantized inference path.

Row: ``[e4m3fn codes: D bytes][fp16 scale][2 zero bytes][zero padding]``
(torchrec_amd/quant/embedding_modules.py). The CPU implementation there is the
reference; the GPU tests check the HIP kernels against it and against a
float64 oracle built from the packed bytes alone.

Round-trip bound (derived, no free constant). With ``s`` the stored scale,
``r = fl(x/s)``, ``c = e4m3(r)`` and ``w = fl(c*s)``:

    |w - x| <= max(2^-4 * |x|, 2^-10 * s) * (1 + 2^-20) + 2^-22 * |x|

half an e4m3 ulp for normals (3 mantissa bits), half the subnormal step 2^-9
below 2^-6, and the two fp32 roundings. A quantiser that truncates instead of
rounding, and a decode of the same bytes as e4m3fnuz, both break it
(``TestBoundHasTeeth``).

Lookup tolerance: the form of tests/test_quant_output_dtype.py,
``u*|y| + (n+6) * 2^-24 * S * (1+u)`` with ``S = sum |w_i| * |decode*scale|``
and ``u = 0`` at fp32 output. The FP8 path makes at most ``n + 5`` fp32
roundings (one for decode*scale, one for the weight, n adds, two for MEAN).
The oracle here is that file's ``pooled_oracle`` with an FP8 arm; its integer
arm is that file's ``table64``.
"""

import functools

import pytest
import torch

from tests.test_quant_nbit import (
    MIXED_B,
    MIXED_ROWS,
    gpu_copy_of,
    make_kjt,
    mixed_dtypes,
    mixed_float_ebc,
    roundtrip_inputs,
    small_dlrm,
)
from tests.test_quant_output_dtype import (
    OUT_CODE,
    UNIT_ROUNDOFF,
    cuda_kjt,
    direct_tbe,
    empty_bag_columns,
    random_bags,
    seq_feat_val_offsets,
    seq_rows,
    table64 as int_table64,
)
from torchrec_amd.inference.modules import quantize_inference_model
from torchrec_amd.modules.embedding_configs import (
    DATA_TYPE_NUM_BITS,
    DataType,
    EmbeddingBagConfig,
    EmbeddingConfig,
    PoolingType,
    data_type_to_dtype,
)
from torchrec_amd.modules.embedding_modules import EmbeddingCollection
from torchrec_amd.quant import (
    dequantize_rowwise_fp8,
    fp8_row_stride,
    quantize_rowwise_fp8,
)
from torchrec_amd.quant.embedding_modules import (
    FP8_FORMAT_CODE,
    EmbeddingBagCollection as QuantEBC,
    EmbeddingCollection as QuantEC,
    QuantTableBatchedEmbeddingBags,
    int8_row_stride,
    quant_data_type,
)
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

FP8 = DataType.FP8
E4M3 = torch.float8_e4m3fn
NAN_CODES = (0x7F, 0xFF)
ALL_DTYPES = [torch.float32, torch.bfloat16, torch.float16]


# ---------------------------------------------------------------------------
# packed-row helpers, the bound, inputs
# ---------------------------------------------------------------------------


def codes_of(packed: torch.Tensor, D: int) -> torch.Tensor:
    return packed[:, :D].contiguous()


def scale_of(packed: torch.Tensor, D: int) -> torch.Tensor:
    """The stored fp16 scale widened to float32, [R]."""
    R = packed.shape[0]
    return packed[:, D : D + 2].contiguous().view(torch.float16).reshape(R).float()


def decode(codes: torch.Tensor, dtype=E4M3) -> torch.Tensor:
    return codes.view(dtype).float()


def fp8_bound(x: torch.Tensor, s: torch.Tensor) -> torch.Tensor:
    """The module docstring's bound, float64 [R, D]; ``s`` is the stored scale [R]."""
    ax = x.double().abs()
    half_step = torch.maximum(2.0**-4 * ax, 2.0**-10 * s.double().unsqueeze(1))
    return half_step * (1 + 2.0**-20) + 2.0**-22 * ax


def special_rows(D: int) -> torch.Tensor:
    """[4, D]: all zero; negative only; one 1e3 outlier among 1e-3 entries
    (they land in e4m3 subnormals or zero); amax = 1e-30 (the scale becomes the
    smallest fp16 subnormal)."""
    g = torch.Generator().manual_seed(11)
    zero = torch.zeros(D)
    negative = -(torch.rand(D, generator=g) + 0.05)
    outlier = 1e-3 * (1 + torch.rand(D, generator=g))
    outlier[::2] *= -1
    outlier[D // 2] = 1e3
    tiny = 1e-30 * (2 * torch.rand(D, generator=g) - 1)
    tiny[0] = 1e-30
    return torch.stack([zero, negative, outlier, tiny])


def fp8_inputs(R: int, D: int):
    families = dict(roundtrip_inputs(R, D))
    families["special"] = special_rows(D)
    return families


def check_rows(x: torch.Tensor, packed: torch.Tensor, what: str) -> None:
    """Everything test 1 asserts of a packed row; the GPU rows must meet it too."""
    R, D = x.shape
    assert packed.dtype == torch.uint8 and packed.shape == (R, fp8_row_stride(D)), what
    codes = codes_of(packed, D)
    s = scale_of(packed, D)
    for nan_code in NAN_CODES:
        assert not (codes == nan_code).any(), f"{what}: NaN code {nan_code:#x} produced"
    assert not packed[:, D + 2 :].any(), f"{what}: reserved bytes / padding not zero"
    amax = x.abs().amax(dim=1)
    live = amax > 0
    assert (s[live] > 0).all(), what
    assert (x[live].double().abs() / s[live].double().unsqueeze(1) <= 448).all(), what
    dead = ~live
    assert (s[dead] == 0).all() and not codes[dead].any(), f"{what}: zero row"
    deq = dequantize_rowwise_fp8(packed, D)
    assert (deq[dead] == 0).all(), f"{what}: zero row must dequantise to exact zeros"
    err = (deq.double() - x.double()).abs()
    bound = fp8_bound(x, s)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst err/bound {ratio:.4f}")
    assert (err <= bound).all(), f"{what}: worst err/bound {ratio}"


def with_codes(packed: torch.Tensor, codes: torch.Tensor) -> torch.Tensor:
    out = packed.clone()
    out[:, : codes.shape[1]] = codes
    return out


def truncating_codes(x: torch.Tensor, packed: torch.Tensor) -> torch.Tensor:
    """The codes a round-toward-zero quantiser would give: the round-to-nearest
    code, one step down in magnitude wherever it overshot |x/s|."""
    D = x.shape[1]
    s = scale_of(packed, D).unsqueeze(1)
    r = torch.where(s == 0, torch.zeros_like(x), x / s)
    codes = codes_of(packed, D)
    over = decode(codes).abs() > r.abs()  # then the magnitude bits are >= 1
    return codes - over.to(torch.uint8)


# ---------------------------------------------------------------------------
# float64 oracle from the packed bytes (integer tables: test_quant_output_dtype's)
# ---------------------------------------------------------------------------


def table64(tbe: QuantTableBatchedEmbeddingBags, t: int):
    """(w64, a64), both [rows, D]: the dequantised row and |decode*scale|."""
    if tbe._weight_dtypes[t] is not FP8:
        return int_table64(tbe, t)
    D = tbe._specs[t][2]
    packed = tbe.packed_table(t).cpu()
    w64 = decode(codes_of(packed, D)).double() * scale_of(packed, D).double().unsqueeze(1)
    return w64, w64.abs()


def pooled_oracle(tbe, indices, offsets, psw, mean: bool):
    """(y64, S, n), each [B, total_D] float64, for a pooled lookup."""
    F = tbe._num_features
    B = (offsets.numel() - 1) // F
    ys, Ss, ns = [], [], []
    for f, t in enumerate(tbe._feature_table_map):
        w64, a64 = table64(tbe, t)
        D = w64.shape[1]
        y = torch.zeros(B, D, dtype=torch.float64)
        S = torch.zeros(B, D, dtype=torch.float64)
        n = torch.zeros(B, D, dtype=torch.float64)
        for b in range(B):
            lo, hi = int(offsets[f * B + b]), int(offsets[f * B + b + 1])
            if hi == lo:
                continue
            idx = indices[lo:hi]
            w = (
                psw[lo:hi].double().unsqueeze(1)
                if psw is not None
                else torch.ones(hi - lo, 1, dtype=torch.float64)
            )
            div = float(hi - lo) if mean else 1.0
            y[b] = (w * w64[idx]).sum(0) / div
            S[b] = (w.abs() * a64[idx]).sum(0) / div
            n[b] = hi - lo
        ys.append(y)
        Ss.append(S)
        ns.append(n)
    return torch.cat(ys, 1), torch.cat(Ss, 1), torch.cat(ns, 1)


def seq_oracle(tbe, indices, feat_val_offsets):
    ys, Ss = [], []
    for f, t in enumerate(tbe._feature_table_map):
        w64, a64 = table64(tbe, t)
        idx = indices[int(feat_val_offsets[f]) : int(feat_val_offsets[f + 1])]
        ys.append(w64[idx])
        Ss.append(a64[idx])
    return torch.cat(ys, 0), torch.cat(Ss, 0)


def tolerance(y64, S, n, dt):
    u = UNIT_ROUNDOFF.get(dt, 0.0)  # fp32 output: no second rounding
    tol = u * y64.abs() + (n + 6) * 2.0**-24 * S * (1 + u)
    return tol + 2.0**-25 if dt == torch.float16 else tol


def assert_within(out, y64, S, n, dt, what=""):
    assert out.dtype == dt, f"{what}: dtype {out.dtype}, want {dt}"
    assert out.shape == y64.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(y64.shape)}"
    assert float(y64.abs().max()) > 0, f"{what}: vacuous"
    err = (out.detach().cpu().double() - y64).abs()
    tol = tolerance(y64, S, n, dt)
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{what} {dt}: worst err/tol {worst:.4f}")
    assert (err <= tol).all(), f"{what} {dt}: worst err/tol {worst}"


# ---------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------

# An FP8 D=20 table in front of an INT4 one: the INT4 segment starts at
# element 20, a multiple of 4 elements only. D=264 is 66 FP8 units (two chunks).
MIXED_FP8 = [  # (name, D, format, features)
    ("p0", 20, FP8, ["f0"]),
    ("p1", 8, DataType.INT4, ["f1"]),
    ("p2", 264, FP8, ["f2", "f3"]),
    ("p3", 20, DataType.INT8, ["f4"]),
    ("p4", 16, DataType.INT2, ["f5"]),
]
MIXED_FP8_KEYS = [f for s in MIXED_FP8 for f in s[3]]
MIXED_FP8_D = sum(s[1] * len(s[3]) for s in MIXED_FP8)

POOL_MODES = [(False, False), (True, False), (False, True)]
POOL_IDS = ["sum", "mean", "weighted"]


@functools.lru_cache(maxsize=None)
def mixed_case(mean: bool, weighted: bool):
    pooling = PoolingType.MEAN if mean else PoolingType.SUM
    ebc = mixed_float_ebc(pooling, weighted, specs=MIXED_FP8)
    # the first and the last bag are empty, and feature f4 has no values at all
    kjt = make_kjt(MIXED_FP8_KEYS, MIXED_ROWS, MIXED_B, weighted, empty_key="f4")
    make = lambda dt=torch.float32: QuantEBC.from_float(
        ebc, output_dtype=dt, per_table_weight_dtype=mixed_dtypes(MIXED_FP8)
    )
    ref = make()
    psw = kjt.weights() if weighted else None
    oracle = pooled_oracle(ref._tbe, kjt.values(), kjt.offsets(), psw, mean)
    return make, kjt, oracle


SEQ_FP8 = [("s0", 32, FP8, ["fa", "fe"]), ("s1", 32, DataType.INT4, ["fb"])]
SEQ_FP8_ROWS = 25


@functools.lru_cache(maxsize=None)
def seq_case():
    torch.manual_seed(0)
    ec = EmbeddingCollection(
        tables=[
            EmbeddingConfig(
                num_embeddings=SEQ_FP8_ROWS, embedding_dim=D, name=n, feature_names=list(fs)
            )
            for (n, D, _, fs) in SEQ_FP8
        ]
    )
    make = lambda dt=torch.float32: QuantEC.from_float(
        ec, output_dtype=dt, per_table_weight_dtype=mixed_dtypes(SEQ_FP8)
    )
    ref = make()
    kjt = make_kjt(["fa", "fe", "fb"], SEQ_FP8_ROWS, 4, empty_key="fe")  # "fe" is empty
    assert kjt.keys() == ref._feature_names
    fvo = seq_feat_val_offsets(kjt, len(ref._feature_names))
    return make, kjt, seq_oracle(ref._tbe, kjt.values(), fvo)


def code_table_tbe(device=None) -> QuantTableBatchedEmbeddingBags:
    """One D=256 FP8 row written by hand: codes 0..255, scale 1.0."""
    tbe = QuantTableBatchedEmbeddingBags([("codes", 1, 256)], weight_dtypes=[FP8], device=device)
    row = torch.zeros(fp8_row_stride(256), dtype=torch.uint8)
    row[:256] = torch.arange(256, dtype=torch.uint8)
    row[256:258] = torch.tensor([1.0], dtype=torch.float16).view(torch.uint8)
    tbe.packed_table(0).copy_(row.unsqueeze(0))
    return tbe


def assert_is_decode_table(got: torch.Tensor, bitwise: bool = True) -> None:
    """``got`` [256] fp32 equals torch's e4m3fn decode of codes 0..255: bitwise
    where finite, NaN exactly at the two NaN codes. ``bitwise=False`` compares
    by value: a pool starts at +0, so code 0x80 (-0) comes out as +0."""
    want = decode(torch.arange(256, dtype=torch.uint8))
    nan = torch.zeros(256, dtype=torch.bool)
    nan[list(NAN_CODES)] = True
    assert torch.equal(want.isnan(), nan)  # what e4m3fn means
    assert want[0x7E] == 448 and want[0x01] == 2.0**-9 and want[0x38] == 1
    got = got.detach().cpu()
    assert got.dtype == torch.float32 and got.shape == (256,)
    assert torch.equal(got.isnan(), nan)
    if bitwise:
        assert torch.equal(got[~nan].view(torch.int32), want[~nan].view(torch.int32))
    else:
        assert torch.equal(got[~nan], want[~nan])


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------


class TestFp8Cpu:
    def test_data_type(self):
        assert DataType.FP8.value == "FP8" and str(DataType.FP8) == "FP8"
        assert DATA_TYPE_NUM_BITS[FP8] == 8
        assert data_type_to_dtype(FP8) == torch.uint8
        assert quant_data_type(FP8) is FP8 and quant_data_type("FP8") is FP8
        assert FP8_FORMAT_CODE != 8

    @pytest.mark.parametrize("D,stride", [(4, 16), (12, 16), (20, 32), (128, 144), (260, 272)])
    def test_stride_is_the_int8_stride(self, D, stride):
        assert fp8_row_stride(D) == stride == int8_row_stride(D)

    @pytest.mark.parametrize("D", [4, 12, 20, 64, 260])
    def test_roundtrip_error_bound(self, D):
        for name, x in fp8_inputs(64, D).items():
            check_rows(x, quantize_rowwise_fp8(x), f"D={D} {name}")

    def test_special_rows_are_what_they_claim(self):
        x = special_rows(64)
        packed = quantize_rowwise_fp8(x)
        s = scale_of(packed, 64)
        assert s[0] == 0
        assert (x[1] < 0).all() and (codes_of(packed, 64)[1] >= 0x80).all()
        small = decode(codes_of(packed, 64))[2].abs() < 2.0**-6  # subnormal or zero
        assert int(small.sum()) == 63
        assert s[3] == 2.0**-24  # the smallest fp16 subnormal
        # the scale is rounded UP: never below amax / 448
        assert (s.double() * 448 >= x.abs().amax(dim=1).double()).all()

    def test_empty_table(self):
        assert quantize_rowwise_fp8(torch.zeros(0, 8)).shape == (0, 16)

    def test_state_dict_roundtrip(self):
        ebc = mixed_float_ebc(specs=MIXED_FP8)
        q = QuantEBC.from_float(ebc, per_table_weight_dtype=mixed_dtypes(MIXED_FP8))
        fresh = QuantEBC(tables=q.embedding_bag_configs())
        assert not torch.equal(fresh._tbe.qweights, q._tbe.qweights)
        fresh.load_state_dict(q.state_dict())
        assert torch.equal(fresh._tbe.qweights, q._tbe.qweights)
        kjt = make_kjt(MIXED_FP8_KEYS, MIXED_ROWS, MIXED_B)
        assert torch.equal(fresh(kjt).values(), q(kjt).values())

    def test_decode_table(self):
        assert_is_decode_table(code_table_tbe().dequantized_table(0)[0])

    @pytest.mark.parametrize("mean,weighted", POOL_MODES, ids=POOL_IDS)
    def test_mixed_ebc_vs_oracle(self, mean, weighted):
        make, kjt, (y, S, n) = mixed_case(mean, weighted)
        q = make()
        assert [c.data_type for c in q.embedding_bag_configs()] == [s[2] for s in MIXED_FP8]
        for t, (_, D, dt, _) in enumerate(MIXED_FP8):
            if dt is FP8:  # the bytes are the FP8 quantiser's
                w = mixed_float_ebc(specs=MIXED_FP8).embedding_bags[f"p{t}"].weight.detach()
                assert torch.equal(q._tbe.packed_table(t), quantize_rowwise_fp8(w))
        out = q(kjt).values()
        assert out.shape == (MIXED_B, MIXED_FP8_D)
        assert_within(out, y, S, n, torch.float32, "cpu mixed")
        assert (out[empty_bag_columns(kjt, q._tbe)] == 0).all()

    def test_uniform_from_float(self):
        ebc = mixed_float_ebc(specs=MIXED_FP8)
        q = QuantEBC.from_float(ebc, weight_dtype=FP8)
        assert [c.data_type for c in q.embedding_bag_configs()] == [FP8] * len(MIXED_FP8)
        assert not q._tbe._all_int8
        kjt = make_kjt(MIXED_FP8_KEYS, MIXED_ROWS, MIXED_B)
        y, S, n = pooled_oracle(q._tbe, kjt.values(), kjt.offsets(), None, False)
        assert_within(q(kjt).values(), y, S, n, torch.float32, "cpu uniform")

    @pytest.mark.parametrize("dt", ALL_DTYPES)
    def test_seq_ec_vs_oracle(self, dt):
        make, kjt, (y, S) = seq_case()
        q = make(dt)
        assert [c.data_type for c in q.embedding_configs()] == [FP8, DataType.INT4]
        out = q(kjt)
        assert out["fe"].values().shape == (0, 32) and out["fe"].values().dtype == dt
        assert_within(seq_rows(out, q._feature_names), y, S, torch.ones_like(y), dt, "cpu seq")

    def test_quantize_inference_model(self):
        model = small_dlrm()
        w0 = model.sparse_arch.embedding_bag_collection.embedding_bags["t0"].weight.detach().clone()
        quantize_inference_model(model, weight_dtype=FP8)
        q = model.sparse_arch.embedding_bag_collection
        assert isinstance(q, QuantEBC)
        assert [c.data_type for c in q.embedding_bag_configs()] == [FP8, FP8]
        assert q._tbe.qweights.numel() == 2 * 50 * fp8_row_stride(8)
        assert torch.equal(q._tbe.packed_table(0), quantize_rowwise_fp8(w0))
        out = model.sparse_arch(make_kjt(["f0", "f1"], 50, 3))
        assert out.shape == (3, 2, 8) and out.dtype == torch.float32

    def test_bad_dim_names_the_table(self):
        with pytest.raises(ValueError, match="bad6"):
            QuantEBC(
                tables=[
                    EmbeddingBagConfig(num_embeddings=4, embedding_dim=6, name="bad6", data_type=FP8)
                ]
            )
        with pytest.raises(ValueError, match="bad6"):
            QuantTableBatchedEmbeddingBags([("bad6", 4, 6)], weight_dtypes=[FP8])
        with pytest.raises(ValueError):
            fp8_row_stride(6)
        with pytest.raises(ValueError):
            quantize_rowwise_fp8(torch.zeros(2, 6))


class TestBoundHasTeeth:
    @pytest.mark.parametrize("D", [20, 64])
    def test_truncation_violates_bound_on_every_family(self, D):
        for name, x in fp8_inputs(64, D).items():
            packed = quantize_rowwise_fp8(x)
            trunc = with_codes(packed, truncating_codes(x, packed))
            err = (dequantize_rowwise_fp8(trunc, D).double() - x.double()).abs()
            n_bad = int((err > fp8_bound(x, scale_of(packed, D))).sum())
            print(f"D={D} {name}: truncation breaks the bound at {n_bad}/{x.numel()} elements")
            assert n_bad > 0, name

    @pytest.mark.parametrize("D", [20, 64])
    def test_fnuz_decode_violates_bound_on_every_family(self, D):
        for name, x in fp8_inputs(64, D).items():
            packed = quantize_rowwise_fp8(x)
            s = scale_of(packed, D)
            fnuz = decode(codes_of(packed, D), torch.float8_e4m3fnuz) * s.unsqueeze(1)
            err = (fnuz.double() - x.double()).abs()  # NaN (fnuz 0x80) compares False
            n_bad = int((err > fp8_bound(x, s)).sum())
            print(f"D={D} {name}: an fnuz decode breaks the bound at {n_bad}/{x.numel()} elements")
            assert n_bad > 0, name


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------


def magnitude_ordinal(codes: torch.Tensor) -> torch.Tensor:
    """Position of a code in e4m3's value ordering: +0 and -0 share 0."""
    c = codes.int()
    return (c & 0x7F) * (1 - 2 * (c >> 7))


@pytest.mark.gpu
class TestFp8Gpu:
    @pytest.mark.parametrize("R", [1, 100])
    @pytest.mark.parametrize("D", [4, 12, 20, 64, 260, 1028])
    def test_quantize_kernel_matches_cpu(self, D, R):
        g = torch.Generator().manual_seed(R * 1000 + D)
        x = torch.randn(R, D, generator=g)
        if R > 1:
            x[:4] = special_rows(D)
            x[4] = 100 * torch.rand(D, generator=g) - 20
            x[5] = 0.37
            x[6] = 0.01 * torch.randn(D, generator=g) + 3
        ref = quantize_rowwise_fp8(x)
        got = quantize_rowwise_fp8(x.cuda())
        torch.cuda.synchronize()
        got = got.cpu()
        assert got.shape == ref.shape and got.dtype == torch.uint8
        # scale, reserved bytes and padding: bytewise
        assert torch.equal(got[:, D:], ref[:, D:])
        step = (magnitude_ordinal(codes_of(got, D)) - magnitude_ordinal(codes_of(ref, D))).abs()
        n_diff = int((codes_of(got, D) != codes_of(ref, D)).sum())
        print(f"D={D} R={R}: codes differing from the CPU's {n_diff}/{R * D}, max step {int(step.max())}")
        assert int(step.max()) <= 1
        check_rows(x, got, f"gpu D={D} R={R}")

    def test_quantize_op_edges(self):
        empty = torch.ops.trec_amd.quantize_rowwise_fp8(torch.zeros(0, 8, device="cuda"))
        assert empty.shape == (0, 16) and empty.dtype == torch.uint8 and empty.is_cuda
        with pytest.raises(RuntimeError):
            torch.ops.trec_amd.quantize_rowwise_fp8(torch.zeros(2, 6, device="cuda"))

    def test_decode_table_on_device(self):
        """Every code through the convert instruction: tells OCP e4m3fn from fnuz."""
        tbe = code_table_tbe(torch.device("cuda"))
        dev = torch.device("cuda")
        out = torch.ops.trec_amd.tbe_forward_seq_nbit(
            tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._weight_bits_t,
            tbe._feat_table_t, torch.tensor([0, 1], device=dev), torch.tensor([0], device=dev),
            256, 64, 0)
        torch.cuda.synchronize()
        assert out.shape == (1, 256)
        assert_is_decode_table(out[0])
        # and through the pooled kernel: a one-row bag
        pooled = tbe(torch.tensor([0], device=dev), torch.tensor([0, 1], device=dev))
        torch.cuda.synchronize()
        assert_is_decode_table(pooled[0], bitwise=False)

    @pytest.mark.parametrize("dt", ALL_DTYPES)
    @pytest.mark.parametrize("mean,weighted", POOL_MODES, ids=POOL_IDS)
    def test_mixed_pooled(self, mean, weighted, dt):
        make, kjt, (y, S, n) = mixed_case(mean, weighted)
        q_cpu = make(dt)
        q = gpu_copy_of(q_cpu, lambda: make(dt))
        out = q(cuda_kjt(kjt)).values()
        torch.cuda.synchronize()
        assert out.is_cuda
        assert_within(out, y, S, n, dt, "gpu mixed")
        assert (out.cpu()[empty_bag_columns(kjt, q_cpu._tbe)] == 0).all()

    @pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
    @pytest.mark.parametrize("D,rows,B", [(64, 5, 3), (260, 4, 3), (1028, 3, 2)])
    def test_uniform_fp8_chunk_boundaries(self, D, rows, B, dt):
        """16 units; 65 units (two chunks, ragged tail); 257 units (64 x 8)."""
        specs = [("u", D, FP8, ["h"])]
        ebc = mixed_float_ebc(specs=specs, rows=rows)
        make = lambda: QuantEBC.from_float(ebc, output_dtype=dt, weight_dtype=FP8)
        q_cpu = make()
        q = gpu_copy_of(q_cpu, make)
        assert q._tbe._max_units == D // 4
        lengths = torch.tensor([3, 0, 2][:B])
        values = torch.arange(int(lengths.sum())) % rows
        kjt = KeyedJaggedTensor(keys=["h"], values=values, lengths=lengths, stride=B)
        y, S, n = pooled_oracle(q_cpu._tbe, kjt.values(), kjt.offsets(), None, False)
        out = q(cuda_kjt(kjt)).values()
        torch.cuda.synchronize()
        assert_within(out, y, S, n, dt, f"gpu uniform D={D}")
        assert (out[1] == 0).all()

    @pytest.mark.parametrize("dt", ALL_DTYPES)
    def test_seq(self, dt):
        make, kjt, (y, S) = seq_case()
        q_cpu = make(dt)
        q = gpu_copy_of(q_cpu, lambda: make(dt))
        out = q(cuda_kjt(kjt))
        torch.cuda.synchronize()
        assert out["fe"].values().shape == (0, 32) and out["fe"].values().dtype == dt
        assert_within(seq_rows(out, q._feature_names), y, S, torch.ones_like(y), dt, "gpu seq")

    @pytest.mark.parametrize("dt", ALL_DTYPES)
    def test_seq_leaves_tail_untouched(self, dt):
        """A D=8 FP8 table in a D_out=20 output: columns past D are not written.
        The output is allocated inside the op, so the guard is a sentinel-filled
        block of the same size released just before the call; when the allocator
        hands the op that block, the columns past D must still hold the sentinel."""
        specs = [("a", 12, 8), ("b", 9, 16)]
        tbe = direct_tbe(specs, [FP8, DataType.INT2])
        indices, offsets, _ = random_bags(specs, 4)
        fvo = offsets[::4][:3].contiguous().cuda()
        idx = indices.cuda()
        n0, N = int(fvo[1]), indices.numel()
        assert 0 < n0 < N
        args = (tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._weight_bits_t,
                tbe._feat_table_t, fvo, idx)
        w64a, a64a = table64(tbe, 0)
        w64b, a64b = table64(tbe, 1)
        D_out = 20
        torch.cuda.synchronize()
        guard = torch.full((N, D_out), -7.0, dtype=dt, device="cuda")
        ptr = guard.data_ptr()
        del guard
        out = torch.ops.trec_amd.tbe_forward_seq_nbit(*args, D_out, 2, OUT_CODE[dt])
        torch.cuda.synchronize()
        assert out.dtype == dt and out.shape == (N, D_out)
        reused = out.data_ptr() == ptr
        print(f"{dt}: guard block reused: {reused}")
        if reused:
            assert (out[:n0, 8:] == -7.0).all()  # past the FP8 table's D
            assert (out[n0:, 16:] == -7.0).all()
        one = torch.ones(N, 1, dtype=torch.float64)
        assert_within(out[:n0, :8], w64a[indices[:n0]], a64a[indices[:n0]], one[:n0], dt, "a")
        assert_within(out[n0:, :16], w64b[indices[n0:]], a64b[indices[n0:]], one[n0:], dt, "b")
        # D_out narrower than the FP8 table's D: the row is cut at D_out
        cut = torch.ops.trec_amd.tbe_forward_seq_nbit(*args, 4, 2, OUT_CODE[dt])
        torch.cuda.synchronize()
        assert cut.shape == (N, 4) and torch.equal(cut[:n0], out[:n0, :4])

    def test_graph_capture_replays_eager(self):
        """One capture and replay of the FP8 pooled forward (a single kernel,
        no parallel branches) reproduces the eager output bit for bit."""
        make, kjt, _ = mixed_case(False, False)
        q = gpu_copy_of(make(), make)
        tbe = q._tbe
        idx, off = kjt.values().cuda(), kjt.offsets().cuda()
        eager = tbe(idx, off).clone()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = tbe(idx, off)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert float(eager.abs().max()) > 0
        assert torch.equal(out, eager)

    def test_end_to_end_from_float_on_gpu(self):
        """GPU quantiser feeds the GPU lookup: a float EBC on the device quantised
        there, against the float64 oracle of its own packed bytes."""
        ebc = mixed_float_ebc(specs=MIXED_FP8)
        kjt = make_kjt(MIXED_FP8_KEYS, MIXED_ROWS, MIXED_B)
        ebc.to(torch.device("cuda"))
        q = QuantEBC.from_float(ebc, per_table_weight_dtype=mixed_dtypes(MIXED_FP8))
        assert q._tbe.qweights.is_cuda
        out = q(cuda_kjt(kjt)).values()
        torch.cuda.synchronize()
        y, S, n = pooled_oracle(q._tbe, kjt.values(), kjt.offsets(), None, False)
        assert_within(out, y, S, n, torch.float32, "gpu end to end")
