"""``output_dtype`` (bf16 / fp16) on the quantized inference path.

Oracle: float64, computed from the packed bytes alone. The codes come from
``unpack_codes_nbit``, the stored fp16 scale and bias are widened to float64,
then the per-sample weights and the MEAN divide are applied in float64.

Bound (no free constant). For a bag of ``n`` rows let

    S = sum_i |w_i| * (|q_i * scale_i| + |bias_i|)      (divided by n for MEAN)

and ``u`` the output type's unit roundoff (2^-8 bf16, 2^-11 fp16). The code
under test computes in fp32: two roundings for ``q*scale + bias``, one for the
weight, one per add of the pool, one or two for the MEAN scale. That is at
most ``n + 6`` fp32 roundings of terms no larger than ``S``; the single
round-to-nearest to the output type adds ``u * |y|`` and scales the fp32 error
by at most ``1 + u``:

    tol = u * |y64| + (n + 6) * 2^-24 * S * (1 + u)   [+ 2^-25 for fp16: subnormals]

A sequence lookup is the same with ``n = 1``. A truncating conversion errs by
up to ``2u * |y|`` and fails this bound on every fixture here
(``TestOracle``), so the bound does tell round-to-nearest from truncation.
"""

import functools

import pytest
import torch

from tests.test_quant_nbit import (
    MIXED,
    MIXED_B,
    MIXED_ROWS,
    SEQ,
    gpu_copy_of,
    make_kjt,
    mixed_dtypes,
    mixed_float_ebc,
    seq_float_ec,
    seq_kjt,
    small_dlrm,
)
from torchrec_amd.inference.modules import quantize_inference_model
from torchrec_amd.modules.embedding_configs import (
    DataType,
    EmbeddingBagConfig,
    EmbeddingConfig,
    PoolingType,
)
from torchrec_amd.modules.embedding_modules import EmbeddingCollection
from torchrec_amd.quant.embedding_modules import (
    EmbeddingBagCollection as QuantEBC,
    EmbeddingCollection as QuantEC,
    QuantTableBatchedEmbeddingBags,
    unpack_codes_nbit,
)
from torchrec_amd.sparse.jagged_tensor import KeyedJaggedTensor

UNIT_ROUNDOFF = {torch.bfloat16: 2.0**-8, torch.float16: 2.0**-11}
OUT_CODE = {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}
LOW = [torch.bfloat16, torch.float16]
MIXED_KEYS = [f for s in MIXED for f in s[3]]


# ---------------------------------------------------------------------------
# float64 oracle from the packed bytes
# ---------------------------------------------------------------------------


def table64(tbe: QuantTableBatchedEmbeddingBags, t: int):
    """(w64, a64), both [rows, D]: the dequantised row and |q*scale| + |bias|."""
    _, rows, D = tbe._specs[t]
    bits = tbe._bits[t]
    packed = tbe.packed_table(t).cpu()
    cb = D * bits // 8
    q = unpack_codes_nbit(packed, D, bits).double()
    sb = packed[:, cb : cb + 4].contiguous().reshape(rows, 2, 2).view(torch.float16)
    sb = sb.reshape(rows, 2).double()
    scale, bias = sb[:, 0:1], sb[:, 1:2]
    return q * scale + bias, (q * scale).abs() + bias.abs()


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
            w = psw[lo:hi].double().unsqueeze(1) if psw is not None else torch.ones(hi - lo, 1, dtype=torch.float64)
            div = float(hi - lo) if mean else 1.0
            y[b] = (w * w64[idx]).sum(0) / div
            S[b] = (w.abs() * a64[idx]).sum(0) / div
            n[b] = hi - lo
        ys.append(y)
        Ss.append(S)
        ns.append(n)
    return torch.cat(ys, 1), torch.cat(Ss, 1), torch.cat(ns, 1)


def seq_oracle(tbe, indices, feat_val_offsets):
    """(y64, S), each [N, D] float64, for a sequence lookup (uniform D)."""
    ys, Ss = [], []
    for f, t in enumerate(tbe._feature_table_map):
        w64, a64 = table64(tbe, t)
        idx = indices[int(feat_val_offsets[f]) : int(feat_val_offsets[f + 1])]
        ys.append(w64[idx])
        Ss.append(a64[idx])
    return torch.cat(ys, 0), torch.cat(Ss, 0)


def tolerance(y64, S, n, dt):
    u = UNIT_ROUNDOFF[dt]
    tol = u * y64.abs() + (n + 6) * 2.0**-24 * S * (1 + u)
    return tol + 2.0**-25 if dt == torch.float16 else tol


def assert_within(out, y64, S, n, dt, what=""):
    assert out.dtype == dt, f"{what}: dtype {out.dtype}, want {dt}"
    assert out.shape == y64.shape, f"{what}: shape {tuple(out.shape)} vs {tuple(y64.shape)}"
    assert float(y64.abs().max()) < 6e4
    err = (out.detach().cpu().double() - y64).abs()
    tol = tolerance(y64, S, n, dt)
    worst = float((err / tol.clamp_min(1e-300)).max()) if err.numel() else 0.0
    print(f"{what} {dt}: worst err/tol {worst:.4f}")
    assert (err <= tol).all(), f"{what} {dt}: worst err/tol {worst}"


def truncate_to(y64, dt):
    """y64 converted to ``dt`` by truncation (toward zero) instead of rounding."""
    if dt == torch.bfloat16:
        bits = y64.float().view(torch.int32) & ~0xFFFF
        return bits.view(torch.float32).to(torch.bfloat16)
    h = y64.to(torch.float16)
    over = h.double().abs() > y64.abs()  # rounded away from zero: one ulp back
    bits = h.view(torch.int16) - over.to(torch.int16)  # sign-magnitude: |h| shrinks
    return bits.view(torch.float16)


# fixtures: module + inputs + oracle, built once per (pooling, weighted)


@functools.lru_cache(maxsize=None)
def mixed_case(mean: bool, weighted: bool):
    pooling = PoolingType.MEAN if mean else PoolingType.SUM
    ebc = mixed_float_ebc(pooling, weighted)
    kjt = make_kjt(MIXED_KEYS, MIXED_ROWS, MIXED_B, weighted)
    make = lambda dt: QuantEBC.from_float(
        ebc, output_dtype=dt, per_table_weight_dtype=mixed_dtypes()
    )
    ref = QuantEBC.from_float(ebc, per_table_weight_dtype=mixed_dtypes())
    psw = kjt.weights() if weighted else None
    oracle = pooled_oracle(ref._tbe, kjt.values(), kjt.offsets(), psw, mean)
    return make, kjt, oracle


INT8_SPECS = [("a0", 20, DataType.INT8, ["g0"]), ("a1", 128, DataType.INT8, ["g1"])]


@functools.lru_cache(maxsize=None)
def int8_case(mean: bool, weighted: bool):
    pooling = PoolingType.MEAN if mean else PoolingType.SUM
    ebc = mixed_float_ebc(pooling, weighted, specs=INT8_SPECS)
    kjt = make_kjt(["g0", "g1"], MIXED_ROWS, MIXED_B, weighted)
    make = lambda dt: QuantEBC.from_float(ebc, output_dtype=dt)
    ref = QuantEBC.from_float(ebc)
    assert ref._tbe._all_int8
    psw = kjt.weights() if weighted else None
    oracle = pooled_oracle(ref._tbe, kjt.values(), kjt.offsets(), psw, mean)
    return make, kjt, oracle


def seq_feat_val_offsets(kjt, F):
    return kjt.offsets()[:: kjt.stride()][: F + 1].contiguous()


@functools.lru_cache(maxsize=None)
def seq_case():
    ec = seq_float_ec()
    kjt = seq_kjt()
    make = lambda dt: QuantEC.from_float(
        ec, output_dtype=dt, per_table_weight_dtype=mixed_dtypes(SEQ)
    )
    ref = QuantEC.from_float(ec, per_table_weight_dtype=mixed_dtypes(SEQ))
    order = [kjt.keys().index(f) for f in ref._feature_names]
    kjt = kjt.permute(order)  # module feature order: rows concatenate in it
    fvo = seq_feat_val_offsets(kjt, len(ref._feature_names))
    oracle = seq_oracle(ref._tbe, kjt.values(), fvo)
    return make, kjt, oracle


@functools.lru_cache(maxsize=None)
def seq_int8_case():
    torch.manual_seed(0)
    tables = [
        EmbeddingConfig(num_embeddings=25, embedding_dim=20, name=n, feature_names=[f])
        for (n, f) in (("s0", "fa"), ("s1", "fb"))
    ]
    ec = EmbeddingCollection(tables=tables)
    kjt = make_kjt(["fa", "fb"], 25, 4)
    make = lambda dt: QuantEC.from_float(ec, output_dtype=dt)
    ref = QuantEC.from_float(ec)
    assert ref._tbe._all_int8
    oracle = seq_oracle(ref._tbe, kjt.values(), seq_feat_val_offsets(kjt, 2))
    return make, kjt, oracle


def seq_rows(out, keys):
    return torch.cat([out[k].values() for k in keys], dim=0)


def empty_bag_columns(kjt, tbe):
    """bool [B, total_D]: columns that belong to an empty bag."""
    B = kjt.stride()
    lengths = kjt.lengths().view(-1, B)
    cols = []
    for f, t in enumerate(tbe._feature_table_map):
        D = tbe._specs[t][2]
        cols.append((lengths[f] == 0).unsqueeze(1).expand(B, D))
    return torch.cat(cols, dim=1)


POOL_MODES = [(False, False), (True, False), (False, True), (True, True)]
POOL_IDS = ["sum", "mean", "sum-weighted", "mean-weighted"]


# ---------------------------------------------------------------------------
# the bound tells rounding from truncation
# ---------------------------------------------------------------------------


class TestOracle:
    @pytest.mark.parametrize("dt", LOW)
    def test_truncation_violates_bound_on_every_fixture(self, dt):
        cases = {
            "mixed-sum": mixed_case(False, False)[2],
            "mixed-mean-weighted": mixed_case(True, True)[2],
            "int8": int8_case(False, False)[2],
        }
        for name, (y, S) in (("seq", seq_case()[2]), ("seq-int8", seq_int8_case()[2])):
            cases[name] = (y, S, torch.ones_like(y))
        for name, (y, S, n) in cases.items():
            tol = tolerance(y, S, n, dt)
            rounded = (y.to(dt).double() - y).abs()
            assert (rounded <= tol).all(), name  # the oracle rounded once passes
            trunc = (truncate_to(y, dt).double() - y).abs()
            n_bad = int((trunc > tol).sum())
            print(f"{name} {dt}: truncation breaks the bound at {n_bad}/{y.numel()} elements")
            assert n_bad > 0, name


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------


class TestOutputDtypeCpu:
    @pytest.mark.parametrize("dt", LOW)
    @pytest.mark.parametrize("mean,weighted", POOL_MODES, ids=POOL_IDS)
    def test_mixed_ebc(self, mean, weighted, dt):
        make, kjt, (y, S, n) = mixed_case(mean, weighted)
        q = make(dt)
        assert q.output_dtype() == dt
        kt = q(kjt)
        assert kt.values().dtype == dt
        assert_within(kt.values(), y, S, n, dt, "cpu mixed")
        assert (kt.values()[empty_bag_columns(kjt, q._tbe)] == 0).all()

    @pytest.mark.parametrize("dt", LOW)
    def test_seq_ec(self, dt):
        make, kjt, (y, S) = seq_case()
        q = make(dt)
        assert q.output_dtype() == dt
        out = q(kjt)
        assert out["fe"].values().shape == (0, 32) and out["fe"].values().dtype == dt
        rows = seq_rows(out, q._feature_names)
        assert_within(rows, y, S, torch.ones_like(y), dt, "cpu seq")

    def test_quantize_inference_model(self):
        model = small_dlrm()
        quantize_inference_model(model, output_dtype=torch.bfloat16, weight_dtype=DataType.INT4)
        q = model.sparse_arch.embedding_bag_collection
        assert isinstance(q, QuantEBC) and q.output_dtype() == torch.bfloat16
        kjt = make_kjt(["f0", "f1"], 50, 3)
        out = model.sparse_arch(kjt)
        assert out.shape == (3, 2, 8) and out.dtype == torch.bfloat16

    @pytest.mark.parametrize("bad", [torch.int8, torch.float64])
    def test_unsupported_dtype_rejected(self, bad):
        with pytest.raises(ValueError):
            QuantTableBatchedEmbeddingBags([("t", 4, 8)], output_dtype=bad)
        cfg = EmbeddingBagConfig(num_embeddings=4, embedding_dim=8, name="t", feature_names=["f"])
        with pytest.raises(ValueError):
            QuantEBC(tables=[cfg], output_dtype=bad)
        with pytest.raises(ValueError):
            QuantEBC.from_float(mixed_float_ebc(), output_dtype=bad)
        with pytest.raises(ValueError):
            QuantEC.from_float(seq_float_ec(), output_dtype=bad)
        with pytest.raises(ValueError):
            quantize_inference_model(small_dlrm(), output_dtype=bad)

    def test_default_is_float32_and_unchanged(self):
        make, kjt, _ = mixed_case(False, False)
        plain = QuantEBC.from_float(mixed_float_ebc(), per_table_weight_dtype=mixed_dtypes())
        explicit = make(torch.float32)
        assert plain.output_dtype() == explicit.output_dtype() == torch.float32
        a, b = plain(kjt).values(), explicit(kjt).values()
        assert a.dtype == b.dtype == torch.float32
        assert torch.equal(a, b)
        smake, skjt, _ = seq_case()
        splain = QuantEC.from_float(seq_float_ec(), per_table_weight_dtype=mixed_dtypes(SEQ))
        assert splain.output_dtype() == torch.float32
        sa, sb = splain(skjt), smake(torch.float32)(skjt)
        for k in sa:
            assert sa[k].values().dtype == torch.float32
            assert torch.equal(sa[k].values(), sb[k].values())


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------


def cuda_kjt(kjt):
    return kjt.to(torch.device("cuda"))


def direct_tbe(specs, dtypes, dt=torch.float32, location="device", seed=0):
    """A GPU quant TBE with random tables; specs are (name, rows, dim)."""
    tbe = QuantTableBatchedEmbeddingBags(
        specs, device=torch.device("cuda"), weight_dtypes=dtypes, output_dtype=dt,
        location=location,
    )
    g = torch.Generator().manual_seed(seed)
    for i, (_, rows, dim) in enumerate(specs):
        tbe.load_float_table(i, torch.randn(rows, dim, generator=g))
    return tbe


def random_bags(specs, B, seed=2, weighted=False):
    g = torch.Generator().manual_seed(seed)
    T = len(specs)
    lengths = torch.randint(0, 4, (T * B,), generator=g)
    lengths[1] = 2  # table 0 holds something
    lengths[-1] = 3  # and so does the last table
    indices = torch.cat(
        [torch.randint(0, specs[i // B][1], (int(l),), generator=g) for i, l in enumerate(lengths)]
    )
    offsets = torch.zeros(T * B + 1, dtype=torch.int64)
    torch.cumsum(lengths, 0, out=offsets[1:])
    psw = torch.rand(indices.numel(), generator=g) if weighted else None
    return indices, offsets, psw


@pytest.mark.gpu
class TestOutputDtypeGpu:
    @pytest.mark.parametrize("dt", LOW)
    @pytest.mark.parametrize("mean,weighted", POOL_MODES, ids=POOL_IDS)
    def test_mixed_pooled(self, mean, weighted, dt):
        """MIXED: the INT4 segment at element 20 (byte 40 of a 2-byte row), a
        33-unit row, narrow tables in a wide launch."""
        make, kjt, (y, S, n) = mixed_case(mean, weighted)
        q_cpu = make(dt)
        q = gpu_copy_of(q_cpu, lambda: make(dt))
        out = q(cuda_kjt(kjt)).values()
        torch.cuda.synchronize()
        assert out.is_cuda
        assert_within(out, y, S, n, dt, "gpu mixed")
        assert (out.cpu()[empty_bag_columns(kjt, q_cpu._tbe)] == 0).all()

    @pytest.mark.parametrize("dt", LOW)
    @pytest.mark.parametrize("mean,weighted", POOL_MODES, ids=POOL_IDS)
    def test_all_int8_pooled(self, mean, weighted, dt):
        make, kjt, (y, S, n) = int8_case(mean, weighted)
        q_cpu = make(dt)
        q = gpu_copy_of(q_cpu, lambda: make(dt))
        assert q._tbe._all_int8
        out = q(cuda_kjt(kjt)).values()
        torch.cuda.synchronize()
        assert_within(out, y, S, n, dt, "gpu int8")
        assert (out.cpu()[empty_bag_columns(kjt, q_cpu._tbe)] == 0).all()

    @pytest.mark.parametrize(
        "D,width", [(1028, DataType.INT8), (2064, DataType.INT2)], ids=["int8-1028", "int2-2064"]
    )
    def test_wide_rows(self, D, width):
        """64 lanes x 8 chunks: the multi-chunk store loop, ragged last chunk."""
        dt = torch.bfloat16
        specs = [("w", D, width, ["h"])]
        ebc = mixed_float_ebc(specs=specs, rows=4)
        make = lambda: QuantEBC.from_float(ebc, output_dtype=dt, weight_dtype=width)
        q_cpu = make()
        q = gpu_copy_of(q_cpu, make)
        kjt = KeyedJaggedTensor(
            keys=["h"], values=torch.tensor([3, 0, 2, 1]), lengths=torch.tensor([3, 0, 1]), stride=3
        )
        y, S, n = pooled_oracle(q_cpu._tbe, kjt.values(), kjt.offsets(), None, False)
        out = q(cuda_kjt(kjt)).values()
        torch.cuda.synchronize()
        assert_within(out, y, S, n, dt, f"gpu wide D={D}")
        assert (out[1] == 0).all()

    @pytest.mark.parametrize("dt", LOW)
    def test_seq(self, dt):
        """SEQ: D_out = 32 at INT4/INT2; one feature has no values."""
        make, kjt, (y, S) = seq_case()
        q_cpu = make(dt)
        q = gpu_copy_of(q_cpu, lambda: make(dt))
        out = q(cuda_kjt(kjt))
        torch.cuda.synchronize()
        assert out["fe"].values().shape == (0, 32) and out["fe"].values().dtype == dt
        assert_within(seq_rows(out, q._feature_names), y, S, torch.ones_like(y), dt, "gpu seq")

    @pytest.mark.parametrize("dt", LOW)
    def test_seq_all_int8_d20(self, dt):
        """D_out = 20: rows start at byte 40*n, 8-byte aligned only."""
        make, kjt, (y, S) = seq_int8_case()
        q_cpu = make(dt)
        q = gpu_copy_of(q_cpu, lambda: make(dt))
        assert q._tbe._all_int8
        out = q(cuda_kjt(kjt))
        torch.cuda.synchronize()
        assert_within(seq_rows(out, q._feature_names), y, S, torch.ones_like(y), dt, "gpu seq8")

    @pytest.mark.parametrize("dt", [torch.float32] + LOW)
    def test_seq_nbit_respects_row_and_output_width(self, dt):
        """A D=8 table in a D_out=20 output (rows 8-byte aligned only): columns
        past D are not written, for every output type as for fp32. The output
        is allocated inside the op, so the guard is a sentinel-filled block of
        the same size released just before the call; when the allocator hands
        the op that block, the columns past D must still hold the sentinel."""
        specs = [("a", 12, 8), ("b", 9, 16)]
        tbe = direct_tbe(specs, [DataType.INT4, DataType.INT2])
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
            assert (out[:n0, 8:] == -7.0).all()  # past table a's D
            assert (out[n0:, 16:] == -7.0).all()  # past table b's D
        if dt != torch.float32:
            one = torch.ones(N, 1, dtype=torch.float64)
            assert_within(out[:n0, :8], w64a[indices[:n0]], a64a[indices[:n0]], one[:n0], dt, "a")
            assert_within(out[n0:, :16], w64b[indices[n0:]], a64b[indices[n0:]], one[n0:], dt, "b")
            # D_out narrower than table b's D: the row is cut at D_out
            cut = torch.ops.trec_amd.tbe_forward_seq_nbit(*args, 8, 2, OUT_CODE[dt])
            torch.cuda.synchronize()
            assert cut.shape == (N, 8)
            assert torch.equal(cut[:n0], out[:n0, :8]) and torch.equal(cut[n0:], out[n0:, :8])

    def test_ops_default_code_and_bad_code(self):
        """output_dtype=0 given explicitly is the call without it; 7 is refused."""
        specs = [("a", 12, 20), ("b", 9, 128)]
        tbe = direct_tbe(specs, [DataType.INT8, DataType.INT8])
        B = 4
        indices, offsets, psw = random_bags(specs, B, weighted=True)
        idx, off, psw = indices.cuda(), offsets.cuda(), psw.cuda()
        bits = tbe._weight_bits_t
        fvo = off[::B][:3].contiguous()
        calls = {
            "tbe_forward_pooled_int8": (
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._feat_table_t,
                tbe._d_out_offsets, idx, off, psw, B, 148, 128, True),
            "tbe_forward_pooled_nbit": (
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, bits, tbe._feat_table_t,
                tbe._d_out_offsets, idx, off, psw, B, 148, 32, True),
            "tbe_forward_seq_int8": (
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._feat_table_t, fvo,
                idx, 128, 128),
            "tbe_forward_seq_nbit": (
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, bits, tbe._feat_table_t, fvo,
                idx, 128, 32),
        }
        n0 = int(fvo[1])
        for name, args in calls.items():
            op = getattr(torch.ops.trec_amd, name)
            a, b = op(*args), op(*args, 0)
            torch.cuda.synchronize()
            assert a.dtype == b.dtype == torch.float32
            if "seq" in name:  # a D=20 row fills the first 20 of 128 columns
                assert torch.equal(a[:n0, :20], b[:n0, :20]) and torch.equal(a[n0:], b[n0:])
            else:
                assert torch.equal(a, b)
            assert float(a.abs().max()) > 0
            with pytest.raises(RuntimeError, match="output_dtype"):
                op(*args, 7)

    @pytest.mark.parametrize("dt", [torch.float32] + LOW)
    def test_ops_empty_batch(self, dt):
        specs = [("a", 12, 20), ("b", 9, 128)]
        tbe = direct_tbe(specs, [DataType.INT8, DataType.INT8])
        dev = torch.device("cuda")
        none = torch.empty(0, dtype=torch.int64, device=dev)
        off0 = torch.zeros(1, dtype=torch.int64, device=dev)
        fvo0 = torch.zeros(3, dtype=torch.int64, device=dev)
        code = OUT_CODE[dt]
        bits = tbe._weight_bits_t
        outs = [
            torch.ops.trec_amd.tbe_forward_pooled_int8(
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._feat_table_t,
                tbe._d_out_offsets, none, off0, tbe._empty_f, 0, 148, 128, False, code),
            torch.ops.trec_amd.tbe_forward_pooled_nbit(
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, bits, tbe._feat_table_t,
                tbe._d_out_offsets, none, off0, tbe._empty_f, 0, 148, 32, False, code),
            torch.ops.trec_amd.tbe_forward_seq_int8(
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, tbe._feat_table_t, fvo0,
                none, 128, 128, code),
            torch.ops.trec_amd.tbe_forward_seq_nbit(
                tbe.qweights, tbe._table_byte_offsets, tbe._dims_t, bits, tbe._feat_table_t,
                fvo0, none, 128, 32, code),
        ]
        torch.cuda.synchronize()
        for o, shape in zip(outs, [(0, 148), (0, 148), (0, 128), (0, 128)]):
            assert o.dtype == dt and o.shape == shape and o.is_cuda

    def test_managed_matches_device(self):
        """Pinned-host packed tables at bf16 match HBM tables bit for bit."""
        specs = [("t0", 50, 64), ("t1", 30, 128)]
        dts = [DataType.INT4, DataType.INT4]
        dev = direct_tbe(specs, dts, torch.bfloat16)
        uvm = QuantTableBatchedEmbeddingBags(
            specs, device=torch.device("cuda"), location="managed", weight_dtypes=dts,
            output_dtype=torch.bfloat16,
        )
        assert not uvm.qweights.is_cuda and uvm.qweights.is_pinned()
        for i in range(len(specs)):
            uvm.packed_table(i).copy_(dev.packed_table(i).cpu())
        indices, offsets, _ = random_bags(specs, 8, seed=1)
        out_dev = dev(indices.cuda(), offsets.cuda())
        out_uvm = uvm(indices.cuda(), offsets.cuda())
        torch.cuda.synchronize()
        assert out_dev.dtype == out_uvm.dtype == torch.bfloat16
        assert float(out_dev.float().abs().max()) > 0
        assert torch.equal(out_dev, out_uvm)

    def test_graph_capture_replays_eager(self):
        """One capture and replay of the bf16 pooled forward (a single kernel,
        no parallel branches) reproduces the eager output bit for bit."""
        make, kjt, _ = mixed_case(False, False)
        q = gpu_copy_of(make(torch.bfloat16), lambda: make(torch.bfloat16))
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
        assert out.dtype == torch.bfloat16
        assert float(eager.float().abs().max()) > 0
        assert torch.equal(out, eager)
